"""The distortion loss on the MI355X (csrc/distortion.hip k_distortion_fwd / k_distortion_bwd,
raymarching.distortion_loss, render(distortion=True), optim.lambda_distortion).  References: tests/distortion_reference.py
(float64: the O(k^2) double sum of the definition and its torch autograd gradient; the op-level case and the preconditions
asserted on it before anything is compared: sigma dt <= 1.5 except the one huge sample, every reference T at least 1e-3
(relative) away from T_thresh, no sample left out).

The tolerance rule (1, 2 and the renderer's loss).  Per ray with k samples, e32 = the error of the float32 restatement of
the header's arithmetic against float64 ON THAT RAY (tests/test_distortion_cpu.py measures and prints it):
  forward   |loss - ref64| <= 4 e32 + COMPOSITE_TOL(k) max_i m_i,
  backward  max_s |dsigma - ref64| <= 4 e32 + COMPOSITE_TOL(k) |go| max_i dt_i max_i m_i
with COMPOSITE_TOL(k) = 32 2^-24 (k + 1), the project's compositing bound (tests/test_gpu_latent_tune.py).  The factor 4
is the rule of tests/test_gpu_orient.py item 3 (the kernel's scans add as a tree where the restatement adds left to
right, and expf is not numpy's exp: the same arithmetic with other roundings).  The second addend carries the weights'
own error through: a weight is good to COMPOSITE_TOL(k) relative, the weights sum to <= 1, so loss <= max m and
dL/dtau <= ~ max m per unit weight error, dsigma = go dt dL/dtau (with shifted mid-points m = (t - t_0) + dt / 2).

1. Op forward: the rule; the empty ray gives exactly 0, ids of no ray are not touched (0 through the binding); ray_sums
   of the empty ray are zeros; two runs give the same bits.
2. Op backward: the rule per sample; rows behind the cut are exactly 0, rows outside every span keep the sentinel, two
   runs give the same bits, the huge-tau ray gives finite values.
3. Binding: torch.autograd.grad through raymarching.distortion_loss equals the raw ABI calls bit for bit.
4. Renderer (the f32 scene of tests/shading_reference.py; albedo, lambertian and latent_tune forms): image, depth and
   weights_sum are the distortion=False render's bits; loss_distortion against the float64 double sum on the march's own
   samples under the rule; parameter gradients of (image . G + lambda mean(loss_distortion)) equal those of image . G
   plus those of the term alone per tensor within 4 x (the albedo render's worst figure against the oracle) x max |sum|,
   the rule of test_f32_training_render_matches_the_oracle.
5. Trainer (the configuration of tests/test_gpu_orient.py's trainer tests: 32 x 32, 12 steps; lambda_distortion = 1e-2):
   captured == eager bit for bit (fp16 true and false), the cached constant is float32(lambda / rays), lambda = 0 is the
   default's path bit for bit AND call for call (the library's call hook: the same entry points the same number of
   times; with the term exactly lnerf_distortion_forward / _backward more), the term acts, step_loss rises by
   lambda mean(loss_distortion), and one run combines start_shading_iter, lambda_orient and lambda_distortion.
Every test prints the figures it asserts on (run with -s).
Measured on the MI355X: op forward, largest error 1.6e-7 (127 samples) at a tolerance of 6.0e-4, worst ratio error /
tolerance 0.001 (the 3-sample ray: 2.3e-10 at 4.5e-7), the float32 restatement's own errors 3e-12 .. 3.7e-7; op backward,
largest error 1.4e-8 (200 samples, max |dsigma| 1.9e-2) at 3.0e-4, worst ratio 0.008, the restatement's 5e-13 .. 1.8e-8;
renderer (216 samples, largest sigma dt 6.5), loss_distortion mean 5.0661e-2 against 5.0661e-2, worst ray 2.3e-8 at
8.0e-6 (ratio 0.003), the same figures for the three forms; gradients, worst tensor |both - (image + term)| / max |sum|
2.9e-7 albedo, 4.1e-7 lambertian, 3.6e-7 latent_tune against r = 3.78e-4; trainer, 268 entry-point calls in 12 steps
without the term and 274 with it (3 + 3), all 7 parameter tensors differ, step_loss 8.643e-4 = 1.459e-4 + 7.184e-4."""
import collections
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import distortion_reference as D
from tests import shading_reference as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
W_NAMES = R.W_NAMES
G, HW, MAX_STEPS, EPS, AMBIENT = (R.SCENE[k] for k in ("G", "HW", "MAX_STEPS", "EPS", "AMBIENT"))
LIGHT = list(R.SCENE["LIGHT"])
S1, S2 = 123.0, -321.0      # sentinels of the forward / backward outputs


def COMPOSITE_TOL(k):          # (tests/test_gpu_latent_tune.py)
    return 32 * ULP * (np.asarray(k, dtype=np.float64) + 1)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(torch.as_tensor(b)))


def _tolerances(sig, deltas, rays, n_ids, d_loss):
    """The rule of the module docstring on one input -> dict(fwd [n_ids], bwd [n_ids], loss64, grad64 [m], cnt [n_ids],
    e = the float32 restatement's figures)."""
    e = D.f32_errors(sig, deltas, rays, n_ids, d_loss)
    cnt = np.zeros(n_ids)
    cnt[rays[:, 0]] = rays[:, 2]
    rows, _ = D.span_rows(rays)
    mmax = D.per_ray_max(e["r32"]["m"].astype(np.float64), rays, n_ids)
    dtmax = D.per_ray_max(np.asarray(deltas, dtype=np.float64)[rows, 0], rays, n_ids)
    go = np.abs(np.asarray(d_loss, dtype=np.float64))
    return dict(fwd=4 * e["fwd"] + COMPOSITE_TOL(cnt) * mmax, bwd=4 * e["bwd"] + COMPOSITE_TOL(cnt) * go * dtmax * mmax,
                loss64=e["loss64"], grad64=e["grad64"], cnt=cnt, e=e)


# ------------------------------------------------------------------------------ 1 - 3: the kernels
class _Op:
    """The op-level case on the device, the two entry points on it, and the reference figures (computed once)."""

    def __init__(self, dev):
        self.k = k = D.op_case()
        self.w, self.T, self.tau = D.check_case(k)        # the preconditions, before anything is compared
        self.dev = dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.sig, self.deltas, self.rays, self.d_loss = t(k["sig"]), t(k["deltas"]), t(k["rays"]), t(k["d_loss"])
        self.tol = _tolerances(k["sig"], k["deltas"], k["rays"], k["n_ids"], k["d_loss"])
        _, self.ids = D.span_rows(k["rays"])

    def forward(self):
        from src.latent_nerf.raymarching import backend as B
        from src.latent_nerf.raymarching.raymarching import _p, _stream
        k = self.k
        loss = torch.full((k["n_ids"],), S1, device=self.dev)
        sums = torch.full((k["n_ids"], 2), S1, device=self.dev)
        B.call("lnerf_distortion_forward", _p(self.sig), _p(self.deltas), _p(self.rays), k["N"], D.T_THRESH, _p(loss),
               _p(sums), _stream())
        torch.cuda.synchronize()
        return loss, sums

    def backward(self, loss, sums, d_loss=None):
        from src.latent_nerf.raymarching import backend as B
        from src.latent_nerf.raymarching.raymarching import _p, _stream
        k = self.k
        out = torch.full((k["cap"],), S2, device=self.dev)
        B.call("lnerf_distortion_backward", _p(self.sig), _p(self.deltas), _p(self.rays), k["N"], D.T_THRESH,
               _p(self.d_loss if d_loss is None else d_loss), _p(loss), _p(sums), _p(out), _stream())
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def op(dev):
    return _Op(dev)


def test_op_forward(op):
    k, tol = op.k, op.tol
    loss, sums = op.forward()
    got = loss.cpu().double().numpy()
    present = np.zeros(k["n_ids"], bool)
    present[k["ids"]] = True
    assert (got[~present] == S1).all() and bool((sums.cpu().numpy()[~present] == S1).all())   # ids of no ray: not touched
    err = np.where(present, np.abs(got - tol["loss64"]), 0.0)
    ratio = np.where(present & (tol["fwd"] > 0), err / np.where(tol["fwd"] > 0, tol["fwd"], 1.0), 0.0)
    for rid in k["ids"]:
        print("ray id %2d (%3d samples): loss %.6e, ref %.6e, error %.3e, f32 restatement %.3e, tolerance %.3e"
              % (rid, tol["cnt"][rid], got[rid], tol["loss64"][rid], err[rid], tol["e"]["fwd"][rid], tol["fwd"][rid]))
    print("forward: worst ratio error / tolerance %.3f (ray id %d)" % (float(ratio.max()), int(ratio.argmax())))
    assert (err <= tol["fwd"]).all(), float((err - tol["fwd"]).max())
    empty = int(k["ids"][D.R_EMPTY])
    assert got[empty] == 0.0 and tol["cnt"][empty] == 0 and not sums[empty].any()         # the empty ray: written, 0
    assert np.isfinite(got).all() and float(tol["loss64"].max()) > 0.1
    # the totals the backward reads: sum of w and of w m per ray (the restatement's, to the compositing bound)
    s32 = tol["e"]["r32"]["sums"].astype(np.float64)
    ds = np.abs(sums.cpu().double().numpy() - s32)[present]
    assert (ds <= (COMPOSITE_TOL(tol["cnt"]) * np.maximum(1.0, np.abs(s32).max(-1)))[present][:, None]).all()
    again, sums2 = op.forward()
    assert _same_bits(again, loss) and _same_bits(sums2, sums)


def test_op_backward(op):
    k, tol, M = op.k, op.tol, op.k["M"]
    loss, sums = op.forward()
    out = op.backward(loss, sums)
    got = out[:M].cpu().double().numpy()                   # (the spans are rows 0 .. M - 1 in ray order)
    assert bool((out[M:] == S2).all())                     # rows outside every span keep the sentinel
    assert np.isfinite(got).all()
    err = np.abs(got - tol["grad64"])
    worst = D.per_ray_max(err, k["rays"], k["n_ids"])
    gmax = D.per_ray_max(tol["grad64"], k["rays"], k["n_ids"])
    for rid in k["ids"]:
        print("ray id %2d (%3d samples): max |dsigma| %.3e, worst error %.3e, f32 restatement %.3e, tolerance %.3e"
              % (rid, tol["cnt"][rid], gmax[rid], worst[rid], tol["e"]["bwd"][rid], tol["bwd"][rid]))
    ratio = np.where(tol["bwd"] > 0, worst / np.where(tol["bwd"] > 0, tol["bwd"], 1.0), 0.0)
    print("backward: worst ratio error / tolerance %.3f (ray id %d)" % (float(ratio.max()), int(ratio.argmax())))
    assert (err <= tol["bwd"][op.ids]).all(), float((err - tol["bwd"][op.ids]).max())
    # behind the cut: exact zeros (the killed ray's tail and everything behind the huge sample)
    dead = op.T < D.T_THRESH
    assert int(dead.sum()) > 100 and (got[dead] == 0).all() and not tol["grad64"][dead].any()
    at = np.concatenate([[0], np.cumsum(k["rays"][:, 2])])
    huge = got[at[D.R_HUGE]:at[D.R_HUGE + 1]]
    assert np.isfinite(huge).all() and (huge[:D.I_HUGE + 1] != 0).any() and (huge[D.I_HUGE + 1:] == 0).all()
    assert float(np.abs(tol["grad64"]).max()) > 1e-3
    assert _same_bits(op.backward(loss, sums), out)


def test_binding(op):
    """The autograd node hands the kernels' results through: ids of no ray are 0, n_ids defaults to N."""
    from src.latent_nerf.raymarching import raymarching as rm
    k, M = op.k, op.k["M"]
    loss_k, sums_k = op.forward()
    want = op.backward(loss_k, sums_k)
    sig = op.sig.clone().requires_grad_()
    loss = rm.distortion_loss(sig, op.deltas, op.rays, D.T_THRESH, k["n_ids"])
    assert loss.shape == (k["n_ids"],) and loss.requires_grad
    present = torch.zeros(k["n_ids"], dtype=torch.bool)
    present[torch.from_numpy(k["ids"])] = True
    assert _same_bits(loss[present.to(op.dev)], loss_k[present.to(op.dev)])
    assert bool((loss[~present.to(op.dev)] == 0).all())                                    # ids of no ray: exactly 0
    grad, = torch.autograd.grad(loss, sig, op.d_loss)
    assert _same_bits(grad[:M], want[:M])
    # n_ids defaults to the number of rays (here with ids 0 .. N - 1, so that they fit); a node without an upstream
    # gradient launches nothing and hands none on
    rays2 = op.rays.clone()
    rays2[:, 0] = torch.arange(k["N"], dtype=torch.int32, device=op.dev)
    sig2 = op.sig.clone().requires_grad_()
    loss2 = rm.distortion_loss(sig2, op.deltas, rays2)
    assert loss2.shape == (k["N"],) and _same_bits(loss2, loss_k[torch.from_numpy(k["ids"]).to(op.dev)])
    g2, = torch.autograd.grad((sig2 * 2.0).sum() + 0.0 * loss2.detach().sum(), sig2)
    assert bool((g2 == 2.0).all())
    with pytest.raises(ValueError, match="n_ids"):
        rm.distortion_loss(sig, op.deltas, op.rays, D.T_THRESH, k["N"] - 1)
    with pytest.raises(ValueError, match="deltas"):
        rm.distortion_loss(sig, op.deltas[:k["cap"] - 1], op.rays)


# ------------------------------------------------------------------------------ 4. renderer
LAMBDA_RENDER = 4.0       # weight of mean(loss_distortion) beside image . G in the gradient comparison


def _grads(net):
    out = {}
    for name, p in net.named_parameters():
        if p.grad is not None:
            out[name] = p.grad.detach().clone()
        p.grad = None
    return out


@pytest.fixture(scope="module")
def scene(dev):
    """The f32 net of the shading tests, its latent_tune twin, and the ALBEDO yardstick of the gradient bound, once."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    net, bits = R.scene_net(O, "f32")
    net = net.to(dev).train()
    ro, rd, bg, g = R.scene_rays(O)
    lv, table, params = R.scene_oracle_leaves(O, net)
    out = net.render(ro[None].to(dev), rd[None].to(dev), bg_color=bg.to(dev), perturb=False, max_steps=MAX_STEPS)
    out["image"].backward(g.to(dev))
    got = _grads(net)
    tab = table.double().requires_grad_()
    par = {k: v.double().requires_grad_() for k, v in params.items()}
    ref = R.render_shaded_oracle(O, ro, rd, tab, par, lv, bits, light=LIGHT, ambient=AMBIENT, textureless=False, eps=EPS, G=G,
                                 max_steps=MAX_STEPS, bg_color=bg, shaded=False)
    ref["image"].backward(g[0])
    assert int(out["counter"][0]) == ref["M"]
    ref_grads = {"encoder.embeddings": tab.grad, **{k: par[k].grad for k in W_NAMES}}
    yard = {k: float((got[k].cpu().double() - ref_grads[k]).abs().max()) / float(ref_grads[k].abs().max())
            for k in ref_grads}
    cfg = RenderConfig(grid_size=G, train_h=HW, train_w=HW, mlp_precision="f32", table_dtype="f32", gridtype="hash",
                       nerf_type=NeRFType("latent_tune"))
    tune = NeRFNetwork(cfg, log2_hashmap_size=R.SCENE["LOG2_T"])
    missing, unexpected = tune.load_state_dict({k: v.cpu() for k, v in net.state_dict().items()}, strict=False)
    assert list(missing) == ["decoder"] and not unexpected
    tune = tune.to(dev).train()
    return dict(net=net, tune=tune, ro=ro, rd=rd, bg=bg, g=g, yard=yard)


@pytest.mark.parametrize("form", ["albedo", "lambertian", "latent_tune"])
def test_render_with_distortion(dev, scene, form):
    c = scene
    net, N = (c["tune"] if form == "latent_tune" else c["net"]), HW * HW
    net.train()
    C = 3 if form == "latent_tune" else 4
    ro, rd = c["ro"][None].to(dev), c["rd"][None].to(dev)
    bg, g = c["bg"][:, :C].contiguous().to(dev), c["g"][..., :C].contiguous().to(dev)
    kw = dict(bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    if form == "lambertian":
        kw.update(shading="lambertian", light_d=LIGHT, ambient_ratio=AMBIENT, normal_eps=EPS)
    const = torch.full((1, N), LAMBDA_RENDER / N, device=dev)
    plain = net.render(ro, rd, **kw)
    assert "loss_distortion" not in plain and plain["image"].shape == (1, N, C)
    plain["image"].backward(g)
    g_image = _grads(net)
    out = net.render(ro, rd, distortion=True, **kw)
    assert out["loss_distortion"].shape == out["weights_sum"].shape == (1, N) and out["loss_distortion"].requires_grad
    for key in ("image", "depth", "weights_sum"):
        assert torch.equal(out[key], plain[key]) and _same_bits(out[key], plain[key]), key
    torch.autograd.backward([out["image"], out["loss_distortion"]], [g, const])
    g_both = _grads(net)
    alone = net.render(ro, rd, distortion=True, **kw)
    assert _same_bits(alone["loss_distortion"], out["loss_distortion"])
    alone["loss_distortion"].backward(const)
    g_term = _grads(net)
    # the loss against the float64 double sum on the march's own samples, under the rule of the module docstring
    rays = out["rays"].cpu().numpy()
    assert rays.shape == (N, 3) and int(rays[:, 2].sum()) == int(out["counter"][0])
    sig, deltas = out["sigmas"].detach().cpu().numpy(), out["deltas"].cpu().numpy()
    d_loss = np.full(N, LAMBDA_RENDER / N, np.float32)
    tol = _tolerances(sig, deltas, rays, N, d_loss)
    w, T, tau = D.weights(sig, deltas, rays)
    margin = float((np.abs(T - D.T_THRESH) / D.T_THRESH).min())
    assert margin >= 1e-3, margin                          # the GPU and the reference agree on which samples are live
    got = out["loss_distortion"][0].detach().cpu().double().numpy()
    err = np.abs(got - tol["loss64"])
    ratio = np.where(tol["fwd"] > 0, err / np.where(tol["fwd"] > 0, tol["fwd"], 1.0), 0.0)
    print("%s loss_distortion: mean %.4e (ref %.4e), %d samples, largest sigma dt %.2f, worst ray error %.3e at a tolerance "
          "of %.3e (ratio %.3f)" % (form, got.mean(), tol["loss64"].mean(), len(w), float(tau.max()), float(err.max()),
                                    float(tol["fwd"][err.argmax()]), float(ratio.max())))
    assert (err <= tol["fwd"]).all(), float((err - tol["fwd"]).max())
    assert (got[tol["cnt"] == 0] == 0).all() and (tol["cnt"] == 0).any() and float(tol["loss64"].mean()) > 1e-5
    # gradients: (image + term) = (image alone) + (term alone), per tensor
    r = 4 * max(c["yard"].values())
    assert set(g_both) == set(g_image) and set(g_term) <= set(g_both) and "encoder.embeddings" in g_term
    for name in sorted(g_both):
        want = g_image[name].double() + (g_term[name].double() if name in g_term else 0.0)
        fig = float((g_both[name].double() - want).abs().max()) / float(want.abs().max())
        share = float(g_term[name].abs().max()) / float(want.abs().max()) if name in g_term else 0.0
        print("%s d%-18s: max |both - (image + term)| / max |sum| = %.3e (r = %.3e); the term's share %.3e"
              % (form, name, fig, r, share))
        assert fig <= r, (name, fig, r)
    assert float(g_term["encoder.embeddings"].abs().max()) > 0
    # the colour-only parameters get nothing from the term
    if "decoder" in g_both:
        assert "decoder" not in g_term or not bool(g_term["decoder"].any())


# ------------------------------------------------------------------------------ 5. trainer
TRAINER_SEED, TRAINER_STEPS, TRAINER_START = 1, 12, 3      # (tests/test_gpu_orient.py)
LAMBDA = 1e-2


def _trainer_cfg(root, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(root), "render.train_h": 32, "render.train_w": 32,
            "render.eval_h": 32, "render.eval_w": 32, "render.grid_size": 64, "optim.iters": TRAINER_STEPS,
            "optim.lr": 5e-3, "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1,
            "optim.seed": TRAINER_SEED, "guide.text": "a lego man", "log.quiet": True}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """name, overrides -> (trainer, parameters, exp_avg, exp_avg_sq, calls) of one 12-step run, each configuration trained
    once; calls = how often every entry point of the library was called during the run."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.training.trainer import Trainer
    root, runs = tmp_path_factory.mktemp("distortion"), {}

    def run(name, **over):
        if name not in runs:
            torch.manual_seed(7)
            torch.cuda.manual_seed(7)
            tr = Trainer(_trainer_cfg(root, **{"log.exp_name": name, **over}), device=dev)
            calls = collections.Counter()
            B.set_profile_hook(lambda entry, when: calls.update([entry] if when == "pre" else []))
            try:
                tr.train()
            finally:
                B.set_profile_hook(None)
            torch.cuda.synchronize()
            st = tr.optimizer.state_dict()
            params = [p.detach().clone() for grp in tr.nerf.get_params(1.0) for p in grp["params"]]
            runs[name] = (tr, params, [t.clone() for t in st["exp_avg"]], [t.clone() for t in st["exp_avg_sq"]], calls)
        return runs[name]

    return run


def _assert_same_run(a, b):
    for what, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), a[1:4], b[1:4]):
        assert len(x) == len(y)
        for i, (s, t) in enumerate(zip(x, y)):
            assert _same_bits(s, t), (what, i)


@pytest.mark.parametrize("fp16", [True, False])
def test_trainer_captured_equals_eager_with_the_term(dev, trained, fp16):
    runs = {}
    for graph in (True, False):
        runs[graph] = trained("d%d%d" % (graph, fp16), **{"optim.fp16": fp16, "optim.graph_step": graph,
                                                         "optim.lambda_distortion": LAMBDA})
        tr = runs[graph][0]
        assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == 0, tr.graph_stats
        assert all(bool(torch.isfinite(p).all()) for p in runs[graph][1])
        assert list(tr._distortion_const) == [(1, 32 * 32)]                   # one constant, allocated before the captures
        assert float(tr._distortion_const[(1, 1024)][0, 0]) == np.float32(LAMBDA / 1024)
        assert bool((tr._distortion_const[(1, 1024)] == float(np.float32(LAMBDA / 1024))).all())
    tr = runs[True][0]
    assert tr.graph_stats["captures"] == 1 and tr._whole, tr.graph_stats      # still ONE graph launch per step
    assert tr.graph_stats["replayed_steps"] + tr.graph_stats["eager_steps"] == TRAINER_STEPS
    assert tr.graph_stats["replayed_steps"] >= TRAINER_STEPS - 4
    assert runs[False][0].graph_stats["captures"] == 0
    _assert_same_run(runs[True], runs[False])


def test_trainer_the_term_acts_and_zero_is_the_default_path(dev, trained):
    on = trained("d11", **{"optim.fp16": True, "optim.graph_step": True, "optim.lambda_distortion": LAMBDA})
    zero = trained("zero", **{"optim.fp16": True, "optim.graph_step": True, "optim.lambda_distortion": 0.0})
    default = trained("default", **{"optim.fp16": True, "optim.graph_step": True})
    assert default[0].cfg.optim.lambda_distortion == 0.0 and not default[0]._distortion_const
    assert not zero[0]._distortion_const
    _assert_same_run(zero, default)
    # lambda = 0 issues the default's launches: the same entry points, the same number of times; with the term exactly
    # the two kernels more, once per render / backward that ran on the host (eager steps and the capture)
    assert zero[4] == default[4] and sum(zero[4].values()) > 50, (zero[4], default[4])
    new = {"lnerf_distortion_forward", "lnerf_distortion_backward"}
    print("entry-point calls of the 12-step run: %d without the term, %d with it; the term's: %s"
          % (sum(zero[4].values()), sum(on[4].values()), {k: on[4][k] for k in sorted(new)}))
    assert not new & set(zero[4]) and set(on[4]) == set(zero[4]) | new
    assert on[4]["lnerf_distortion_forward"] == on[4]["lnerf_composite_rays_train_forward"] > 0
    assert on[4]["lnerf_distortion_backward"] == on[4]["lnerf_composite_rays_train_backward"] > 0
    assert {k: v for k, v in on[0].graph_stats.items() if k != "host_s"} \
        == {k: v for k, v in zero[0].graph_stats.items() if k != "host_s"}
    assert {k: v for k, v in on[4].items() if k not in new} == dict(zero[4])
    differ = [i for i, (x, y) in enumerate(zip(on[1], zero[1])) if not torch.equal(x, y)]
    print("parameters that differ between lambda_distortion = 1e-2 and 0: %s of %d" % (differ, len(on[1])))
    assert differ
    # the logged value of the auxiliary terms carries the term
    from src.latent_nerf.training.guidance import sparsity_loss
    tr = on[0]
    tr.nerf.train()
    with torch.cuda.stream(tr.stream):
        out, _ = tr._render_train(tr._camera())
        with_term = float(tr.step_loss(out))
        assert out["loss_distortion"].shape == (1, 1024)
        want = float(LAMBDA * out["loss_distortion"].detach().mean())
        base = float(tr.cfg.optim.lambda_sparsity * sparsity_loss(out["weights_sum"].detach()))
    zero[0].nerf.train()
    with torch.cuda.stream(zero[0].stream):
        out0, _ = zero[0]._render_train(zero[0]._camera())
        assert "loss_distortion" not in out0
    torch.cuda.synchronize()
    print("step_loss %.6e = sparsity %.6e + lambda mean(loss_distortion) %.6e" % (with_term, base, want))
    assert want > 0 and abs(with_term - (base + want)) <= 1e-6 * max(abs(with_term), 1e-6)


def test_trainer_shading_orient_and_distortion_together(dev, trained):
    from src.latent_nerf.training import shading as SH
    n_shaded = sum(k != "albedo" for k in SH.schedule(TRAINER_SEED, 1, TRAINER_STEPS, TRAINER_START))
    over = {"optim.fp16": True, "optim.start_shading_iter": TRAINER_START, "optim.lambda_orient": 1e-2,
            "optim.lambda_distortion": LAMBDA}
    a = trained("all1", **{"optim.graph_step": True, **over})
    b = trained("all0", **{"optim.graph_step": False, **over})
    for tr in (a[0], b[0]):
        assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == n_shaded > 0, tr.graph_stats
        assert list(tr._distortion_const) == [(1, 1024)] and list(tr._orient_const) == [(1, 1024)]
    assert a[0].graph_stats["captures"] == 2 and a[0]._gstep_shaded is not None, a[0].graph_stats
    _assert_same_run(a, b)
    assert all(bool(torch.isfinite(p).all()) for p in a[1])
    # both terms are in a shaded render's dict, the distortion term alone in a plain one
    tr = a[0]
    tr.nerf.train()
    with torch.cuda.stream(tr.stream):
        tr._shaded = True
        out, _ = tr._render_train(tr._camera())
        tr._shaded = False
        out0, _ = tr._render_train(tr._camera())
    torch.cuda.synchronize()
    assert "loss_orient" in out and "loss_distortion" in out and "loss_orient" not in out0 and "loss_distortion" in out0
    only_orient = trained("orient", **{"optim.graph_step": True, "optim.fp16": True,
                                       "optim.start_shading_iter": TRAINER_START, "optim.lambda_orient": 1e-2})
    assert [i for i, (x, y) in enumerate(zip(a[1], only_orient[1])) if not torch.equal(x, y)]
