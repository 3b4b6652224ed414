"""The composited normal image and the 2D normal-smoothness term on the MI355X (csrc/normal_image.hip,
raymarching.normal_image / image_smooth, render(normal_image=True), optim.lambda_normal_smooth).  Reference:
tests/normal_image_reference.py (float64 plain form, validated against central differences in
tests/test_normal_smooth_cpu.py; the op-level case with cnt = 0, 1, 3, 63, 64, 65, 130, permuted ids, one id of no ray, a
ray that goes opaque mid-span, a sample with six equal offsets, a sample with a NaN offset; its preconditions are asserted
before anything is compared, and NO sample is left out of any comparison).

The tolerance rule (the project's, tests/test_gpu_distortion.py).  Per ray with k samples, e32 = the error of the float32
restatement of the header's arithmetic against float64 ON THAT RAY, COMPOSITE_TOL(k) = 32 2^-24 (k + 1):
  forward        max_a |N_a - ref64|        <= 4 e32 + COMPOSITE_TOL(k) * 1              (|n| <= 1, sum w <= 1)
  centre rows    |dsigmas7[7 s] - ref64|    <= 4 e32 + COMPOSITE_TOL(k) |dN| max dt density_scale
  offset rows    |dsigmas7[7 s + j] - ref64| <= 4 e32(s) + COMPOSITE_TOL(k) |dN| inv_2eps r(s)
with |dN| the Euclidean length of the ray's upstream gradient and max dt over the ray's samples.  The offset rows are
held to their OWN sample's figures -- e32(s) the restatement's error on the six rows of sample s, r(s) = 1 / |g| of sample
s -- not to the ray's largest: r is 1e10 on the degenerate and the NaN sample (their rows ARE that large, and are compared
like every other row), and the ray's maximum would excuse every other sample of those two rays.

1. Op forward / backward at density_scale 1 and 0.5: the rule; the empty ray writes zeros, the id of no ray and the rows
   outside every span keep their poison; rows behind the cut are exact zeros; two runs give the same bits.
2. Binding: autograd through raymarching.normal_image equals the raw calls bit for bit, rows outside spans and ids of no
   ray are 0.
3. image_smooth forward and backward EQUAL the float32 restatement (no transcendental: ==) at (B,H,W,C) = (1,1,1,3),
   (1,1,5,3), (1,5,1,3), (2,3,4,3), (1,4,4,1).
4. Renderer (the f32 scene of tests/shading_reference.py: 8 x 8 rays, max_steps 32, textureless): image, depth and
   weights_sum are the normal_image=False render's bits; normal_image against float64 on the render's own sigmas7 AND
   against composite_rays_train of the reference normals under the forward rule; the gradient of
   image_smooth(normal_image).sum() reaches the hash table and the MLP, non-zero and finite.
5. Trainer (16 x 16, 8 steps, synthetic guidance, start_shading_iter = 1; seed 1 draws albedo, 3 x lambertian,
   textureless, albedo, 2 x textureless): lambda = 0 is the default's run bit for bit and call for call; lambda > 0
   differs, calls exactly the four new entry points more, and step_loss carries the term; captured == eager bit for bit;
   views_per_step = 2 runs.
Every test prints the figures it asserts on (run with -s).
Measured on the MI355X, worst ratio error / tolerance per case: forward 0.004 (density_scale 1; the 3-sample ray, 2.9e-8 at
7.8e-6) and 0.006 (0.5; the 1-sample ray), largest error 8.0e-8 (65 samples) at 1.3e-4, the float32 restatement's own
errors 2.3e-8 .. 1.6e-7; backward centre rows 0.008 and 0.008 (the 1-sample ray, 1.4e-9 at 1.8e-7), offset rows 0.002 and
0.005, on the two 1e10 samples 1.4e4 / 1.8e4 of rows of 2.8e10 / 2.9e10 (the restatement's own error there); image_smooth:
0 differing elements at every shape, both ways; renderer (216 samples, longest ray 10, largest |N| 0.985): 1.2e-7 at 2.1e-5
against float64 (ratio 0.006), 1.2e-7 against the compositing of the reference normals (0.007); all 7 parameter tensors
receive a non-zero gradient; trainer: 283 entry-point calls in 8 steps without the term, 295 with it (4 x 3), all 7 parameter
tensors differ, step_loss 9.954e-3 = 9.13e-5 + 9.863e-3."""
import collections

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import normal_image_reference as R
from tests import shading_reference as SR

pytestmark = pytest.mark.gpu


ULP = 2.0 ** -24
S1, S2 = 123.0, -321.0      # poison of the forward / backward outputs
HW, MAX_STEPS, EPS, AMBIENT = (SR.SCENE[k] for k in ("HW", "MAX_STEPS", "EPS", "AMBIENT"))
LIGHT = list(SR.SCENE["LIGHT"])


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


def _tolerances(sig7, deltas, rays, n_ids, ds, dN):
    """The rule of the module docstring on one input -> dict(fwd, centre [n_ids], stencil [m] per span row, cnt [n_ids],
    e = f32_errors())."""
    e = R.f32_errors(sig7, deltas, rays, n_ids, R.INV_2EPS, ds, dN)
    cnt = np.zeros(n_ids)
    cnt[rays[:, 0]] = rays[:, 2]
    rows, _ = R.span_rows(rays)
    dtmax = R.per_ray_max(np.asarray(deltas, dtype=np.float64)[rows, 0], rays, n_ids)
    _, ids = R.span_rows(rays)
    e_s = np.abs(e["r32"]["grad"].astype(np.float64) - e["t64"]["grad"])[:, 1:].max(-1) if len(ids) else np.zeros(0)
    go = np.linalg.norm(np.asarray(dN, dtype=np.float64), axis=-1)
    tol = COMPOSITE_TOL(cnt)
    return dict(fwd=4 * e["fwd"] + tol * 1.0, centre=4 * e["centre"] + tol * go * dtmax * float(np.float32(ds)),
                stencil=4 * e_s + (tol * go)[ids] * R.INV_2EPS * e["t64"]["r"], cnt=cnt, e=e)


def _ratio(err, tol):
    return np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))


# ------------------------------------------------------------------------------ 1, 2: the ray kernels
class _Op:
    """The op-level case on the device, the two entry points on it, and the reference figures (computed once)."""

    def __init__(self, dev):
        self.k = k = R.op_case()
        self.truth = R.check_case(k)                       # the preconditions, before anything is compared
        self.dev = dev
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.sig7, self.deltas, self.rays, self.dN = t(k["sig7"]), t(k["deltas"]), t(k["rays"]), t(k["dN"])
        self.tol = {ds: _tolerances(k["sig7"], k["deltas"], k["rays"], k["n_ids"], ds, k["dN"]) for ds in R.DENSITY_SCALES}
        _, self.ids = R.span_rows(k["rays"])

    def forward(self, ds):
        from src.latent_nerf.raymarching import backend as B
        from src.latent_nerf.raymarching.raymarching import _p, _stream
        k = self.k
        image = torch.full((k["n_ids"], 3), S1, device=self.dev)
        B.call("lnerf_normal_image_forward", _p(self.sig7), _p(self.deltas), _p(self.rays), k["N"], R.INV_2EPS, ds,
               R.T_THRESH, _p(image), _stream())
        torch.cuda.synchronize()
        return image

    def backward(self, ds, image):
        from src.latent_nerf.raymarching import backend as B
        from src.latent_nerf.raymarching.raymarching import _p, _stream
        k = self.k
        out = torch.full((7 * k["cap"],), S2, device=self.dev)
        B.call("lnerf_normal_image_backward", _p(self.sig7), _p(self.deltas), _p(self.rays), k["N"], R.INV_2EPS, ds,
               R.T_THRESH, _p(self.dN), _p(image), _p(out), _stream())
        torch.cuda.synchronize()
        return out


@pytest.fixture(scope="module")
def op(dev):
    return _Op(dev)


@pytest.mark.parametrize("ds", R.DENSITY_SCALES)
def test_op_forward(op, ds):
    k, tol, t64 = op.k, op.tol[ds], op.truth[ds]
    image = op.forward(ds)
    got = image.cpu().double().numpy()
    present = np.zeros(k["n_ids"], bool)
    present[k["ids"]] = True
    assert int((~present).sum()) == 1 and (got[~present] == S1).all()          # the id of no ray: not touched
    err = np.where(present, np.abs(got - t64["image"]).max(-1), 0.0)
    ratio = _ratio(err, tol["fwd"])
    for rid in k["ids"]:
        print("density_scale %.1f ray id %d (%3d samples): N = (%+.4f %+.4f %+.4f), error %.3e, f32 restatement %.3e, "
              "tolerance %.3e" % (ds, rid, tol["cnt"][rid], *got[rid], err[rid], tol["e"]["fwd"][rid], tol["fwd"][rid]))
    print("forward, density_scale %.1f: worst ratio error / tolerance %.3f (ray id %d)"
          % (ds, float(ratio.max()), int(ratio.argmax())))
    assert (err <= tol["fwd"]).all(), float((err - tol["fwd"]).max())
    empty = int(k["ids"][R.R_EMPTY])
    assert tol["cnt"][empty] == 0 and not got[empty].any()                       # the empty ray: written, zeros
    assert np.isfinite(got).all() and float(np.abs(t64["image"]).max()) > 0.05
    assert _same_bits(op.forward(ds), image)


@pytest.mark.parametrize("ds", R.DENSITY_SCALES)
def test_op_backward(op, ds):
    k, tol, t64, M = op.k, op.tol[ds], op.truth[ds], op.k["M"]
    image = op.forward(ds)
    out = op.backward(ds, image)
    assert bool((out[7 * M:] == S2).all())                 # rows outside every span keep the poison
    got = out[:7 * M].cpu().double().numpy().reshape(M, 7)   # (the spans are rows 0 .. M - 1 in ray order)
    assert np.isfinite(got).all()
    err = np.abs(got - t64["grad"])                        # every row of every sample, the NaN and degenerate ones included
    worst_c = R.per_ray_max(err[:, 0], k["rays"], k["n_ids"])
    worst_s = R.per_ray_max(err[:, 1:], k["rays"], k["n_ids"])
    ratio_s = _ratio(err[:, 1:].max(-1), tol["stencil"])       # per sample, against the sample's own tolerance
    tol_s = R.per_ray_max(tol["stencil"], k["rays"], k["n_ids"])
    big_c = R.per_ray_max(t64["grad"][:, 0], k["rays"], k["n_ids"])
    big_s = R.per_ray_max(t64["grad"][:, 1:], k["rays"], k["n_ids"])
    for rid in k["ids"]:
        print("density_scale %.1f ray id %d (%3d samples): centre rows max %.3e, error %.3e (f32 restatement %.3e, tolerance "
              "%.3e); offset rows max %.3e, error %.3e (f32 restatement %.3e, largest tolerance %.3e)"
              % (ds, rid, tol["cnt"][rid], big_c[rid], worst_c[rid], tol["e"]["centre"][rid], tol["centre"][rid],
                 big_s[rid], worst_s[rid], tol["e"]["stencil"][rid], tol_s[rid]))
    rc, rs = _ratio(worst_c, tol["centre"]), R.per_ray_max(ratio_s, k["rays"], k["n_ids"])
    print("backward, density_scale %.1f: worst ratio error / tolerance, centre rows %.3f (ray id %d), offset rows %.3f (ray "
          "id %d)" % (ds, float(rc.max()), int(rc.argmax()), float(rs.max()), int(rs.argmax())))
    assert (err[:, 0] <= tol["centre"][op.ids]).all(), float((err[:, 0] - tol["centre"][op.ids]).max())
    assert (err[:, 1:] <= tol["stencil"][:, None]).all(), float(ratio_s.max())
    # behind the cut: exact zeros in all seven rows
    dead = ~t64["live"]
    assert int(dead.sum()) >= 10 and not got[dead].any() and not t64["grad"][dead].any()
    # the degenerate and the NaN sample: rows of the stated size (r = 1e10), finite
    at = np.concatenate([[0], np.cumsum(k["rays"][:, 2])])
    for ray, i in ((R.R_DEGENERATE, R.I_DEGENERATE), (R.R_NAN, R.I_NAN)):
        assert float(np.abs(got[at[ray] + i, 1:]).min()) > 1e6
    assert float(np.abs(t64["grad"][:, 0]).max()) > 1e-3
    assert _same_bits(op.backward(ds, image), out)


def test_binding(op):
    from src.latent_nerf.raymarching import raymarching as rm
    k, M, ds = op.k, op.k["M"], 0.5
    image_k = op.forward(ds)
    want = op.backward(ds, image_k)
    sig7 = op.sig7.clone().requires_grad_()
    image = rm.normal_image(sig7, op.deltas, op.rays, k["n_ids"], R.EPS, ds, R.T_THRESH)
    assert image.shape == (k["n_ids"], 3) and image.requires_grad
    present = torch.zeros(k["n_ids"], dtype=torch.bool)
    present[torch.from_numpy(k["ids"])] = True
    present = present.to(op.dev)
    assert _same_bits(image[present], image_k[present]) and not bool(image[~present].any())   # ids of no ray: exactly 0
    grad, = torch.autograd.grad(image, sig7, op.dN)
    assert _same_bits(grad[:7 * M], want[:7 * M]) and not bool(grad[7 * M:].any())            # outside the spans: 0
    # n_ids defaults to the number of rays (ids 0 .. N - 1 here, so that they fit); no upstream gradient: no launch
    rays2 = op.rays.clone()
    rays2[:, 0] = torch.arange(k["N"], dtype=torch.int32, device=op.dev)
    sig2 = op.sig7.clone().requires_grad_()
    image2 = rm.normal_image(sig2, op.deltas, rays2, None, R.EPS, ds, R.T_THRESH)
    assert image2.shape == (k["N"], 3) and _same_bits(image2, image_k[torch.from_numpy(k["ids"]).to(op.dev)])
    finite = torch.nan_to_num(sig2)
    g2, = torch.autograd.grad((finite * 2.0).sum() + 0.0 * image2.detach().sum(), sig2)
    assert int((g2 == 2.0).sum()) == g2.numel() - 1


# ------------------------------------------------------------------------------ 3. the stencil
@pytest.mark.parametrize("shape", R.SMOOTH_SHAPES)
def test_image_smooth_equals_the_float32_restatement(dev, shape):
    from src.latent_nerf.raymarching import raymarching as rm
    img_np, dl_np = R.smooth_case(shape)
    img = torch.from_numpy(img_np).to(dev).requires_grad_()
    loss = rm.image_smooth(img)
    assert loss.shape == tuple(shape[:3]) + (2,) and loss.requires_grad
    d_img, = torch.autograd.grad(loss, img, torch.from_numpy(dl_np).to(dev))
    want_f, want_b = R.smooth_forward(img_np, np.float32), R.smooth_backward(img_np, dl_np, np.float32)
    got_f, got_b = loss.detach().cpu().numpy(), d_img.cpu().numpy()
    print("image_smooth %s: forward max %.4e, backward max %.4e, differing elements %d + %d"
          % (shape, float(np.abs(want_f).max()), float(np.abs(want_b).max()), int((got_f != want_f).sum()),
             int((got_b != want_b).sum())))
    assert got_f.dtype == np.float32 and np.array_equal(got_f, want_f)
    assert got_b.shape == tuple(shape) and np.array_equal(got_b, want_b)
    assert not got_f[:, :, -1, 0].any() and not got_f[:, -1, :, 1].any()          # no pair past the last column / row
    again = rm.image_smooth(img.detach())
    assert _same_bits(again, loss)


# ------------------------------------------------------------------------------ 4. renderer
@pytest.fixture(scope="module")
def scene(dev):
    net, _ = SR.scene_net(O, "f32")
    net = net.to(dev).train()
    ro, rd, bg, g = SR.scene_rays(O)
    return dict(net=net, ro=ro[None].to(dev), rd=rd[None].to(dev), bg=bg.to(dev))


def _render(c, **kw):
    return c["net"].render(c["ro"], c["rd"], bg_color=c["bg"], perturb=False, max_steps=MAX_STEPS, shading="textureless",
                           light_d=LIGHT, ambient_ratio=AMBIENT, normal_eps=EPS, **kw)


def test_render_with_normal_image(dev, scene):
    from src.latent_nerf.raymarching import raymarching as rm
    c, N = scene, HW * HW
    net = c["net"]
    plain = _render(c)
    assert "normal_image" not in plain
    out = _render(c, normal_image=True)
    assert out["normal_image"].shape == (1, N, 3) and out["normal_image"].requires_grad
    for key in ("image", "depth", "weights_sum"):
        assert torch.equal(out[key], plain[key]) and _same_bits(out[key], plain[key]), key
    # the render's own sigmas7, computed again (the field's forward repeats its bits): the node on them gives the image
    cap = out["xyzs"].shape[0]
    with torch.no_grad():
        pts7, m7 = rm.fd_points(out["xyzs"], net.bound, EPS, cap, out["counter"][0:1])
        sigmas7, _ = net.field(pts7, 7 * cap, m7, 7 * cap)
        again = rm.normal_image(sigmas7, out["deltas"], out["rays"], N, EPS, net.density_scale, 1e-4)
    assert _same_bits(again, out["normal_image"][0])
    rays = out["rays"].cpu().numpy()
    M = int(out["counter"][0])
    assert rays.shape == (N, 3) and int(rays[:, 2].sum()) == M > 100
    sig7, deltas = sigmas7.cpu().numpy(), out["deltas"].cpu().numpy()
    dN = np.zeros((N, 3), np.float32)
    tol = _tolerances(sig7, deltas, rays, N, float(net.density_scale), dN)
    t64 = tol["e"]["t64"]
    margin = float((np.abs(t64["T"] - R.T_THRESH) / R.T_THRESH).min())
    assert margin >= 1e-3, margin                          # the GPU and the reference agree on which samples are live
    got = out["normal_image"][0].detach().cpu().double().numpy()
    err = np.abs(got - t64["image"]).max(-1)
    ratio = _ratio(err, tol["fwd"])
    print("normal_image against float64: %d samples, longest ray %d, largest |N| %.4f, worst ray error %.3e at a tolerance "
          "of %.3e (ratio %.3f)" % (M, int(rays[:, 2].max()), float(np.linalg.norm(got, axis=-1).max()), float(err.max()),
                                    float(tol["fwd"][err.argmax()]), float(ratio.max())))
    assert (err <= tol["fwd"]).all(), float((err - tol["fwd"]).max())
    assert (tol["cnt"] == 0).any() and not got[tol["cnt"] == 0].any() and float(np.abs(t64["image"]).max()) > 0.05
    # the training compositing of the reference normals (float64 normals of the same sigmas7, handed over as colours)
    rows, _ = R.span_rows(rays)
    n_ref = np.zeros((cap, 3), np.float32)
    n_ref[rows] = t64["n"].astype(np.float32)
    with torch.no_grad():
        _, _, comp = rm.composite_rays_train(out["sigmas"].detach(), torch.from_numpy(n_ref).to(dev), out["deltas"],
                                             out["rays"], 1e-4, None)
    err_c = np.abs(got - comp.cpu().double().numpy()).max(-1)
    ratio_c = _ratio(err_c, tol["fwd"])
    print("normal_image against composite_rays_train of the reference normals: worst ray difference %.3e (ratio %.3f)"
          % (float(err_c.max()), float(ratio_c.max())))
    assert (err_c <= tol["fwd"]).all(), float((err_c - tol["fwd"]).max())


def test_smoothness_gradient_reaches_the_table_and_the_mlp(dev, scene):
    from src.latent_nerf.raymarching import raymarching as rm
    c = scene
    for p in c["net"].parameters():
        p.grad = None
    out = _render(c, normal_image=True)
    pairs = rm.image_smooth(out["normal_image"].view(1, HW, HW, 3))
    assert pairs.shape == (1, HW, HW, 2) and float(pairs.detach().sum()) > 0
    pairs.sum().backward()
    grads = {name: p.grad for name, p in c["net"].named_parameters() if p.grad is not None}
    for name in sorted(grads):
        print("d%-20s: max |grad| %.3e" % (name, float(grads[name].abs().max())))
    assert "encoder.embeddings" in grads and len(grads) >= 3
    sigma_side = [name for name in grads if float(grads[name].abs().max()) > 0]
    assert "encoder.embeddings" in sigma_side and len(sigma_side) >= 3           # the table and the density MLP's layers
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    for p in c["net"].parameters():
        p.grad = None


# ------------------------------------------------------------------------------ 5. trainer
TRAINER_SEED, TRAINER_STEPS, TRAINER_START, TRAIN_HW = 1, 8, 1, 16
LAMBDA = 0.5
NEW = {"lnerf_normal_image_forward", "lnerf_normal_image_backward", "lnerf_image_smooth_forward",
       "lnerf_image_smooth_backward"}


def _trainer_cfg(root, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(root), "render.train_h": TRAIN_HW, "render.train_w": TRAIN_HW,
            "render.eval_h": TRAIN_HW, "render.eval_w": TRAIN_HW, "render.grid_size": 32, "optim.iters": TRAINER_STEPS,
            "optim.lr": 5e-3, "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1,
            "optim.seed": TRAINER_SEED, "guide.text": "a lego man", "log.quiet": True,
            "optim.start_shading_iter": TRAINER_START}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """name, overrides -> (trainer, parameters, exp_avg, exp_avg_sq, calls) of one 8-step run, each configuration trained
    once; calls = how often every entry point of the library was called during the run."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.training.trainer import Trainer
    root, runs = tmp_path_factory.mktemp("normal_smooth"), {}

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


def _n_shaded():
    from src.latent_nerf.training import shading as SH
    return sum(k != "albedo" for k in SH.schedule(TRAINER_SEED, 1, TRAINER_STEPS, TRAINER_START))


def test_trainer_captured_equals_eager_with_the_term(dev, trained):
    n_shaded = _n_shaded()
    assert n_shaded >= 5
    runs = {}
    for graph in (True, False):
        runs[graph] = trained("n%d" % graph, **{"optim.graph_step": graph, "optim.lambda_normal_smooth": LAMBDA})
        tr = runs[graph][0]
        assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == n_shaded, tr.graph_stats
        assert all(bool(torch.isfinite(p).all()) for p in runs[graph][1])
        key = (1, TRAIN_HW, TRAIN_HW, 2)
        assert list(tr._normal_smooth_const) == [key]                            # one constant, allocated before the captures
        g = tr._normal_smooth_const[key]
        n_pairs = TRAIN_HW * (TRAIN_HW - 1) * 3
        assert bool((g == float(np.float32(LAMBDA / n_pairs))).all())           # (H = W: both channels hold the same value)
    tr = runs[True][0]
    assert tr.graph_stats["captures"] >= 1 and tr._gstep_shaded is not None, tr.graph_stats   # the shaded form is replayed
    assert tr.graph_stats["replayed_steps"] >= 3
    assert runs[False][0].graph_stats["captures"] == 0
    _assert_same_run(runs[True], runs[False])


def test_trainer_the_term_acts_and_zero_is_the_default_path(dev, trained):
    on = trained("n1", **{"optim.graph_step": True, "optim.lambda_normal_smooth": LAMBDA})
    zero = trained("zero", **{"optim.graph_step": True, "optim.lambda_normal_smooth": 0.0})
    default = trained("default", **{"optim.graph_step": True})
    assert default[0].cfg.optim.lambda_normal_smooth == 0.0
    assert not default[0]._normal_smooth_const and not zero[0]._normal_smooth_const
    assert zero[0].graph_stats["shaded_steps"] == on[0].graph_stats["shaded_steps"] == _n_shaded()
    _assert_same_run(zero, default)
    # lambda = 0 issues the default's launches, call for call; with the term exactly the four entry points more
    assert zero[4] == default[4] and sum(zero[4].values()) > 50, (zero[4], default[4])
    print("entry-point calls of the %d-step run: %d without the term, %d with it; the term's: %s"
          % (TRAINER_STEPS, sum(zero[4].values()), sum(on[4].values()), {k: on[4][k] for k in sorted(NEW)}))
    assert not NEW & set(zero[4]) and set(on[4]) == set(zero[4]) | NEW
    assert {k: v for k, v in on[4].items() if k not in NEW} == dict(zero[4])
    assert on[4]["lnerf_normal_image_forward"] == on[4]["lnerf_image_smooth_forward"] == on[4]["lnerf_shade_fd_forward"] > 0
    assert on[4]["lnerf_normal_image_backward"] == on[4]["lnerf_image_smooth_backward"] == on[4]["lnerf_shade_fd_backward"] > 0
    differ = [i for i, (x, y) in enumerate(zip(on[1], zero[1])) if not torch.equal(x, y)]
    print("parameters that differ between lambda_normal_smooth = %g and 0: %s of %d" % (LAMBDA, differ, len(on[1])))
    assert differ
    # the logged value of the auxiliary terms carries the term on a shaded render, and only there
    from src.latent_nerf.training.guidance import sparsity_loss
    tr = on[0]
    tr.nerf.train()
    with torch.cuda.stream(tr.stream):
        tr._shaded = True
        out, _ = tr._render_train(tr._camera())
        with_term = float(tr.step_loss(out))
        tr._shaded = False
        out0, _ = tr._render_train(tr._camera())
        assert out["normal_image"].shape == (1, TRAIN_HW * TRAIN_HW, 3) and "normal_image" not in out0
        img = out["normal_image"].detach().double().view(1, TRAIN_HW, TRAIN_HW, 3)
        n_pairs = TRAIN_HW * (TRAIN_HW - 1) * 3
        want = LAMBDA * (float(((img[:, :, 1:] - img[:, :, :-1]) ** 2).sum()) / n_pairs
                         + float(((img[:, 1:] - img[:, :-1]) ** 2).sum()) / n_pairs)
        base = float(tr.cfg.optim.lambda_sparsity * sparsity_loss(out["weights_sum"].detach()))
    torch.cuda.synchronize()
    print("step_loss %.6e = sparsity %.6e + the normal-smoothness term %.6e" % (with_term, base, want))
    assert want > 0 and abs(with_term - (base + want)) <= 1e-5 * max(abs(with_term), 1e-6)


def test_trainer_two_views_per_step(dev, trained):
    run = trained("views2", **{"optim.graph_step": True, "optim.lambda_normal_smooth": LAMBDA, "optim.views_per_step": 2})
    tr = run[0]
    assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == _n_shaded(), tr.graph_stats
    assert list(tr._normal_smooth_const) == [(2, TRAIN_HW, TRAIN_HW, 2)]
    n_pairs = 2 * TRAIN_HW * (TRAIN_HW - 1) * 3
    assert bool((tr._normal_smooth_const[(2, TRAIN_HW, TRAIN_HW, 2)] == float(np.float32(LAMBDA / n_pairs))).all())
    assert all(bool(torch.isfinite(p).all()) for p in run[1])
    assert run[4]["lnerf_normal_image_forward"] > 0 and run[4]["lnerf_image_smooth_backward"] > 0
    one = trained("n1", **{"optim.graph_step": True, "optim.lambda_normal_smooth": LAMBDA})
    assert [i for i, (x, y) in enumerate(zip(run[1], one[1])) if not torch.equal(x, y)]
