"""Shaded renders on the MI355X (shading = 'lambertian' / 'textureless'; csrc/shade.hip, NeRFRenderer.run_cuda, the trainer's
optim.start_shading_iter).

1. lnerf_fd_points and 2. lnerf_shade_fd_forward / _backward against the numpy restatement (tests/shading_reference.py),
   bit for bit, untouched rows checked with sentinels.
3. render(shading=...) in training mode is the chain of its public pieces, bit for bit (f32 / hash and bf16 / blocked).
4. The f32 render against the oracle composition (f64 field and shade, the oracle's f32 march and compositing).
   Image, per ray with k samples:  COMPOSITE_TOL(k) (1 + max_k |c_k|) + 2e-3 (1 - ambient) max_k |albedo_k|  -- the
   compositing bound of tests/test_gpu_latent_tune.py plus the 2e-3 rad normal bound of tests/test_gpu_normals.py carried
   through lam.  Parameter gradients, per tensor:  max |grad - ref| <= r max |ref| with ONE r = 4 x the figure of the
   ALBEDO render of the same case against the same oracle, that render's figure being its worst tensor's
   max |grad - ref| / max |ref| (existing code: the yardstick is not the code under test; the factor covers the
   seven-fold addend count and the run-to-run spread of the float sums).  Both figures are printed, and every tensor's.
   Measured on the MI355X (this case, 216 samples): image error / tolerance 0.002 (lambertian), 0.013 (textureless);
   gradient figure 1.05e-4 (lambertian) and 1.43e-4 (textureless) against the albedo render's 9.44e-5, r = 3.78e-4.
   A FINDING, per tensor: the three bias tensors miss 4 x their OWN albedo figure -- lambertian db1 3.8e-6, db2 9.4e-6,
   db3 1.1e-6 and textureless 1.2e-5, 2.2e-5, 2.7e-5 against the albedo render's 2.3e-7, 1.4e-7, 1.1e-7 (the albedo
   bias gradients are plain sums and land at f32 epsilon; table and weights sit at 1e-5 .. 1e-4 either way).  It is the
   finite difference in f32, not the kernels: g = (sigma+ - sigma-) / (2 eps) multiplies the f32 rounding of sigma by
   sigma / |sigma+ - sigma-| (tens to hundreds at eps 1e-2), and the oracle composition itself evaluated in f32 on the
   CPU (torch ops, no kernel of this library) gives the same figures against its f64 form: lambertian 4.0e-6, 9.1e-6,
   1.1e-6; textureless 1.2e-5, 2.0e-5, 6.9e-5.
5. The evaluation loop against the oracle's inference loop with the bound of 4; albedo / normal renders around it keep
   their bits.
6. The trainer: captured == eager bit for bit over a schedule with all three kinds, at most two captures, and
   start_shading_iter = None is the plain path.
Every test prints the figures it asserts on (run with -s)."""

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import shading_reference as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
W_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
G, HW, LOG2_T, MAX_STEPS, EPS, AMBIENT = (R.SCENE[k] for k in ("G", "HW", "LOG2_T", "MAX_STEPS", "EPS", "AMBIENT"))
LIGHT = list(R.SCENE["LIGHT"])


def COMPOSITE_TOL(k):          # (tests/test_gpu_latent_tune.py)
    return 32 * ULP * (k + 1)


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


# ------------------------------------------------------------------------------ 1. points
def test_fd_points_bit_equal_and_rows_past_the_count_untouched(dev):
    from src.latent_nerf.raymarching import raymarching as rm
    cap, m, bound = 300, 257, 1.0
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, (cap, 3)).astype(np.float32)
    x[0] = (1.0, -1.0, 1.0)                                       # exact +-bound
    x[1] = (-1.0, 1.0, -1.0)
    x[2] = (1.0 - 0.004, -1.0 + 0.004, 0.0)                       # within eps of the faces
    x[3] = (np.nextafter(np.float32(1.0 - EPS), np.float32(2)), -0.995, 0.995)
    x[256] = (0.999, 0.999, -0.999)                               # the last counted sample
    xd = torch.from_numpy(x).to(dev)
    m_dev = torch.tensor([m], dtype=torch.int32, device=dev)
    sentinel = -777.0
    pts7 = torch.full((7 * cap, 3), sentinel, device=dev)
    m7 = torch.full((1,), -5, dtype=torch.int32, device=dev)
    got, got_m7 = rm.fd_points(xd, bound, EPS, cap, m_dev, out=(pts7, m7))
    assert got.data_ptr() == pts7.data_ptr() and got_m7.data_ptr() == m7.data_ptr()
    ref = R.fd_points(x, bound, EPS, m)
    assert int(m7.item()) == 1799 == 7 * m
    assert _same_bits(pts7[:7 * m], ref)
    assert bool((pts7[7 * m:] == sentinel).all())
    moved = pts7[:7 * m].view(m, 7, 3).cpu()
    assert float(moved[:, 1:].abs().max()) <= 1.0                 # every offset point stays in the box
    # the host bound alone (no device counter), more than one block, and a fresh allocation
    got2, m7b = rm.fd_points(xd, bound, EPS, 290)
    assert int(m7b.item()) == 7 * 290 and _same_bits(got2[:7 * 290], R.fd_points(x, bound, EPS, 290))
    # m_host = 0: nothing is launched, nothing is touched
    pts7.fill_(sentinel)
    m7.fill_(-5)
    rm.fd_points(xd, bound, EPS, 0, m_dev, out=(pts7, m7))
    assert bool((pts7 == sentinel).all()) and int(m7.item()) == -5
    # a device counter of zero under a positive host bound: the counter is written, no row is
    rm.fd_points(xd, bound, EPS, cap, torch.zeros(1, dtype=torch.int32, device=dev), out=(pts7, m7))
    assert bool((pts7 == sentinel).all()) and int(m7.item()) == 0
    with pytest.raises(ValueError, match="GPU"):
        rm.fd_points(torch.from_numpy(x), bound, EPS, cap)


# ------------------------------------------------------------------------------ 2. shade forward / backward
COUNTS = (0, 1, 63, 64, 65, 130)


def _shade_case(C, seed=2):
    rng = np.random.default_rng(seed)
    offs = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
    rays = np.stack([np.array([4, 0, 5, 2, 1, 3]), offs, np.array(COUNTS)], -1).astype(np.int32)   # ids 0..5, shuffled
    M = int(sum(COUNTS))
    cap = M + 17
    sig = rng.uniform(0.0, 4.0, (cap, 7)).astype(np.float32)
    sig[5] = 2.25                                                  # an all-equal septuple: s = 0
    sig[70, 1:] = 0.5                                              # s = 0 with another centre
    alb = rng.normal(size=(cap, 7, C)).astype(np.float32)
    l0 = np.array([0.6, 0.0, 0.8])
    l1 = np.array([-0.48, 0.6, -0.64])
    shade = np.array([[*l0, 0.1, 0.0], [*l1, 0.1, 1.0]], dtype=np.float32)       # view 0 lambertian, view 1 textureless
    dsig = rng.normal(size=cap).astype(np.float32)
    dcol = rng.normal(size=(cap, C)).astype(np.float32)
    return rays, M, cap, sig, alb, shade, dsig, dcol


@pytest.mark.parametrize("C", [4, 3, 2, 1])
def test_shade_forward_and_backward_bit_equal_to_numpy(dev, C):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    rays, M, cap, sig, alb, shade, dsig, dcol = _shade_case(C)
    inv = 1.0 / (2.0 * EPS)
    rpv, nviews = 3, 2
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d_sig, d_alb, d_rays, d_shade, d_dsig, d_dcol = (t(sig.reshape(-1)), t(alb.reshape(-1, C)), t(rays), t(shade), t(dsig),
                                                     t(dcol))
    S1, S2 = 123.0, -321.0

    def run():
        sc, co = torch.full((cap,), S1, device=dev), torch.full((cap, C), S1, device=dev)
        B.call("lnerf_shade_fd_forward", _p(d_sig), _p(d_alb), C, _p(d_rays), rays.shape[0], rpv, _p(d_shade), nviews, inv,
               _p(sc), _p(co), _stream())
        d7, dr7 = torch.full((7 * cap,), S2, device=dev), torch.full((7 * cap, C), S2, device=dev)
        B.call("lnerf_shade_fd_backward", _p(d_sig), _p(d_alb), C, _p(d_rays), rays.shape[0], rpv, _p(d_shade), nviews, inv,
               _p(d_dsig), _p(d_dcol), _p(d7), _p(dr7), _stream())
        torch.cuda.synchronize()
        return sc, co, d7, dr7

    sc, co, d7, dr7 = run()
    r_sc, r_co = np.full(cap, S1, np.float32), np.full((cap, C), S1, np.float32)
    R.shade_forward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, rpv, inv, r_sc, r_co)
    r_d7, r_dr7 = np.full(7 * cap, S2, np.float32), np.full((7 * cap, C), S2, np.float32)
    R.shade_backward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, rpv, inv, dsig, dcol, r_d7, r_dr7)
    # the case reaches every branch: s = 0, d < 0 and d > 0 under both kinds
    rows, ids = R._span_rows(rays)
    rec = shade[np.minimum(ids // rpv, 1)]
    n, s, r, d, lam = R._lambert(sig[rows], rec[:, :3], rec[:, 3], inv)
    for kind in (0.0, 1.0):
        sel = rec[:, 4] == kind
        assert (d[sel] < 0).any() and (d[sel] > 0).any()
    assert int((s == 0).sum()) == 2
    # (sentinels included: rows past the last span, and sample rows of no ray, keep theirs)
    assert _same_bits(sc, r_sc) and _same_bits(co, r_co)
    assert _same_bits(d7, r_d7) and _same_bits(dr7, r_dr7)
    assert bool((sc[M:] == S1).all()) and bool((co[M:] == S1).all())
    assert bool((d7[7 * M:] == S2).all()) and bool((dr7[7 * M:] == S2).all())
    assert bool((dr7[:7 * M].view(M, 7, C)[:, 1:] == 0).all())
    again = run()
    for a, b in zip((sc, co, d7, dr7), again):
        assert _same_bits(a, b)


def test_shade_fd_binding_and_autograd(dev):
    """The autograd node hands the kernels' results through unchanged, and rejects CPU tensors."""
    from src.latent_nerf.raymarching import raymarching as rm
    C = 4
    rays, M, cap, sig, alb, shade, dsig, dcol = _shade_case(C)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    s7, a7 = t(sig.reshape(-1)).requires_grad_(), t(alb.reshape(-1, C)).requires_grad_()
    sc, co = rm.shade_fd(s7, a7, t(rays), t(shade), 3, EPS)
    dsig[M:], dcol[M:] = 0.0, 0.0
    torch.autograd.backward([sc, co], [t(dsig), t(dcol)])
    inv = 1.0 / (2.0 * EPS)
    r_sc, r_co = np.zeros(cap, np.float32), np.zeros((cap, C), np.float32)
    R.shade_forward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, 3, inv, r_sc, r_co)
    r_d7, r_dr7 = np.zeros(7 * cap, np.float32), np.zeros((7 * cap, C), np.float32)
    R.shade_backward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, 3, inv, dsig, dcol, r_d7, r_dr7)
    assert _same_bits(sc[:M], r_sc[:M]) and _same_bits(co[:M], r_co[:M])
    assert _same_bits(s7.grad[:7 * M], r_d7[:7 * M]) and _same_bits(a7.grad[:7 * M], r_dr7[:7 * M])
    with pytest.raises(ValueError, match="GPU"):
        rm.shade_fd(torch.from_numpy(sig.reshape(-1)), torch.from_numpy(alb.reshape(-1, C)), t(rays), t(shade), 3, EPS)
    rec = rm.shade_record([0.0, 3.0, 4.0], 0.25, True, 2, dev)
    assert rec.shape == (2, 5) and torch.equal(rec.cpu(), torch.tensor([[0.0, 0.6, 0.8, 0.25, 1.0]] * 2))
    assert rm.shade_record(rec, 0.9, False, 2, dev) is rec or torch.equal(rm.shade_record(rec, 0.9, False, 2, dev), rec)


# ------------------------------------------------------------------------------ the tiny scene of 3, 4, 5
def _scene_net(dev, precision):
    net, bits = R.scene_net(O, precision)          # (built on the CPU, as tests/test_shading_cpu.py builds it)
    return net.to(dev), bits


def _scene_rays():
    return R.scene_rays(O)


def _grads(net):
    out = {"table": net.encoder.embeddings.grad.detach().clone()}
    out.update({k: getattr(net, k).grad.detach().clone() for k in W_NAMES})
    for p in net.parameters():
        p.grad = None
    return out


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_training_render_equals_the_chain_of_its_pieces(dev, precision):
    from src.latent_nerf.raymarching import raymarching as rm
    net, _ = _scene_net(dev, precision)
    net.train()
    ro, rd, bg, g = _scene_rays()
    ro, rd, bg, g = ro[None].to(dev), rd[None].to(dev), bg.to(dev), g.to(dev)
    N = HW * HW
    out = net.render(ro, rd, shading="lambertian", light_d=LIGHT, ambient_ratio=AMBIENT, normal_eps=EPS, bg_color=bg,
                     perturb=False, max_steps=MAX_STEPS)
    assert out["image"].shape == (1, N, 4) and out["sigmas"].shape == (out["xyzs"].shape[0],)
    M = int(out["counter"][0])
    assert M > 100 and out["xyzs"].shape[0] >= M
    out["image"].backward(g)
    g_render = _grads(net)
    p = net.prepare_rays(ro, rd, bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    shade = rm.shade_record(LIGHT, AMBIENT, False, 1, dev)
    pts7, m7 = rm.fd_points(p.march.xyzs, net.bound, EPS, p.cap, p.march.counter[0:1])
    assert int(m7.item()) == 7 * M
    s7, c7 = net.field(pts7, 7 * p.cap, m7, 7 * p.cap)
    sc, col = rm.shade_fd(s7, c7, p.march.rays, shade, N, EPS)
    ws, depth, image = rm.composite_rays_train(sc, col, p.march.deltas, p.march.rays, 1e-4, p.bg)
    image.backward(g[0])
    g_chain = _grads(net)
    assert _same_bits(out["image"][0], image) and _same_bits(out["depth"][0], depth)
    assert _same_bits(out["weights_sum"][0], ws)
    assert _same_bits(out["sigmas"][:M], sc[:M])
    for k in g_render:
        assert float(g_render[k].abs().max()) > 0, k
        assert _same_bits(g_render[k], g_chain[k]), k
    # the record form the trainer passes gives the same frame; textureless differs from lambertian
    out2 = net.render(ro, rd, shading="textureless", light_d=shade, bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    assert _same_bits(out2["image"], out["image"])                 # (the record's flag rules: lambertian)
    out3 = net.render(ro, rd, shading="textureless", light_d=LIGHT, bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    assert not torch.equal(out3["image"], out["image"]) and _same_bits(out3["weights_sum"], out["weights_sum"])


# ------------------------------------------------------------------------------ 4. against the oracle (f32)
@pytest.fixture(scope="module")
def oracle_case(dev):
    """The f32 net, the oracle's leaves and the ALBEDO yardstick of the gradient bound, computed once."""
    net, bits = _scene_net(dev, "f32")
    net.train()
    ro, rd, bg, g = _scene_rays()
    lv, table, params = R.scene_oracle_leaves(O, net)

    def oracle(shaded, textureless=False):
        tab = table.double().requires_grad_()
        par = {k: v.double().requires_grad_() for k, v in params.items()}
        ref = R.render_shaded_oracle(O, ro, rd, tab, par, lv, bits, light=LIGHT, ambient=AMBIENT, textureless=textureless,
                                     eps=EPS, G=G, max_steps=MAX_STEPS, bg_color=bg, shaded=shaded)
        ref["image"].backward(g[0])
        grads = {"table": tab.grad}
        grads.update({k: par[k].grad for k in W_NAMES})
        return ref, grads

    def figures(got, ref):
        return {k: float((got[k].cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}

    out = net.render(ro[None].to(dev), rd[None].to(dev), bg_color=bg.to(dev), perturb=False, max_steps=MAX_STEPS)
    out["image"].backward(g.to(dev))
    ref, ref_grads = oracle(False)
    assert int(out["counter"][0]) == ref["M"]
    yard = figures(_grads(net), ref_grads)
    return dict(net=net, bits=bits, ro=ro, rd=rd, bg=bg, g=g, lv=lv, table=table, params=params, oracle=oracle,
                figures=figures, yard=yard)


def _ray_max(values, rays, N):
    """Per ray id: the largest |value| over the ray's samples (0 for an empty span)."""
    out = torch.zeros(N, dtype=torch.float64)
    for rid, off, cnt in rays.tolist():
        if cnt > 0:
            out[rid] = float(values[off:off + cnt].abs().max())
    return out


@pytest.mark.parametrize("shading", ["lambertian", "textureless"])
def test_f32_training_render_matches_the_oracle(dev, oracle_case, shading):
    c = oracle_case
    net, N = c["net"], HW * HW
    ref, ref_grads = c["oracle"](True, shading == "textureless")
    # (the seed keeps every normal well conditioned: tests/test_shading_cpu.py checks the same on the CPU)
    flat = int((ref["s"] < 1e-12).sum())
    assert flat <= ref["M"] // 1000, flat
    net.train()
    out = net.render(c["ro"][None].to(dev), c["rd"][None].to(dev), shading=shading, light_d=LIGHT, ambient_ratio=AMBIENT,
                     normal_eps=EPS, bg_color=c["bg"].to(dev), perturb=False, max_steps=MAX_STEPS)
    out["image"].backward(c["g"].to(dev))
    got = _grads(net)
    assert int(out["counter"][0]) == ref["M"]
    k = torch.zeros(N, dtype=torch.float64)
    k[ref["rays"][:, 0].long()] = ref["rays"][:, 2].double()
    cmax = _ray_max(ref["colours"], ref["rays"], N)
    amax = _ray_max(ref["albedo"], ref["rays"], N)
    tol = COMPOSITE_TOL(k) * (1.0 + cmax) + 2e-3 * (1.0 - AMBIENT) * amax
    err = (out["image"][0].cpu().double() - ref["image"].detach().double()).abs().amax(-1)
    worst = int((err / tol).argmax())
    print("%s image: worst error %.3e at a tolerance of %.3e (ratio %.3f; compositing share %.3e)"
          % (shading, float(err[worst]), float(tol[worst]), float((err / tol).max()),
             float(COMPOSITE_TOL(k[worst]) * (1.0 + cmax[worst]))))
    assert bool((err <= tol).all()), float((err - tol).max())
    for key in ("depth", "weights_sum"):
        e = (out[key][0].cpu().double() - ref[key].detach().double()).abs()
        t = COMPOSITE_TOL(k) * max(float(ref[key].abs().max()), 1e-30)
        assert bool((e <= t).all()), (key, float((e - t).max()))
    fig = c["figures"](got, ref_grads)
    yard = max(c["yard"].values())          # the albedo render's figure: its worst tensor
    r = 4 * yard
    for name in fig:
        print("%s d%-5s: max|grad - ref| / max|ref| = %.3e   (albedo render, same tensor: %.3e)"
              % (shading, name, fig[name], c["yard"][name]))
    print("%s: shaded figure %.3e, albedo figure %.3e, r = 4 x albedo = %.3e" % (shading, max(fig.values()), yard, r))
    for name in fig:
        assert fig[name] <= r, (name, fig[name], r)


# ------------------------------------------------------------------------------ 5. evaluation
def test_evaluation_render_matches_the_oracle_loop_and_leaks_no_state(dev, oracle_case):
    c = oracle_case
    net, N = c["net"], HW * HW
    net.eval()
    ro, rd, bg = c["ro"][None].to(dev), c["rd"][None].to(dev), c["bg"].to(dev)
    with torch.no_grad():
        alb0 = net.render(ro, rd, bg_color=bg, max_steps=MAX_STEPS)
        nrm0 = net.render(ro, rd, bg_color=bg, max_steps=MAX_STEPS, shading="normal")
        out = net.render(ro, rd, bg_color=bg, max_steps=MAX_STEPS, shading="textureless", light_d=LIGHT,
                         ambient_ratio=AMBIENT, normal_eps=EPS)
        alb1 = net.render(ro, rd, bg_color=bg, max_steps=MAX_STEPS)
        nrm1 = net.render(ro, rd, bg_color=bg, max_steps=MAX_STEPS, shading="normal")
    for a, b in ((alb0, alb1), (nrm0, nrm1)):
        for key in ("image", "depth", "weights_sum"):
            assert _same_bits(a[key], b[key]), key
    assert _same_bits(out["depth"], alb0["depth"]) and _same_bits(out["weights_sum"], alb0["weights_sum"])
    ref = R.render_shaded_oracle_infer(O, c["ro"], c["rd"], c["table"].double(), {k: v.double() for k, v in c["params"].items()},
                                       c["lv"], c["bits"], light=LIGHT, ambient=AMBIENT, textureless=True, eps=EPS, G=G,
                                       max_steps=MAX_STEPS, bg_color=c["bg"].double())
    k = ref["counts"].double()
    assert int((k > 0).sum()) > N // 8
    # textureless: |c| = lam <= 1; the albedo factor of the normal term is the largest the field gives on these samples
    tol = COMPOSITE_TOL(k) * (1.0 + 1.0) + 2e-3 * (1.0 - AMBIENT) * ref["albedo_max"]
    err = (out["image"][0].cpu().double() - ref["image"]).abs().amax(-1)
    print("evaluation textureless: worst error %.3e, tolerance there %.3e (ratio %.3f)"
          % (float(err.max()), float(tol[err.argmax()]), float((err / tol).max())))
    assert bool((err <= tol).all()), float((err - tol).max())
    net.train()


# ------------------------------------------------------------------------------ 6. trainer
TRAINER_SEED, TRAINER_STEPS, TRAINER_START = 1, 14, 3      # (tests/test_shading_cpu.py checks these draws on the CPU)


def _trainer_cfg(tmp_path, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32,
            "render.eval_h": 32, "render.eval_w": 32, "render.grid_size": 64, "optim.iters": TRAINER_STEPS,
            "optim.lr": 5e-3, "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1,
            "optim.seed": TRAINER_SEED, "guide.text": "a lego man", "log.quiet": True}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


def _train(dev, tmp_path, name, **over):
    from src.latent_nerf.training.trainer import Trainer
    torch.manual_seed(7)
    torch.cuda.manual_seed(7)
    tr = Trainer(_trainer_cfg(tmp_path, **{"log.exp_name": name, **over}), device=dev)
    tr.train()
    torch.cuda.synchronize()
    st = tr.optimizer.state_dict()
    params = [p.detach().clone() for grp in tr.nerf.get_params(1.0) for p in grp["params"]]
    return tr, params, [t.clone() for t in st["exp_avg"]], [t.clone() for t in st["exp_avg_sq"]]


@pytest.mark.parametrize("fp16", [True, False])
def test_trainer_schedule_captured_equals_eager(dev, tmp_path, fp16):
    from src.latent_nerf.training import shading as SH
    want = SH.schedule(TRAINER_SEED, 1, TRAINER_STEPS, TRAINER_START)
    assert set(want[2:]) == set(SH.KINDS)
    n_shaded = sum(k != "albedo" for k in want)
    runs = {}
    for graph in (True, False):
        tr, params, m, v = _train(dev, tmp_path, "g%d%d" % (graph, fp16),
                                  **{"optim.fp16": fp16, "optim.graph_step": graph, "optim.start_shading_iter": TRAINER_START})
        assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == n_shaded, tr.graph_stats
        assert [tr.shading_kind(s) for s in range(1, TRAINER_STEPS + 1)] == want
        assert all(bool(torch.isfinite(p).all()) for p in params)
        if graph:
            assert tr.graph_stats["captures"] == 2, tr.graph_stats           # one plain, one shaded; no recapture
            assert tr.graph_stats["eager_steps"] == 4 and tr.graph_stats["replayed_steps"] == TRAINER_STEPS - 4
            assert tr._gstep is not None and tr._gstep_shaded is not None
            assert tr._static["shade"].shape == (1, 5) and tr._static["cam"].numel() == 26
        else:
            assert tr.graph_stats["captures"] == 0 and tr.graph_stats["eager_steps"] == TRAINER_STEPS
        runs[graph] = (params, m, v)
    for what, a, b in zip(("parameters", "exp_avg", "exp_avg_sq"), runs[True], runs[False]):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert _same_bits(x, y), (what, i)


def test_no_start_step_is_the_plain_path(dev, tmp_path):
    """start_shading_iter = None (captured steps) against the plain path with the schedule switched on but never reached
    (eager steps): the same parameters and moments bit for bit, no shaded step; and a shaded run differs."""
    a = _train(dev, tmp_path, "none", **{"optim.fp16": True})
    b = _train(dev, tmp_path, "never", **{"optim.fp16": True, "optim.graph_step": False,
                                         "optim.start_shading_iter": 10 ** 6})
    assert a[0].graph_stats["shaded_steps"] == 0 == b[0].graph_stats["shaded_steps"]
    assert a[0].graph_stats["captures"] == 1
    for k in (1, 2, 3):
        for x, y in zip(a[k], b[k]):
            assert _same_bits(x, y)
    c = _train(dev, tmp_path, "shaded", **{"optim.fp16": True, "optim.start_shading_iter": TRAINER_START})
    assert not torch.equal(a[1][0], c[1][0])
