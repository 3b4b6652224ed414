"""The orientation regulariser on the MI355X (csrc/shade.hip k_shade_fwd / k_shade_bwd with ORIENT = true,
raymarching.shade_fd(orient=...), render(orient=True), optim.lambda_orient).  References: tests/orient_reference.py
(float64; its op-level case and the preconditions asserted on it before anything is compared: sigma' dt <= 1.5, every
reference T at least 1e-3 (relative) away from T_thresh, every lit / away-facing normal more than 0.1 rad from l / v).

1. Forward: sigma_c and colours are lnerf_shade_fd_forward's bits; per ray with k samples |orient - ref| <= 2 COMPOSITE_TOL(k)
   (the compositing bound 32 2^-24 (k + 1) in its (1 + max |c|) form with q^2 <= 1); the empty ray and the back-facing ray
   give exactly 0; sentinel rows untouched.
2. Backward with d_orient = None: lnerf_shade_fd_backward's bits.
3. Backward, orientation alone and combined.  Yardstick r0: the EXISTING lnerf_shade_fd_backward against the float64
   reference of itself on these inputs, max over samples of max_j |x - ref| / max_j |ref|.  Then per sample of the fused
   backward  max_j |got - ref| <= 4 r0 (max_j |ref_lam| + max_j |ref_or|) + COMPOSITE_TOL(k) |go| max_j |U|
   (4: the factor of tests/test_gpu_shading.py, for the second addend and the extra dot product; second term: the
   weight's error carried through).  Reference zeros (w = 0, q = 0, g = 0) are exact zeros in the orientation-alone case;
   two runs give the same bits.
4. Renderer (the f32 scene of tests/shading_reference.py): loss_orient is shade_fd(orient=...) fed the chain's own pieces,
   image / depth / weights_sum are the orient=False render's bits, parameter gradients of image . G + lambda
   mean(loss_orient) against float64 autograd of the oracle chain (render_shaded_oracle + orient_reference.orient_torch)
   with the rule of test_f32_training_render_matches_the_oracle: per tensor max |grad - ref| <= 4 x (the albedo render's
   worst figure) x max |ref|; prepared= and the camera form give the ray form's bits.
5. Trainer (the configuration of test_trainer_schedule_captured_equals_eager, lambda_orient = 1e-2, 12 steps): captured ==
   eager bit for bit, shaded steps happen, the term acts, and lambda_orient = 0 is the default's path bit for bit.
Every test prints the figures it asserts on (run with -s).
Measured on the MI355X: forward, worst ray 4.0e-8 at a tolerance of 2.5e-4; r0 = 4.8e-7 (C = 4), 4.2e-7 (C = 3); backward,
orientation alone 6.9e-11 at 1.3e-7 (ratio 0.001), combined 4.1e-7 at 1.6e-6 (ratio 0.25); renderer gradients, worst
tensor 1.05e-4 (lambertian) and 1.45e-4 (textureless) against the albedo render's 9.44e-5, r = 3.78e-4; loss_orient mean
1.0189e-2 against 1.0189e-2, worst ray 2.4e-6."""
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import orient_reference as Q
from tests import shading_reference as R

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
W_NAMES = R.W_NAMES
G, HW, LOG2_T, MAX_STEPS, EPS, AMBIENT = (R.SCENE[k] for k in ("G", "HW", "LOG2_T", "MAX_STEPS", "EPS", "AMBIENT"))
LIGHT = list(R.SCENE["LIGHT"])
S1, S2 = 123.0, -321.0      # sentinels of the forward / backward outputs


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


# ------------------------------------------------------------------------------ 1 - 3: the kernels
class _Op:
    """The op-level case on the device and the four entry points on it."""

    def __init__(self, dev, C, density_scale):
        self.k = k = Q.op_case(C, density_scale)
        self.terms, self.w, self.T = Q.check_case(k)        # the preconditions, before anything is compared
        self.dev, self.C, self.ds = dev, C, float(density_scale)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        self.sig, self.alb, self.rays, self.shade = t(k["sig"].reshape(-1)), t(k["alb"].reshape(-1, C)), t(k["rays"]), t(k["shade"])
        self.deltas, self.rays_d = t(k["deltas"]), t(k["rays_d"])
        self.t = t
        self.head = (k["sig"].reshape(-1), k["alb"].reshape(-1, C), k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"])
        self.tail = (k["deltas"], k["rays_d"], self.ds, Q.T_THRESH)
        self.counts = k["rays"][:, 2][np.searchsorted(np.cumsum(k["rays"][:, 2]), np.arange(k["M"]), side="right")]

    def _call(self, name, *args):
        from src.latent_nerf.raymarching import backend as B
        from src.latent_nerf.raymarching.raymarching import _p, _stream
        k = self.k
        B.call(name, _p(self.sig), _p(self.alb), self.C, _p(self.rays), k["N"], Q.RAYS_PER_VIEW, _p(self.shade), Q.N_VIEWS,
               k["inv"], *[_p(a) if torch.is_tensor(a) else a for a in args], _stream())

    def forward(self, orient):
        cap = self.k["cap"]
        sc, co = torch.full((cap,), S1, device=self.dev), torch.full((cap, self.C), S1, device=self.dev)
        if not orient:
            self._call("lnerf_shade_fd_forward", sc, co)
            return sc, co, None
        out = torch.full((self.k["N"],), S1, device=self.dev)
        self._call("lnerf_shade_fd_orient_forward", self.deltas, self.rays_d, self.ds, Q.T_THRESH, sc, co, out)
        return sc, co, out

    def backward(self, dsig, dcol, d_orient="plain"):
        cap = self.k["cap"]
        d7, dr7 = torch.full((7 * cap,), S2, device=self.dev), torch.full((7 * cap, self.C), S2, device=self.dev)
        dsig, dcol = self.t(dsig), self.t(dcol)
        if isinstance(d_orient, str):
            self._call("lnerf_shade_fd_backward", dsig, dcol, d7, dr7)
        else:
            self._call("lnerf_shade_fd_orient_backward", dsig, dcol, self.deltas, self.rays_d, self.ds, Q.T_THRESH,
                       None if d_orient is None else self.t(d_orient), d7, dr7)
        torch.cuda.synchronize()
        return d7, dr7

    def rows7(self, d7):
        return d7.view(self.k["cap"], 7)[: self.k["M"]].cpu().double().numpy()      # (the spans are rows 0 .. M - 1 in ray order)


CASES = [(4, 1.0), (3, 0.5), (4, 0.5), (3, 1.0)]
CASES_EVERY_C = CASES + [(2, 1.0), (1, 0.5)]      # the entry points dispatch on C = 1..4


@pytest.mark.parametrize("C,density_scale", CASES_EVERY_C)
def test_forward(dev, C, density_scale):
    op = _Op(dev, C, density_scale)
    k, M = op.k, op.k["M"]
    assert np.array_equal(op.terms["rows"], np.arange(M)) and all(i != r for r, i in enumerate(Q.IDS))
    sc0, co0, _ = op.forward(False)
    sc, co, got = op.forward(True)
    torch.cuda.synchronize()
    assert torch.equal(sc, sc0) and torch.equal(co, co0) and _same_bits(sc, sc0) and _same_bits(co, co0)
    assert bool((sc[M:] == S1).all()) and bool((co[M:] == S1).all())          # sentinel rows
    ref = Q.orient_forward(op.head[0], k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"], *op.tail, k["N"])
    got = got.cpu().double().numpy()
    cnt_of_id = np.zeros(k["N"])
    cnt_of_id[k["rays"][:, 0]] = k["rays"][:, 2]
    tol = 2 * COMPOSITE_TOL(cnt_of_id)
    err = np.abs(got - ref)
    for rid in range(k["N"]):
        print("C=%d scale=%g ray id %d (%3d samples): orient %.6f, ref %.6f, error %.3e, tolerance %.3e"
              % (C, density_scale, rid, cnt_of_id[rid], got[rid], ref[rid], err[rid], tol[rid]))
    assert (err <= tol).all(), float((err - tol).max())
    assert got[Q.IDS[0]] == 0.0 and cnt_of_id[Q.IDS[0]] == 0                 # the empty ray: written, 0
    assert got[Q.IDS[Q.R_BACK]] == 0.0 and ref[Q.IDS[Q.R_BACK]] == 0.0       # the back-facing ray
    assert float(ref.max()) > 0.05
    again = op.forward(True)
    torch.cuda.synchronize()
    assert _same_bits(again[2], torch.from_numpy(got).float())


@pytest.mark.parametrize("C,density_scale", CASES_EVERY_C)
def test_backward_without_a_gradient_for_the_term_is_the_plain_backward(dev, C, density_scale):
    op = _Op(dev, C, density_scale)
    k, M = op.k, op.k["M"]
    d7a, dr7a = op.backward(k["dsig"], k["dcol"])
    d7b, dr7b = op.backward(k["dsig"], k["dcol"], None)
    assert torch.equal(d7a, d7b) and torch.equal(dr7a, dr7b) and _same_bits(d7a, d7b) and _same_bits(dr7a, dr7b)
    assert bool((d7b[7 * M:] == S2).all()) and bool((dr7b[7 * M:] == S2).all())


@pytest.mark.parametrize("C,density_scale", CASES)
def test_backward_orientation_alone_and_combined(dev, C, density_scale):
    op = _Op(dev, C, density_scale)
    k, M, cap = op.k, op.k["M"], op.k["cap"]
    zs, zc = np.zeros(cap, np.float32), np.zeros((cap, C), np.float32)
    # the yardstick: the EXISTING backward against the float64 reference of itself (not the code under test)
    ref0 = Q.orient_backward(*op.head, k["dsig"], k["dcol"], *op.tail, None)
    d7_plain, dr7_plain = op.backward(k["dsig"], k["dcol"])
    e0 = np.abs(op.rows7(d7_plain) - ref0["lam"]).max(-1) / np.abs(ref0["lam"]).max(-1)
    r0 = float(e0.max())
    print("C=%d scale=%g: r0 = %.3e (lnerf_shade_fd_backward against its float64 reference, worst sample %d)"
          % (C, density_scale, r0, int(e0.argmax())))
    assert 0 < r0 < 1e-3
    for name, dsig, dcol in (("orientation alone", zs, zc), ("combined", k["dsig"], k["dcol"])):
        ref = Q.orient_backward(*op.head, dsig, dcol, *op.tail, k["d_orient"])
        d7, dr7 = op.backward(dsig, dcol, k["d_orient"])
        got = op.rows7(d7)
        want = ref["lam"] + ref["orient"]
        err = np.abs(got - want).max(-1)
        tol = (4 * r0 * (np.abs(ref["lam"]).max(-1) + np.abs(ref["orient"]).max(-1))
               + COMPOSITE_TOL(op.counts) * np.abs(ref["go"]) * np.abs(ref["U"]).max(-1))
        live = tol > 0
        worst = int(np.argmax(np.where(live, err / np.where(live, tol, 1.0), 0.0)))
        print("C=%d scale=%g %s: worst sample %d: error %.3e at a tolerance of %.3e (ratio %.3f; weight share %.3e); "
              "max |ref_or| %.3e, max |ref_lam| %.3e"
              % (C, density_scale, name, worst, err[worst], tol[worst], err[worst] / max(tol[worst], 1e-300),
                 float((COMPOSITE_TOL(op.counts) * np.abs(ref["go"]) * np.abs(ref["U"]).max(-1))[worst]),
                 float(np.abs(ref["orient"]).max()), float(np.abs(ref["lam"][:, 1:]).max())))
        assert (err <= tol).all(), (name, float((err - tol).max()))
        assert float(np.abs(ref["orient"]).max()) > 1e-3
        # the rows the term does not reach: the albedo gradient, the sentinels
        plain_rgb = dr7_plain if name == "combined" else op.backward(dsig, dcol)[1]
        assert torch.equal(dr7, plain_rgb) and bool((d7[7 * M:] == S2).all()) and bool((dr7[7 * M:] == S2).all())
        if name == "orientation alone":
            zero = ~ref["orient"].any(-1)
            # (all three kinds of zero are in the case: killed weights, back-facing normals, the flat sample)
            assert (ref["w"] == 0).any() and ((ref["w"] > 0) & (op.terms["q"] == 0)).any()
            assert zero[np.cumsum(k["rays"][:, 2])[Q.R_KILL - 1] + Q.I_FLAT]
            assert int(zero.sum()) > 100 and (got[zero] == 0).all()
            assert bool((dr7[:7 * M] == 0).all())
        d7b, dr7b = op.backward(dsig, dcol, k["d_orient"])
        assert _same_bits(d7, d7b) and _same_bits(dr7, dr7b)


def test_shade_fd_binding(dev):
    """The autograd node hands the kernels' results through: one node, three outputs, d_orient None -> NULL."""
    from src.latent_nerf.raymarching import raymarching as rm
    op = _Op(dev, 4, 0.5)
    k, M, cap = op.k, op.k["M"], op.k["cap"]
    s7, a7 = op.sig.clone().requires_grad_(), op.alb.clone().requires_grad_()
    orient = (op.deltas, op.rays_d, op.ds, Q.T_THRESH, k["N"])
    sc, co, ori = rm.shade_fd(s7, a7, op.rays, op.shade, Q.RAYS_PER_VIEW, Q.EPS, orient=orient)
    assert sc.grad_fn is co.grad_fn is ori.grad_fn and ori.shape == (k["N"],)
    sc_k, co_k, ori_k = op.forward(True)
    assert _same_bits(sc[:M], sc_k[:M]) and _same_bits(co[:M], co_k[:M]) and _same_bits(ori, ori_k)
    dsig, dcol = k["dsig"].copy(), k["dcol"].copy()
    dsig[M:], dcol[M:] = 0.0, 0.0
    torch.autograd.backward([sc, co, ori], [op.t(dsig), op.t(dcol), op.t(k["d_orient"])])
    d7, dr7 = op.backward(dsig, dcol, k["d_orient"])
    assert _same_bits(s7.grad[:7 * M], d7[:7 * M]) and _same_bits(a7.grad[:7 * M], dr7[:7 * M])
    # without a gradient for the term: the plain node's gradients
    s7b, a7b = op.sig.clone().requires_grad_(), op.alb.clone().requires_grad_()
    sc, co, ori = rm.shade_fd(s7b, a7b, op.rays, op.shade, Q.RAYS_PER_VIEW, Q.EPS, orient=orient)
    torch.autograd.backward([sc, co], [op.t(dsig), op.t(dcol)])
    d7p, dr7p = op.backward(dsig, dcol)
    assert _same_bits(s7b.grad[:7 * M], d7p[:7 * M]) and _same_bits(a7b.grad[:7 * M], dr7p[:7 * M])
    with pytest.raises(ValueError, match="rays_d"):
        rm.shade_fd(s7, a7, op.rays, op.shade, Q.RAYS_PER_VIEW, Q.EPS,
                    orient=(op.deltas, op.rays_d[:4], op.ds, Q.T_THRESH, k["N"]))
    with pytest.raises(ValueError, match="deltas"):
        rm.shade_fd(s7, a7, op.rays, op.shade, Q.RAYS_PER_VIEW, Q.EPS,
                    orient=(op.deltas[:cap - 1], op.rays_d, op.ds, Q.T_THRESH, k["N"]))


# ------------------------------------------------------------------------------ 4. renderer
LAMBDA_RENDER = 4.0       # weight of mean(loss_orient) beside image . G in the gradient comparison


def _grads(net):
    out = {"table": net.encoder.embeddings.grad.detach().clone()}
    out.update({k: getattr(net, k).grad.detach().clone() for k in W_NAMES})
    for p in net.parameters():
        p.grad = None
    return out


@pytest.fixture(scope="module")
def scene(dev):
    """The f32 net of the shading tests, the oracle's leaves and the ALBEDO yardstick of the gradient bound, once."""
    net, bits = R.scene_net(O, "f32")
    net = net.to(dev).train()
    ro, rd, bg, g = R.scene_rays(O)
    lv, table, params = R.scene_oracle_leaves(O, net)

    def leaves():
        tab = table.double().requires_grad_()
        par = {k: v.double().requires_grad_() for k, v in params.items()}
        return tab, par

    def collect(tab, par):
        grads = {"table": tab.grad}
        grads.update({k: par[k].grad for k in W_NAMES})
        return grads

    def figures(got, ref):
        return {k: float((got[k].cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}

    out = net.render(ro[None].to(dev), rd[None].to(dev), bg_color=bg.to(dev), perturb=False, max_steps=MAX_STEPS)
    out["image"].backward(g.to(dev))
    tab, par = leaves()
    ref = R.render_shaded_oracle(O, ro, rd, tab, par, lv, bits, light=LIGHT, ambient=AMBIENT, textureless=False, eps=EPS, G=G,
                                 max_steps=MAX_STEPS, bg_color=bg, shaded=False)
    ref["image"].backward(g[0])
    assert int(out["counter"][0]) == ref["M"]
    yard = figures(_grads(net), collect(tab, par))
    return dict(net=net, bits=bits, ro=ro, rd=rd, bg=bg, g=g, lv=lv, leaves=leaves, collect=collect, figures=figures,
                yard=yard)


def _oracle_orient(c, tab, par, textureless):
    """float64: mean over the rays of the term on the oracle's march, weights detached (the oracle chain's second part)."""
    N = HW * HW
    aabb = [-1.0] * 3 + [1.0] * 3
    with torch.no_grad():
        nears, fars = O.near_far_from_aabb(c["ro"], c["rd"], aabb, 0.1)
        xyzs, dirs, deltas, rays, M = O.march_rays_train(c["ro"], c["rd"], nears, fars, c["bits"], 1.0, 1, G, MAX_STEPS, 0.0,
                                                         None)
    rows, ids = R._span_rows(rays.numpy())
    assert np.array_equal(np.sort(rows), np.arange(M))
    pts7 = R._pts7_torch(xyzs, 1.0, EPS).double()
    sig7, _ = R._field64(O, pts7, tab, par, c["lv"], 1.0, 5.0, 0.2)
    sg = sig7.reshape(M, 7)[torch.from_numpy(rows)]
    v = torch.from_numpy(Q.view_dirs(c["rd"].numpy()))[ids]
    w = Q.weights_torch(sg[:, 0], deltas[:, 0].double()[torch.from_numpy(rows)], rays, 1.0, 1e-4)
    ori = Q.orient_torch(sg, v, w, torch.from_numpy(ids), N, 1.0 / (2.0 * EPS))
    return ori, M


@pytest.mark.parametrize("shading", ["lambertian", "textureless"])
def test_render_with_orient(dev, scene, shading):
    from src.latent_nerf.raymarching import raymarching as rm
    c = scene
    net, N = c["net"], HW * HW
    net.train()
    ro, rd, bg, g = c["ro"][None].to(dev), c["rd"][None].to(dev), c["bg"].to(dev), c["g"].to(dev)
    kw = dict(shading=shading, light_d=LIGHT, ambient_ratio=AMBIENT, normal_eps=EPS, bg_color=bg, perturb=False,
              max_steps=MAX_STEPS)

    def total(out):
        return [out["image"], out["loss_orient"]], [g, torch.full((1, N), LAMBDA_RENDER / N, device=dev)]

    plain = net.render(ro, rd, **kw)
    assert "loss_orient" not in plain
    out = net.render(ro, rd, orient=True, **kw)
    assert out["loss_orient"].shape == out["weights_sum"].shape == (1, N) and out["loss_orient"].requires_grad
    for key in ("image", "depth", "weights_sum"):
        assert torch.equal(out[key], plain[key]) and _same_bits(out[key], plain[key]), key
    torch.autograd.backward(*total(out))
    got = _grads(net)
    # the chain of the public pieces
    p = net.prepare_rays(ro, rd, bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    assert p.rays_d.shape == (N, 3)
    shade = rm.shade_record(LIGHT, AMBIENT, shading == "textureless", 1, dev)
    pts7, m7 = rm.fd_points(p.march.xyzs, net.bound, EPS, p.cap, p.march.counter[0:1])
    s7, c7 = net.field(pts7, 7 * p.cap, m7, 7 * p.cap)
    sc, col, ori = rm.shade_fd(s7, c7, p.march.rays, shade, N, EPS,
                               orient=(p.march.deltas, p.rays_d, net.density_scale, 1e-4, N))
    ws, depth, image = rm.composite_rays_train(sc, col, p.march.deltas, p.march.rays, 1e-4, p.bg)
    assert torch.equal(out["loss_orient"][0], ori) and _same_bits(out["loss_orient"][0], ori)
    assert _same_bits(out["image"][0], image)
    torch.autograd.backward([image, ori], [g[0], torch.full((N,), LAMBDA_RENDER / N, device=dev)])
    chain = _grads(net)
    for k in got:
        assert _same_bits(got[k], chain[k]), k
    # prepared= and the camera form
    p = net.prepare_rays(ro, rd, bg_color=bg, perturb=False, max_steps=MAX_STEPS)
    out_p = net.render(None, None, prepared=p, orient=True, **kw)
    assert _same_bits(out_p["loss_orient"], out["loss_orient"]) and _same_bits(out_p["image"], out["image"])
    torch.autograd.backward(*total(out_p))
    got_p = _grads(net)
    for k in got:
        assert _same_bits(got[k], got_p[k]), k
    f = HW / (2 * math.tan(math.radians(55) / 2))
    intr = (f, f, HW / 2, HW / 2)
    pose = O.pose_from_angles(math.radians(60), 0.3, 1.25).to(dev)
    ro2, rd2 = rm.get_rays(pose, intr, HW, HW)
    a = net.render(ro2, rd2, orient=True, **kw)
    torch.autograd.backward(*total(a))
    ga = _grads(net)
    b = net.render(None, None, camera=(pose, intr, HW, HW), orient=True, **kw)
    torch.autograd.backward(*total(b))
    gb = _grads(net)
    assert _same_bits(a["loss_orient"], b["loss_orient"]) and _same_bits(a["image"], b["image"])
    assert float(a["loss_orient"].detach().max()) > 0
    for k in ga:
        assert _same_bits(ga[k], gb[k]), k
    # against the oracle chain in float64
    tab, par = c["leaves"]()
    ref = R.render_shaded_oracle(O, c["ro"], c["rd"], tab, par, c["lv"], c["bits"], light=LIGHT, ambient=AMBIENT,
                                 textureless=shading == "textureless", eps=EPS, G=G, max_steps=MAX_STEPS, bg_color=c["bg"])
    ref_ori, M = _oracle_orient(c, tab, par, shading == "textureless")
    assert int(out["counter"][0]) == ref["M"] == M
    ((ref["image"] * c["g"][0]).sum() + LAMBDA_RENDER * ref_ori.mean()).backward()
    ref_grads = c["collect"](tab, par)
    k_of = torch.zeros(N, dtype=torch.float64)
    k_of[ref["rays"][:, 0].long()] = ref["rays"][:, 2].double()
    e = (out["loss_orient"][0].detach().cpu().double() - ref_ori.detach()).abs()
    # forward, per ray: the compositing bound (q^2 <= 1) plus the 2e-3 rad normal bound of tests/test_gpu_normals.py
    # carried through q^2 (|d q^2| <= 2 q |dn| <= 4e-3 per unit weight, weights summing to <= 1)
    tol = 2 * COMPOSITE_TOL(k_of) + 4e-3
    print("%s loss_orient: mean %.4e (ref %.4e), worst ray error %.3e at a tolerance of %.3e"
          % (shading, float(out["loss_orient"].detach().mean()), float(ref_ori.detach().mean()), float(e.max()), float(tol[e.argmax()])))
    assert bool((e <= tol).all()) and float(ref_ori.detach().mean()) > 1e-4
    fig = c["figures"](got, ref_grads)
    yard = max(c["yard"].values())
    r = 4 * yard
    for name in fig:
        print("%s d%-5s: max|grad - ref| / max|ref| = %.3e   (albedo render, same tensor: %.3e)"
              % (shading, name, fig[name], c["yard"][name]))
    print("%s: figure with the term %.3e, albedo figure %.3e, r = 4 x albedo = %.3e" % (shading, max(fig.values()), yard, r))
    for name in fig:
        assert fig[name] <= r, (name, fig[name], r)


# ------------------------------------------------------------------------------ 5. trainer
TRAINER_SEED, TRAINER_STEPS, TRAINER_START = 1, 12, 3      # (the schedule of tests/test_gpu_shading.py, two steps shorter)


def _trainer_cfg(root, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(root), "render.train_h": 32, "render.train_w": 32,
            "render.eval_h": 32, "render.eval_w": 32, "render.grid_size": 64, "optim.iters": TRAINER_STEPS,
            "optim.lr": 5e-3, "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1,
            "optim.seed": TRAINER_SEED, "guide.text": "a lego man", "log.quiet": True,
            "optim.start_shading_iter": TRAINER_START}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


@pytest.fixture(scope="module")
def trained(dev, tmp_path_factory):
    """name, overrides -> (trainer, parameters, exp_avg, exp_avg_sq) of one 12-step run, each configuration trained once."""
    from src.latent_nerf.training.trainer import Trainer
    root, runs = tmp_path_factory.mktemp("orient"), {}

    def run(name, **over):
        if name not in runs:
            torch.manual_seed(7)
            torch.cuda.manual_seed(7)
            tr = Trainer(_trainer_cfg(root, **{"log.exp_name": name, **over}), device=dev)
            tr.train()
            torch.cuda.synchronize()
            st = tr.optimizer.state_dict()
            params = [p.detach().clone() for grp in tr.nerf.get_params(1.0) for p in grp["params"]]
            runs[name] = (tr, params, [t.clone() for t in st["exp_avg"]], [t.clone() for t in st["exp_avg_sq"]])
        return runs[name]

    return run


def _assert_same_run(a, b):
    for what, x, y in zip(("parameters", "exp_avg", "exp_avg_sq"), a[1:], b[1:]):
        assert len(x) == len(y)
        for i, (s, t) in enumerate(zip(x, y)):
            assert _same_bits(s, t), (what, i)


@pytest.mark.parametrize("fp16", [True, False])
def test_trainer_captured_equals_eager_with_the_term(dev, trained, fp16):
    from src.latent_nerf.training import shading as SH
    want = SH.schedule(TRAINER_SEED, 1, TRAINER_STEPS, TRAINER_START)
    n_shaded = sum(k != "albedo" for k in want)
    assert n_shaded >= 4 and "albedo" in want[2:]
    runs = {}
    for graph in (True, False):
        runs[graph] = trained("o%d%d" % (graph, fp16), **{"optim.fp16": fp16, "optim.graph_step": graph,
                                                         "optim.lambda_orient": 1e-2})
        tr = runs[graph][0]
        assert tr.train_step == TRAINER_STEPS and tr.graph_stats["shaded_steps"] == n_shaded > 0, tr.graph_stats
        assert all(bool(torch.isfinite(p).all()) for p in runs[graph][1])
        assert list(tr._orient_const) == [(1, 32 * 32)]                       # one constant, allocated before the captures
        assert float(tr._orient_const[(1, 1024)][0, 0]) == np.float32(1e-2 / 1024)
    tr = runs[True][0]
    assert tr.graph_stats["captures"] == 2 and tr._gstep_shaded is not None, tr.graph_stats
    assert tr.graph_stats["eager_steps"] == 4 and tr.graph_stats["replayed_steps"] == TRAINER_STEPS - 4
    assert runs[False][0].graph_stats["captures"] == 0
    _assert_same_run(runs[True], runs[False])


def test_trainer_the_term_acts_and_zero_is_the_default_path(dev, trained):
    on = trained("o11", **{"optim.fp16": True, "optim.graph_step": True, "optim.lambda_orient": 1e-2})
    zero = trained("zero", **{"optim.fp16": True, "optim.graph_step": True, "optim.lambda_orient": 0.0})
    default = trained("default", **{"optim.fp16": True, "optim.graph_step": True})
    assert default[0].cfg.optim.lambda_orient == 0.0 and not default[0]._orient_const and not zero[0]._orient_const
    assert zero[0].graph_stats["shaded_steps"] == on[0].graph_stats["shaded_steps"] > 0
    _assert_same_run(zero, default)
    differ = [i for i, (x, y) in enumerate(zip(on[1], zero[1])) if not torch.equal(x, y)]
    print("parameters that differ between lambda_orient = 1e-2 and 0: %s of %d" % (differ, len(on[1])))
    assert differ
    # the logged value of the auxiliary terms carries the term on a shaded render
    tr = on[0]
    tr.nerf.train()
    with torch.cuda.stream(tr.stream):
        tr._shaded = True
        out, _ = tr._render_train(tr._camera())
        with_term = float(tr.step_loss(out))
        tr._shaded = False
        out0, _ = tr._render_train(tr._camera())
        assert "loss_orient" in out and "loss_orient" not in out0
        want = float(tr.cfg.optim.lambda_orient * out["loss_orient"].detach().mean())
        from src.latent_nerf.training.guidance import sparsity_loss
        base = float(tr.cfg.optim.lambda_sparsity * sparsity_loss(out["weights_sum"].detach()))
    torch.cuda.synchronize()
    assert want >= 0 and abs(with_term - (base + want)) <= 1e-6 * max(abs(with_term), 1e-6)
