"""Field surface normals: the encoder's position gradient (csrc/grid_input.hip, lnerf_grid_encode_backward_input), the
density gradient / normal built on it (NeRFNetwork.density_gradient / normal, lnerf_density_normals), the normal-shaded
evaluation render, the field normals of export_mesh and the trainer's `log.eval_normals`.

The reference is autograd of the oracle in the sample position: O.grid_encode and O.sigma_latent_mlp are differentiable
in x (floor has zero gradient, so the derivative is the one of the cell the sample sits in, one-sided on lattice
planes), in f32 and in the bf16 restatement.

Tolerances
  * encoder gradient: max-abs <= 1e-4 max|ref|, the project's form for summed gradients (f32 summation-order noise
    measured on the CPU against f64 blends: <= 3.6e-7 of the maximum), also for each level alone (one-hot dfeat):
    the coarsest level carries ~1e-3 of the total and would otherwise hide under the fine levels.
  * density gradient, per sample: |g - g_ref|_2 <= 1e-3 |g_ref|_2 (the per-sample gradient rtol applied to the vector),
    normals within 2e-3 rad; at most 0.1 % of the samples may miss either, because a ReLU pre-activation within
    rounding of zero can flip.  (f32 oracle against its f64 restatement on these inputs: 0 of 3001 outside, worst
    relative error 1.2e-5.)
  * bf16: max-abs <= 1e-2 max|ref|, the project's bf16 gradient bound.
  * render: COMPOSITE_TOL(k) of test_gpu_inference.py (32 * 2^-24 (k + 1), the composite's own arithmetic) + 1e-3
    (a 2e-3 rad normal error moves (n + 1) / 2 by at most 1e-3), per ray with its sample count k."""
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

SMALL = dict(num_levels=16, base_resolution=4, desired_resolution=128, log2_hashmap_size=12)
FULL = dict(num_levels=16, base_resolution=16, desired_resolution=2048, log2_hashmap_size=19)
W_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def COMPOSITE_TOL(k):          # (test_gpu_inference.py)
    return 32 * 2.0 ** -24 * (k + 1)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _rand_points(M, bound=1.0, seed=0):      # (test_gpu_parity.py: both box corners and the origin)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(M, 3, generator=g) * 2 - 1) * bound
    x[0] = torch.tensor([-bound, -bound, -bound])
    x[1] = torch.tensor([bound, bound, bound])
    x[2] = torch.tensor([0.0, 0.0, 0.0])
    return x


def _plane_coordinate(scale, k):
    """An f32 coordinate whose level position ((x + 1) / 2) * scale + 0.5 is EXACTLY the integer k (f32 arithmetic of
    the oracle and the kernel)."""
    s = torch.tensor(scale, dtype=torch.float32)
    x = torch.tensor(2.0 * (k - 0.5) / scale - 1.0, dtype=torch.float32)
    cands = [x]
    lo = hi = x
    for _ in range(16):
        lo, hi = torch.nextafter(lo, torch.tensor(-2.0)), torch.nextafter(hi, torch.tensor(2.0))
        cands += [lo, hi]
    for c in cands:
        if float(((c + 1.0) / 2.0) * s + 0.5) == float(k):
            return float(c)
    raise AssertionError("no f32 coordinate lands on lattice plane %d of scale %r" % (k, scale))


def _points(M, scale0, res0):
    """_rand_points plus 8 points exactly on lattice planes of level 0 (one, two and three coordinates on a plane)."""
    x = _rand_points(M)
    ks = [1, max(1, res0 // 2), max(1, res0 - 1)]
    p = [_plane_coordinate(scale0, k) for k in ks]
    r = _rand_points(16, seed=7)[3:11]
    extra = r.clone()
    extra[0, 0], extra[1, 1], extra[2, 2] = p[0], p[0], p[0]
    extra[3, 0], extra[4, 1], extra[5, 2] = p[2], p[2], p[2]
    extra[6, 0], extra[6, 1] = p[0], p[2]
    extra[7] = torch.tensor([p[1], p[0], p[2]])
    pos = ((extra + 1.0) / 2.0) * torch.tensor(scale0, dtype=torch.float32) + 0.5
    assert bool(((pos == torch.floor(pos)).sum(1) >= 1).all()) and int((pos == torch.floor(pos)).sum()) >= 11
    return torch.cat([x, extra])


def _levels(kw, gridtype):
    from src.latent_nerf.models import encoding as E
    lv = O.make_grid_levels(blocked=gridtype == "blocked", tiled=gridtype == "tiled", **kw)
    levels = E.GridLevels(kw["num_levels"], 2, kw["base_resolution"], kw["desired_resolution"], kw["log2_hashmap_size"],
                          gridtype=gridtype)
    assert levels.offsets == lv.offsets and levels.resolutions == lv.resolutions
    return lv, levels


def _dfeat(g, L, stride, dev):
    M = g.shape[0]
    d = torch.zeros(L, stride, 2)
    d[:, :M, :] = g.reshape(M, L, 2).permute(1, 0, 2)
    return d.to(dev)


# ------------------------------------------------------------------------------ 1. encoder input gradient
def _check_input_gradient(dev, kw, M, gridtype, table_dtype, seed):
    from src.latent_nerf.models import encoding as E
    lv, levels = _levels(kw, gridtype)
    L = kw["num_levels"]
    torch.manual_seed(seed)
    table = torch.randn(lv.n_rows, 2) * 0.1
    if table_dtype == "bf16":
        table = table.to(torch.bfloat16).float()          # rounded before both sides see it
    x = _points(M, lv.scales[0], lv.resolutions[0])
    M = x.shape[0]
    g = torch.randn(M, 2 * L)
    xr = x.clone().requires_grad_()
    feat_ref = O.grid_encode((xr + 1.0) / 2.0, table, lv)
    ref = torch.autograd.grad(feat_ref, xr, g, retain_graph=True)[0]
    stride = M + 37
    m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
    xd = torch.zeros(stride, 3)
    xd[:M] = x
    xd = xd.to(dev)
    src = table.to(dev).to(torch.bfloat16) if table_dtype == "bf16" else table.to(dev)
    sentinel = -777.25

    def run(gl):
        out = torch.full((stride, 3), sentinel, device=dev)
        E.grid_encode_backward_input(xd, 1.0, src, levels, _dfeat(gl, L, stride, dev), stride, m_dev, stride, out=out)
        return out

    got = run(g)
    err, scale = float((got[:M].cpu() - ref).abs().max()), float(ref.abs().max())
    print("input gradient %s/%s: max abs err %.3e, max |ref| %.3e (%.2e)" % (gridtype, table_dtype, err, scale, err / scale))
    assert err <= 1e-4 * scale, (err, scale)
    assert bool((got[M:] == sentinel).all()), "rows >= M were touched"
    assert torch.equal(run(g), got), "two calls differ"
    # every level alone
    for l in range(L):
        gl = torch.zeros_like(g)
        gl[:, 2 * l:2 * l + 2] = g[:, 2 * l:2 * l + 2]
        ref_l = torch.autograd.grad(feat_ref, xr, gl, retain_graph=True)[0]
        got_l = run(gl)[:M].cpu()
        err, scale = float((got_l - ref_l).abs().max()), float(ref_l.abs().max())
        assert scale > 0 and err <= 1e-4 * scale, ("level", l, err, scale)
    # m_host == 0: OK, nothing written
    out = torch.full((stride, 3), sentinel, device=dev)
    E.grid_encode_backward_input(xd, 1.0, src, levels, _dfeat(g, L, stride, dev), 0, m_dev, stride, out=out)
    assert bool((out == sentinel).all())


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", ["hash", "blocked", "tiled"])
def test_encoder_input_gradient_matches_oracle_autograd(dev, gridtype, table_dtype):
    _check_input_gradient(dev, SMALL, 3001, gridtype, table_dtype, seed=1)


def test_encoder_input_gradient_full_size(dev):
    _check_input_gradient(dev, FULL, 20000, "hash", "f32", seed=1)


# ------------------------------------------------------------------------------ 2. autograd wiring
@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
def test_grid_encoder_is_differentiable_in_its_input(dev, table_dtype):
    from src.latent_nerf.models import encoding as E
    torch.manual_seed(2)
    enc = E.GridEncoder(table_dtype=torch.bfloat16 if table_dtype == "bf16" else torch.float32, **SMALL).to(dev)
    enc.embeddings.data.normal_(0, 0.1)
    x = _points(3001, enc.levels.scales[0], enc.levels.resolutions[0]).to(dev)
    M = x.shape[0]
    g = torch.randn(M, 32, device=dev)
    xa = x.clone().requires_grad_()
    enc(xa).backward(g)
    gx, gt = xa.grad, enc.embeddings.grad.clone()
    enc.embeddings.grad = None
    enc(x).backward(g)                                   # the input does not require grad: the path of every step
    assert torch.equal(enc.embeddings.grad, gt)
    src = enc.shadow() if table_dtype == "bf16" else enc.embeddings.detach()
    assert (src.dtype == torch.bfloat16) == (table_dtype == "bf16")
    dfeat = g.reshape(M, 16, 2).permute(1, 0, 2).contiguous()
    direct = E.grid_encode_backward_input(x, 1.0, src, enc.levels, dfeat, M, None, M)
    assert gx is not None and torch.equal(gx, direct) and float(gx.abs().max()) > 0


# ------------------------------------------------------------------------------ 3 / 4. density gradient and normals
def _field_net(dev, precision, seed=3, zero_table=False, blob_std=0.2, b3_0=None):
    """NeRFNetwork over the SMALL encoder with the oracle's MLP parameters -> (net, lv, table (cpu, as the gather reads
    it), params (cpu))."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.models.network_grid import NeRFNetwork
    cfg = RenderConfig(grid_size=32, train_h=16, train_w=16, mlp_precision=precision, table_dtype=precision)
    net = NeRFNetwork(cfg, base_resolution=4, log2_hashmap_size=12, blob_std=blob_std)
    net.encoder = E.GridEncoder(table_dtype=torch.bfloat16 if precision == "bf16" else torch.float32,
                                scatter_variant=3 if precision == "bf16" else 2, **SMALL)
    lv = O.make_grid_levels(**SMALL)
    assert net.encoder.levels.offsets == lv.offsets
    torch.manual_seed(seed)
    table = torch.zeros(lv.n_rows, 2) if zero_table else torch.randn(lv.n_rows, 2) * 0.1
    if precision == "bf16":
        table = table.to(torch.bfloat16).float()
    params = O.init_mlp_params(32, 64, 5, seed=0)
    if b3_0 is not None:
        params["b3"][0] = b3_0
    net.encoder.embeddings.data.copy_(table)
    for k in W_NAMES:
        getattr(net, k).data.copy_(params[k])
    return net.to(dev).eval(), lv, table, params


def _reference_gradient(x, lv, table, params, blob_std=0.2, bf16=False):
    xr = x.clone().requires_grad_()
    feat = O.grid_encode((xr + 1.0) / 2.0, table, lv)
    sigma = O.sigma_latent_mlp(feat, xr, params, 5.0, blob_std, bf16=bf16)[0]
    (g,) = torch.autograd.grad(sigma.sum(), xr)
    return sigma.detach(), g


def _safe_normal(g):
    return -g / torch.sqrt(torch.clamp((g * g).sum(-1, keepdim=True), min=1e-20))


def _angles(a, b):
    a, b = a.double(), b.double()
    return torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(-1))


@pytest.mark.parametrize("clamp", [False, True])
def test_density_gradient_and_normals_f32(dev, clamp):
    """clamp: b3[0] = 16 puts every pre-activation above 15, where the trunc-exp backward uses exp(15) (_TruncExp)."""
    net, lv, table, params = _field_net(dev, "f32", b3_0=16.0 if clamp else None)
    x = _points(3001, lv.scales[0], lv.resolutions[0])
    M = x.shape[0]
    sig_ref, g_ref = _reference_gradient(x, lv, table, params)
    if clamp:
        assert float(sig_ref.min()) > math.exp(15.0)
    sig, g = net.density_gradient(x.to(dev))
    n = net.normal(x.to(dev))
    assert sig.shape == (M,) and g.shape == (M, 3) and n.shape == (M, 3)
    assert float(((sig.cpu() - sig_ref).abs() / sig_ref).max()) <= 1e-3
    rel = (g.cpu() - g_ref).norm(dim=-1) / g_ref.norm(dim=-1)
    ang = _angles(n.cpu(), _safe_normal(g_ref))
    allowed = M // 1000            # 0.1 %
    print("density gradient (clamp=%s): worst rel %.3e, %d outside; worst angle %.3e rad, %d outside (of %d)"
          % (clamp, float(rel.max()), int((rel > 1e-3).sum()), float(ang.max()), int((ang > 2e-3).sum()), M))
    assert int((rel > 1e-3).sum()) <= allowed, (float(rel.max()), int((rel > 1e-3).sum()))
    assert int((ang > 2e-3).sum()) <= allowed, (float(ang.max()), int((ang > 2e-3).sum()))
    assert float((n.norm(dim=-1) - 1).abs().max()) < 1e-5
    # density_scale multiplies sigma only
    net.density_scale = 3.0
    sig3, g3 = net.density_gradient(x.to(dev))
    assert torch.equal(sig3, 3.0 * sig) and torch.equal(g3, g) and torch.equal(net.normal(x.to(dev)), n)
    # leading dimensions are flattened, an empty query is an empty answer
    assert torch.equal(net.normal(x.to(dev).view(-1, 17, 3)), n)
    assert net.normal(torch.zeros(0, 3, device=dev)).shape == (0, 3)


def test_zero_table_normals_are_radial(dev):
    """With a zero table the field is the density blob alone: grad sigma = e grad blob, so normal(x) = x / |x| (and the
    zero vector at the origin).  blob_std is 0.5 here: with the default 0.2 the blob's gradient at the box corners is
    ~1e-14, its square below the 1e-20 floor of safe_normalize, and the DEFINED result there is shorter than a unit
    vector; at 0.5 the corner gradient is ~1e-2 and the property holds over the whole box, corners included."""
    net, lv, table, params = _field_net(dev, "f32", zero_table=True, blob_std=0.5)
    x = _points(3001, lv.scales[0], lv.resolutions[0])
    n = net.normal(x.to(dev)).cpu()
    assert bool(torch.isfinite(n).all())
    r = x.norm(dim=-1, keepdim=True)
    nz = r[:, 0] > 0
    assert int((~nz).sum()) == 1 and bool((n[~nz] == 0).all())
    assert float(r[nz].max()) == pytest.approx(math.sqrt(3.0))          # the corners are in
    err = float((n[nz] - x[nz] / r[nz]).abs().max())
    print("zero table: max |n - x/|x|| = %.3e" % err)
    assert err <= 1e-5


def test_density_gradient_bf16(dev):
    net, lv, table, params = _field_net(dev, "bf16", seed=4)
    x = _points(3001, lv.scales[0], lv.resolutions[0])
    sig_ref, g_ref = _reference_gradient(x, lv, table, params, bf16=True)
    sig, g = net.density_gradient(x.to(dev))
    err, scale = float((g.cpu() - g_ref).abs().max()), float(g_ref.abs().max())
    print("bf16 density gradient: max abs err %.3e, max |ref| %.3e (%.2e)" % (err, scale, err / scale))
    assert err <= 1e-2 * scale
    assert bool(torch.isfinite(net.normal(x.to(dev))).all())


# ------------------------------------------------------------------------------ 5. normal-shaded render
def _ray_t_margins(ro, rd, sigma_of, bits, G, max_steps, T_thresh=1e-4, bound=1.0, min_near=0.1):
    """Per ray: the smallest |T / T_thresh - 1| over the float64 transmittance before and after every sample the eval
    loop composites (the per-ray form of test_gpu_inference.py's _t_margin)."""
    N = ro.shape[0]
    nears, fars = O.near_far_from_aabb(ro, rd, [-bound] * 3 + [bound] * 3, min_near)
    alive = torch.arange(N, dtype=torch.int32)
    xyzs, _, deltas = O.march_rays_infer(alive, max_steps, nears.clone(), ro, rd, fars, bits, bound, 1, G, max_steps, 0.0)
    real = deltas[:, 1] >= 0
    sg = torch.zeros(xyzs.shape[0], dtype=torch.float64)
    sg[real] = sigma_of(xyzs[real]).double()
    sg, dl = sg.view(N, max_steps), deltas.view(N, max_steps, 2).double()
    T = torch.ones(N, dtype=torch.float64)
    go = torch.ones(N, dtype=torch.bool)
    margin = torch.full((N,), float("inf"), dtype=torch.float64)
    for s in range(max_steps):
        go = go & (dl[:, s, 1] >= 0)
        margin = torch.where(go, torch.minimum(margin, (T / T_thresh - 1).abs()), margin)
        T = torch.where(go, T * torch.exp(-sg[:, s] * dl[:, s, 0]), T)
        margin = torch.where(go, torch.minimum(margin, (T / T_thresh - 1).abs()), margin)
        go = go & (T >= T_thresh)
    return margin


def test_normal_shaded_render_matches_oracle(dev):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    G, HW, max_steps = 32, 16, 128
    torch.manual_seed(6)
    cfg = RenderConfig(grid_size=G, train_h=HW, train_w=HW, mlp_precision="f32", table_dtype="f32")
    net = NeRFNetwork(cfg, log2_hashmap_size=12)
    net.encoder.embeddings.data.normal_(0, 0.1)
    net = net.to(dev).eval()
    assert net.latent_mode and net.img_dims == 4
    grid = O.density_grid_from_function(lambda p: (p.norm(dim=-1) < 0.5).float() * 10.0, G, 1, 1.0)
    bits = O.packbits(grid.reshape(-1), 0.01)
    net.density_grid.copy_(grid.to(dev))
    net.density_bitfield.copy_(bits.to(dev))
    lv = O.make_grid_levels(16, 2, 16, 2048, 12)
    assert lv.offsets == net.encoder.levels.offsets
    params = {k: getattr(net, k).detach().cpu().clone() for k in W_NAMES}
    table = net.encoder.embeddings.detach().cpu().clone()
    f = HW / (2 * math.tan(math.radians(55) / 2))
    ro, rd = O.get_rays(O.pose_from_angles(math.radians(60), 0.3, 1.25), f, f, HW / 2, HW / 2, HW, HW)
    ro, rd = ro[0].contiguous(), rd[0].contiguous()
    N = HW * HW

    def field(p):
        with torch.enable_grad():
            sigma, g = _reference_gradient(p, lv, table, params)
        return sigma, (_safe_normal(g) + 1.0) / 2.0

    ref = O.render_frame_infer(ro, rd, field, bitfield=bits, bound=1.0, cascade=1, G=G, max_steps=max_steps,
                               schedule=lambda n, a, s: O.renderer_schedule(n, a, s, max_steps))
    assert ref["image"].shape == (N, 3) and int((ref["counts"] > 0).sum()) > N // 8
    assert float(ref["weights_sum"].max()) > 0.5
    margin = _ray_t_margins(ro, rd, lambda p: field(p)[0], bits, G, max_steps)
    keep = margin > 1e-3
    assert int((~keep).sum()) <= N // 100, int((~keep).sum())
    bg = torch.rand(N, 4, generator=torch.Generator().manual_seed(8)).to(dev)
    with torch.no_grad():
        out = net.render(ro[None].to(dev), rd[None].to(dev), shading="normal", bg_color=bg, max_steps=max_steps)
        alb = net.render(ro[None].to(dev), rd[None].to(dev), bg_color=bg, max_steps=max_steps)
    assert out["image"].shape == (1, N, 3) and alb["image"].shape == (1, N, 4)      # 3 channels in latent mode
    assert torch.equal(out["depth"], alb["depth"]) and torch.equal(out["weights_sum"], alb["weights_sum"])
    err = (out["image"][0].cpu().double() - ref["image"]).abs().max(dim=-1)[0]
    tol = COMPOSITE_TOL(ref["counts"].double()) + 1e-3
    print("normal render: worst error %.3e (tolerance there %.3e), %d rays excluded"
          % (float(err[keep].max()), float(tol[keep][err[keep].argmax()]), int((~keep).sum())))
    assert bool((err[keep] <= tol[keep]).all()), float((err[keep] - tol[keep]).max())
    # no background: a ray that misses everything is black, whatever bg_color says
    miss = ref["counts"] == 0
    assert int(miss.sum()) > 0 and bool((out["image"][0].cpu()[miss] == 0).all())
    # the default and "albedo" are the render of before
    with torch.no_grad():
        alb2 = net.render(ro[None].to(dev), rd[None].to(dev), bg_color=bg, max_steps=max_steps, shading="albedo")
    assert torch.equal(alb2["image"], alb["image"])
    net.train()
    with pytest.raises(ValueError, match="evaluation render"):
        net.render(ro[None].to(dev), rd[None].to(dev), shading="normal", max_steps=max_steps)


# ------------------------------------------------------------------------------ 6. non-interference
def _trainer_cfg(tmp_path, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32,
            "render.eval_h": 32, "render.eval_w": 32, "render.grid_size": 64, "optim.iters": 60, "optim.lr": 5e-3,
            "log.save_interval": 30, "log.eval_size": 2, "log.full_eval_size": 3, "optim.fp16": False,
            "guide.text": "a lego man"}                                  # (test_gpu_trainer.py's smallest trainer)
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


def test_normal_query_leaves_training_state_alone(dev, tmp_path):
    """bf16 with the fragment-shadow optimiser and the fused table update: step, normal(points), step gives the bits of
    step, step -- parameters, both Adam moments and the bf16 shadow."""
    from src.latent_nerf.training.trainer import Trainer
    pts = _rand_points(5000, seed=9).to(dev)

    def run(name, query):
        tr = Trainer(_trainer_cfg(tmp_path, **{"optim.fp16": True, "optim.graph_step": False, "log.exp_name": name}),
                     device=dev)
        assert tr.nerf.precision == "bf16" and tr.nerf.encoder.fused_update is not None
        assert tr.nerf._frag_owner is not None
        tr.nerf.train()
        tr.nerf.update_extra_state()
        for k in range(2):
            tr.train_step += 1
            tr.optimizer.zero_grad()
            tr._eager_step()
            if k == 0 and query:
                n = tr.nerf.normal(pts)
                assert bool(torch.isfinite(n).all()) and float(n.abs().max()) > 0
        torch.cuda.synchronize()
        st = tr.optimizer.state_dict()
        params = [p.detach().clone() for g in tr.nerf.get_params(1.0) for p in g["params"]]
        return (params, [t.clone() for t in st["exp_avg"]], [t.clone() for t in st["exp_avg_sq"]],
                tr.nerf.encoder.shadow().clone(), [p.grad is None for g in tr.nerf.get_params(1.0) for p in g["params"]])

    a, b = run("plain", False), run("query", True)
    assert a[4] == b[4]
    for k, what in enumerate(("parameters", "exp_avg", "exp_avg_sq")):
        assert len(a[k]) == len(b[k])
        for i, (u, v) in enumerate(zip(a[k], b[k])):
            assert torch.equal(u, v), (what, i)
    assert torch.equal(a[3], b[3]), "bf16 shadow"
    assert float((a[0][0] - a[0][0].mean()).abs().max()) > 0


# ------------------------------------------------------------------------------ 7. mesh export
def test_export_mesh_with_field_normals(dev, tmp_path):
    net, lv, table, params = _field_net(dev, "f32", zero_table=True)          # the blob sphere
    thresh = net.cfg.density_thresh
    out = net.export_mesh(str(tmp_path / "m"), resolution=32, S=32, thresh=thresh, target_faces=400, field_normals=True)
    v, n = out["verts"].cpu(), out["normals"].cpu()
    assert 0 < out["faces"].shape[0] <= 400 and v.shape[0] > 50 and n.shape == v.shape
    cos = (n * v / v.norm(dim=-1, keepdim=True)).sum(-1)
    print("field normals on the blob sphere: min cos %.6f" % float(cos.min()))
    assert float(cos.min()) >= 0.999
    assert torch.equal(out["normals"], net.normal(out["verts"]))
    lines = open(tmp_path / "m" / "mesh.obj").read().splitlines()
    n_v, n_vn = sum(l.startswith("v ") for l in lines), sum(l.startswith("vn ") for l in lines)
    assert n_v == n_vn == v.shape[0]
    # the default is the export of before: the decimated mesh's own normals
    base = net.export_mesh(str(tmp_path / "b"), resolution=32, S=32, thresh=thresh, target_faces=400)
    assert torch.equal(base["verts"], out["verts"]) and not torch.equal(base["normals"], out["normals"])
    assert "normal_map" not in base
    # textured: an object-space normal map beside the albedo
    tex = net.export_mesh(str(tmp_path / "t"), resolution=32, S=32, thresh=thresh, target_faces=400,
                          texture_resolution=256, field_normals=True)
    assert (tmp_path / "t" / "normal_object.png").exists() and (tmp_path / "t" / "albedo.png").exists()
    nm, mask = tex["normal_map"], tex["mask"]
    assert nm.shape == (3, 256, 256)
    dec = (nm * 2.0 - 1.0).permute(1, 2, 0)[mask == 2]
    assert dec.shape[0] > 1000 and float((dec.norm(dim=-1) - 1).abs().max()) <= 1e-3
    plain = net.export_mesh(str(tmp_path / "p"), resolution=32, S=32, thresh=thresh, target_faces=400,
                            texture_resolution=256)
    assert not (tmp_path / "p" / "normal_object.png").exists() and "normal_map" not in plain
    assert open(tmp_path / "p" / "mesh.mtl").read() == open(tmp_path / "t" / "mesh.mtl").read()


# ------------------------------------------------------------------------------ 8. trainer flag
@pytest.mark.parametrize("flag", [True, False])
def test_trainer_eval_normals_flag(dev, tmp_path, flag):
    from PIL import Image
    from src.latent_nerf.training.trainer import Trainer
    over = {"optim.iters": 2, "log.save_interval": 2, "render.train_h": 16, "render.train_w": 16, "render.eval_h": 16,
            "render.eval_w": 16, "log.eval_size": 2, "log.full_eval_size": 1}
    if flag:
        over["log.eval_normals"] = True
    tr = Trainer(_trainer_cfg(tmp_path, **over), device=dev)
    tr.train()
    names = sorted(p.name for p in tr.eval_renders_path.iterdir())
    rgb = ["step_00002_0000_rgb.png", "step_00002_0001_rgb.png"]
    nrm = ["step_00002_0000_normals.png", "step_00002_0001_normals.png"]
    if not flag:
        assert names == rgb
        assert [p.name for p in tr.final_renders_path.iterdir() if "normals" in p.name] == []
        return
    assert names == sorted(rgb + nrm)
    for name in nrm:
        img = np.asarray(Image.open(tr.eval_renders_path / name))
        assert img.shape == (16, 16, 3) and img.min() != img.max()
    assert len(list(tr.final_renders_path.glob("step_00002_normals.*"))) == 1
