"""The inference ray loop (csrc/rays.hip k_march_rays / k_composite_rays / k_compact_rays, driven by the eval branch of
NeRFRenderer.run_cuda) against the oracle's restatement (oracle/nerf_oracle.py march_rays_infer, composite_rays_infer,
compact_rays, render_frame_infer).

The march and the compaction are bit-exact.  The composite is compared with a float64 reference; its tolerance
follows from the kernel's arithmetic.  Per sample the kernel forms e = __expf(-sigma dt) (v_exp_f32 of a rounded
product: a few ulp), alpha = 1 - e and T *= 1 - alpha.  The inputs keep sigma dt <= 1.5, so 1 - alpha >= 0.22 and the
two roundings of 1 - (1 - e) cost at most 2^-24 / 0.22 relative: every factor of T is within ~12 ulp (12 * 2^-24)
of exp(-sigma dt), and each w = alpha T and each f32 accumulate adds a few ulp more.  So after k samples the relative
error of T and the error of weights_sum / depth / image relative to their scale is below 32 * 2^-24 per sample:
COMPOSITE_TOL(k) = 32 * 2^-24 * (k + 1) ~= 1.9e-6 (k + 1).  Kill decisions (T < T_thresh) are compared exactly, so
the inputs are checked to keep every reference T at least 1e-3 (relative) away from T_thresh, far outside that."""
import math

import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24


def COMPOSITE_TOL(k):
    return 32 * ULP * (k + 1)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _scene(N, bound, seed, miss_every=7):
    """Rays from a sphere of radius 2.5*bound towards jittered points in the box; every `miss_every`-th ray points
    away from it (near = far = FLT_MAX)."""
    g = torch.Generator().manual_seed(seed)
    eye = torch.randn(N, 3, generator=g)
    ro = 2.5 * bound * eye / eye.norm(dim=-1, keepdim=True)
    rd = (torch.rand(N, 3, generator=g) - 0.5) * bound - ro
    rd[::miss_every] = ro[::miss_every]
    rd = rd / rd.norm(dim=-1, keepdim=True)
    return ro.float().contiguous(), rd.float().contiguous()


# ------------------------------------------------------------------------------------------------------ march
@pytest.mark.parametrize("bound,cascade", [(1.0, 1), (2.0, 2)])
@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
@pytest.mark.parametrize("n_step", [1, 3, 8])
def test_march_rays_bit_exact(dev, bound, cascade, dt_gamma, n_step):
    from src.latent_nerf.raymarching import raymarching as rm
    G, max_steps, N = 32, 128, 6000
    g = torch.Generator().manual_seed(17 + n_step)
    bits = O.packbits((torch.rand(cascade * G ** 3, generator=g) < 0.6).float(), 0.5)
    ro, rd = _scene(N, bound, seed=n_step + cascade)
    nears, fars = O.near_far_from_aabb(ro, rd, [-bound] * 3 + [bound] * 3, 0.1)
    hit = nears < fars
    # rays_t part-way along the ray, as an earlier call leaves it; some at or past far (padding from the start)
    u = torch.rand(N, generator=g)
    rays_t = torch.where(hit, nears + (fars - nears) * (u * 1.1 - 0.05).clamp(0, 1.05), nears)
    rays_t[::11] = torch.where(hit[::11], fars[::11], nears[::11])
    # a ray that reaches far inside the call: its rows after the last lattice point are padding
    assert int((hit & (rays_t >= fars)).sum()) > 0
    for n_alive in (1, 255, 257, 5000):
        alive = torch.randperm(N, generator=g)[:n_alive].to(torch.int32)
        alive[torch.rand(n_alive, generator=g) < 0.1] = -1
        xyzs, dirs, deltas = rm.march_rays(n_alive, n_step, alive.to(dev), rays_t.to(dev), ro.to(dev), rd.to(dev),
                                           bound, bits.to(dev), cascade, G, fars.to(dev), dt_gamma, max_steps)
        rx, rdirs, rdl = O.march_rays_infer(alive, n_step, rays_t, ro, rd, fars, bits, bound, cascade, G, max_steps,
                                            dt_gamma)
        assert torch.equal(xyzs.cpu(), rx), n_alive
        assert torch.equal(dirs.cpu(), rdirs), n_alive
        assert torch.equal(deltas.cpu(), rdl), n_alive
        if n_alive == 5000:   # every kind of row is present: samples, padding after far, dead and missed entries
            real = (rdl[:, 1] >= 0).reshape(n_alive, n_step)
            assert bool(real.all(1).any()) and bool((real.any(1) & ~real.all(1)).any()) or n_step == 1
            assert bool((~real.any(1)).any())


# -------------------------------------------------------------------------------------------------- composite
def _composite_inputs(A, n_step, C, seed):
    """Entries of a permuted rays_alive over 3A rays (10 % dead); incoming state with T < 1 and non-zero sums;
    sigma dt <= 1.5; padding tails on a fifth of the entries; some entries start with T near T_thresh so that they
    die in the middle of the chunk."""
    g = torch.Generator().manual_seed(seed)
    N = 3 * A
    alive = torch.randperm(N, generator=g)[:A].to(torch.int32)
    alive[torch.rand(A, generator=g) < 0.1] = -1
    T = torch.exp(-torch.rand(N, generator=g) * 3.0)
    low = torch.rand(N, generator=g) < 0.3
    T[low] = 1e-4 * (1.5 + 20.0 * torch.rand(int(low.sum()), generator=g))
    ws = (1.0 - T) * (0.9 + 0.1 * torch.rand(N, generator=g))
    depth = torch.rand(N, generator=g) * 3.0
    image = torch.rand(N, C, generator=g)
    rays_t = 0.5 + torch.rand(N, generator=g) * 2.0
    sig = torch.rand(A * n_step, generator=g) * 3.0
    sig[torch.rand(A * n_step, generator=g) < 0.2] = 0.0
    dt = 0.02 + torch.rand(A * n_step, generator=g) * 0.48
    t = (rays_t[alive.clamp(min=0).long()][:, None] + torch.arange(n_step) * 0.5).reshape(-1)
    deltas = torch.stack([dt, t], -1)
    pad_from = torch.randint(0, n_step + 1, (A,), generator=g)
    pad_from[torch.rand(A, generator=g) > 0.2] = n_step
    padrow = (torch.arange(n_step)[None, :] >= pad_from[:, None]).reshape(-1)
    deltas[padrow] = torch.tensor([0.0, -1.0])
    rgbs = torch.rand(A * n_step, C, generator=g)
    return alive, rays_t, sig, rgbs, deltas, ws, depth, image, T


def _t_margin(alive, sig, deltas, T, n_step, T_thresh):
    """Smallest |T_k / T_thresh - 1| over the float64 T before and after each composited sample."""
    A = alive.shape[0]
    m = math.inf
    for i in range(A):
        n = int(alive[i])
        if n < 0:
            continue
        Tk = float(T[n])
        m = min(m, abs(Tk / T_thresh - 1))
        for s in range(n_step):
            dt, t = float(deltas[i * n_step + s, 0]), float(deltas[i * n_step + s, 1])
            if t < 0:
                break
            Tk *= math.exp(-float(sig[i * n_step + s]) * dt)
            m = min(m, abs(Tk / T_thresh - 1))
            if Tk < T_thresh:
                break
    return m


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("n_step", [1, 3, 8])
def test_composite_rays_matches_float64(dev, C, n_step):
    from src.latent_nerf.raymarching import raymarching as rm
    A, T_thresh = 700, 1e-4
    alive, rays_t, sig, rgbs, deltas, ws, depth, image, T = _composite_inputs(A, n_step, C, seed=C * 10 + n_step)
    assert _t_margin(alive, sig, deltas, T, n_step, T_thresh) > 1e-3   # no kill decision within rounding distance
    ref = O.composite_rays_infer(alive, n_step, rays_t, sig, rgbs, deltas, ws, depth, image, T, T_thresh)
    r_alive, r_t, r_ws, r_depth, r_image, r_T = ref
    # the cases are all there: killed by T_thresh mid-chunk, killed by padding, survivors and dead entries
    died = (r_alive < 0) & (alive >= 0)
    by_T = died & (r_T[alive.clamp(min=0).long()] < T_thresh)
    assert int(by_T.sum()) > 0 and int((died & ~by_T).sum()) > 0 and int((r_alive >= 0).sum()) > 0
    assert int((alive < 0).sum()) > 0
    g = [x.to(dev).contiguous() for x in (alive, rays_t, ws, depth, image, T)]
    rm.composite_rays(A, n_step, g[0], g[1], sig.to(dev), rgbs.to(dev), deltas.to(dev), g[2], g[3], g[4], g[5], T_thresh)
    k_alive, k_t, k_ws, k_depth, k_image, k_T = [x.cpu() for x in g]
    assert torch.equal(k_alive, r_alive)
    assert torch.equal(k_t, r_t)
    # state rows of rays without a live entry are untouched, bit for bit
    untouched = torch.ones(3 * A, dtype=torch.bool)
    untouched[alive[alive >= 0].long()] = False
    for k, r in ((k_ws, ws), (k_depth, depth), (k_image, image), (k_T, T)):
        assert torch.equal(k[untouched], r[untouched])
    tol = COMPOSITE_TOL(n_step)
    assert float(((k_T.double() - r_T).abs() / r_T).max()) <= tol
    assert float((k_ws.double() - r_ws).abs().max()) <= tol * float(r_ws.abs().max())
    assert float((k_depth.double() - r_depth).abs().max()) <= tol * float(r_depth.abs().max())
    assert float((k_image.double() - r_image).abs().max()) <= tol * float(r_image.abs().max())


# ---------------------------------------------------------------------------------------------------- compact
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 262145])
def test_compact_rays_bit_exact(dev, n):
    from src.latent_nerf.raymarching import raymarching as rm
    g = torch.Generator().manual_seed(n)
    size = n + 37
    fills = {"mixed": None, "dead": -1, "alive": 1} if n in (1, 4097) else {"mixed": None}
    for kind, fill in fills.items():
        a = torch.randperm(size, generator=g).to(torch.int32)   # non-negative junk past n must be ignored
        if fill is None:
            a[:n][torch.rand(n, generator=g) < 0.4] = -1
        elif fill < 0:
            a[:n] = -1
        out = torch.full((size,), -7, dtype=torch.int32, device=dev)
        cnt = torch.full((1,), -7, dtype=torch.int32, device=dev)
        out, cnt = rm.compact_rays(a.to(dev), n, out, cnt)
        want = O.compact_rays(a, n)
        k = int(cnt.item())
        assert k == want.shape[0], (kind, k)
        assert torch.equal(out[:k].cpu(), want), kind
        assert bool((out[k:] == -7).all()), kind     # nothing written past the count


# --------------------------------------------------------------------------------------------- argument checks
def test_inference_ops_refuse_bad_arguments_without_launching(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    z = lambda *s, dt=torch.float32: torch.full(s, 5.0, dtype=dt, device=dev)  # noqa: E731
    alive = torch.zeros(4, dtype=torch.int32, device=dev)
    xyzs = z(12, 3)
    bits = torch.full((32 ** 3 // 8,), 255, dtype=torch.uint8, device=dev)
    ro, t = z(4, 3), z(4)

    def march(n_step, ptr=True):
        return ("lnerf_march_rays", 4, n_step, _p(alive), _p(t), _p(ro), _p(ro), _p(t), _p(bits) if ptr else None,
                1.0, 1, 32, 64, 0.0, _p(xyzs), _p(xyzs), _p(xyzs), None)

    def composite(C, ptr=True):
        return ("lnerf_composite_rays", 4, 1, _p(alive), _p(t), _p(t), _p(xyzs), _p(xyzs), C, 1e-4, _p(t), _p(t),
                _p(xyzs) if ptr else None, _p(t), None)
    for call, msg in ((march(0), "n_step"), (march(3, ptr=False), "null pointer"), (composite(5), "C must be"),
                      (composite(3, ptr=False), "null pointer"),
                      (("lnerf_compact_rays", _p(alive), 4, None, _p(alive), None), "null pointer")):
        with pytest.raises(_b.LnerfError, match=msg):
            _b.call(*call)
        assert msg.split()[0] in _b.get_lib().lnerf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((xyzs == 5.0).all()) and bool((t == 5.0).all()) and bool((alive == 0).all())


# ------------------------------------------------------------------------------------ the eval loop, end to end
def _net(dev, G, bound, seed=0, log2_T=12, base_res=16, sphere=True):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(seed)
    cfg = RenderConfig(grid_size=G, train_h=16, train_w=16, bound=bound)
    net = NeRFNetwork(cfg, base_resolution=base_res, log2_hashmap_size=log2_T)
    net.encoder.embeddings.data.normal_(0, 0.1)
    net = net.to(dev).eval()
    cascade = net.cascade
    if sphere:
        grid = O.density_grid_from_function(lambda x: (x.norm(dim=-1) < 0.5 * bound).float() * 10.0, G, cascade, bound)
        bits = O.packbits(grid.reshape(-1), 0.01)
    else:
        grid = torch.full((cascade, G ** 3), 10.0)
        bits = torch.full((cascade * G ** 3 // 8,), 255, dtype=torch.uint8)
    net.density_grid.copy_(grid.to(dev))
    net.density_bitfield.copy_(bits.to(dev))
    return net, cascade, bits


def _fake_field(x):
    """Deterministic elementwise field of xyz (mul/add only, so the CPU and the GPU agree to rounding): low density,
    so no ray of the test frame dies before max_steps."""
    r2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
    sigma = 0.2 + 0.02 * r2
    rgb = torch.stack([0.5 + 0.25 * x[:, 0], 0.5 - 0.25 * x[:, 1], 0.25 + 0.125 * x[:, 2], 0.125 * r2], -1)
    return sigma, rgb


def _miss_frame(n_hit, bound, seed):
    """n_hit rays through the middle of the box, followed by 7 * n_hit that miss it: the first march has n_step 1,
    every later one 8 (N // n_alive = 8)."""
    g = torch.Generator().manual_seed(seed)
    eye = torch.randn(n_hit, 3, generator=g)
    ro_h = 2.5 * bound * eye / eye.norm(dim=-1, keepdim=True)
    rd_h = (torch.rand(n_hit, 3, generator=g) - 0.5) * 0.3 * bound - ro_h
    eye = torch.randn(7 * n_hit, 3, generator=g)
    ro_m = 2.5 * bound * eye / eye.norm(dim=-1, keepdim=True)
    ro, rd = torch.cat([ro_h, ro_m]), torch.cat([rd_h, ro_m])
    return ro.float(), (rd / rd.norm(dim=-1, keepdim=True)).float()


@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 128])
def test_eval_loop_with_a_fixed_field_is_schedule_independent_and_capped(dev, monkeypatch, dt_gamma):
    """7/8 of the rays miss the box, so after the first march the live rays take 8 samples per call: with
    max_steps 32 the loop's last chunk would take them to 33.  Every ray must take exactly the samples the oracle
    gives it (the first max_steps occupied lattice points), whatever frame it is rendered in and in whatever order."""
    from src.latent_nerf.raymarching import raymarching as rm
    G, bound, max_steps, n_hit = 16, 2.0, 32, 16
    net, cascade, bits = _net(dev, G, bound, sphere=False)
    assert cascade == 2
    monkeypatch.setattr(net, "field", lambda xyzs, m_host, *a: _fake_field(xyzs))
    counts = {}
    orig = rm.march_rays

    def counting(n_alive, n_step, rays_alive, *a, **k):
        xyzs, dirs, deltas = orig(n_alive, n_step, rays_alive, *a, **k)
        real = (deltas[:, 1] >= 0).reshape(n_alive, n_step).sum(1).cpu()
        for n, c in zip(rays_alive[:n_alive].cpu().tolist(), real.tolist()):
            counts[n] = counts.get(n, 0) + c
        return xyzs, dirs, deltas

    monkeypatch.setattr(rm, "march_rays", counting)
    ro, rd = _miss_frame(n_hit, bound, seed=3)
    N = ro.shape[0]
    bg = torch.rand(N, 4, generator=torch.Generator().manual_seed(4))

    def render(idx):
        counts.clear()
        with torch.no_grad():
            out = net.run_cuda(ro[idx].to(dev), rd[idx].to(dev), dt_gamma=dt_gamma, bg_color=bg[idx].to(dev),
                               max_steps=max_steps)
        c = torch.zeros(len(idx), dtype=torch.int64)
        for n, k in counts.items():
            c[n] = k
        return {k: out[k].cpu() for k in ("image", "depth", "weights_sum")}, c

    ref = O.render_frame_infer(ro, rd, _fake_field, bitfield=bits, bound=bound, cascade=cascade, G=G,
                               max_steps=max_steps, dt_gamma=dt_gamma, bg_color=bg)
    assert bool((ref["counts"][:n_hit] == max_steps).all())      # the cap binds on every hitting ray
    assert bool((ref["transmittance"][:n_hit] > 0.1).all())      # and none of them dies by T_thresh first
    full, c_full = render(torch.arange(N))
    assert int(c_full.max()) <= max_steps, "a ray took more than max_steps samples"
    assert torch.equal(c_full, ref["counts"])
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(5))
    shuf, c_shuf = render(perm)
    alone, c_alone = render(torch.arange(n_hit))                # n_step 1 on every call
    assert torch.equal(c_alone, ref["counts"][:n_hit])
    inv = torch.argsort(perm)
    for k in ("image", "depth", "weights_sum"):
        assert torch.equal(shuf[k][inv], full[k]), k
        assert torch.equal(alone[k], full[k][:n_hit]), k
    tol = COMPOSITE_TOL(max_steps)
    for k in ("image", "depth", "weights_sum"):
        r = ref[k]
        assert float((full[k].double() - r).abs().max()) <= tol * float(r.abs().max()), k


@pytest.mark.parametrize("cfg", ["small", "cascade2"])
def test_eval_render_matches_oracle(dev, cfg):
    """The real field (HIP grid encoder + MLP) through the whole eval loop, at the tolerances of
    test_render_train_matches_oracle."""
    if cfg == "small":
        G, bound, dt_gamma, HW = 32, 1.0, 0.0, 16
    else:
        G, bound, dt_gamma, HW = 32, 2.0, 1.0 / 128, 20
    net, cascade, bits = _net(dev, G, bound, seed=6)
    lv = O.make_grid_levels(16, 2, 16, 2048 * bound, 12)     # the encoder's finest level scales with the bound
    assert lv.offsets == net.encoder.levels.offsets
    params = {k: getattr(net, k).detach().cpu().clone() for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    table = net.encoder.embeddings.detach().cpu().clone()
    f = HW / (2 * math.tan(math.radians(55) / 2))
    c2w = O.pose_from_angles(math.radians(60), 0.3, 1.25 * bound)
    ro, rd = O.get_rays(c2w, f, f, HW / 2, HW / 2, HW, HW)
    ro, rd = ro[0], rd[0]
    N = HW * HW
    bg = torch.rand(N, 4, generator=torch.Generator().manual_seed(8))
    with torch.no_grad():
        out = net.run_cuda(ro.to(dev), rd.to(dev), dt_gamma=dt_gamma, bg_color=bg.to(dev))
    ref = O.render_frame_infer(ro, rd, None, table=table, mlp_params=params, lv=lv, bitfield=bits, bound=bound,
                               cascade=cascade, G=G, dt_gamma=dt_gamma, bg_color=bg)
    assert int((ref["counts"] > 0).sum()) > N // 8 and float(ref["weights_sum"].max()) > 0.5

    def err(a, b):
        return float((a.cpu().double() - b).abs().max()), float(b.abs().max())
    e, s = err(out["image"], ref["image"])
    assert e <= 1e-4 * max(s, 1.0), ("image", e, s)
    e, s = err(out["weights_sum"], ref["weights_sum"])
    assert e <= 1e-4, ("weights_sum", e)
    e, s = err(out["depth"], ref["depth"])
    assert e <= 2e-4 * max(s, 1.0), ("depth", e, s)
