"""CPU checks of the oracle itself: integer parts against the scalar C restatement
(oracle/bits.c), structural properties of the march / encoding / compositing, and the
hand-derived compositing gradient (the one the HIP backward implements) against autograd."""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O


def _np_ptr(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def test_morton_roundtrip_and_c_oracle(bits_oracle):
    rng = np.random.RandomState(0)
    coords = rng.randint(0, 1024, size=(5000, 3)).astype(np.int32)
    coords[:4] = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1023, 1023, 1023]]
    idx = O.morton3d(torch.from_numpy(coords).long())
    assert idx[:3].tolist() == [0, 1, 2]
    out = np.zeros(len(coords), dtype=np.uint32)
    bits_oracle.oracle_morton3d(_np_ptr(coords, ctypes.c_int32), _np_ptr(out, ctypes.c_uint32),
                                ctypes.c_size_t(len(coords)))
    assert np.array_equal(out.astype(np.int64), idx.numpy())
    back = O.morton3d_invert(idx)
    assert torch.equal(back, torch.from_numpy(coords).long())
    inv = np.zeros_like(coords)
    bits_oracle.oracle_morton3d_invert(_np_ptr(out, ctypes.c_uint32), _np_ptr(inv, ctypes.c_int32),
                                       ctypes.c_size_t(len(coords)))
    assert np.array_equal(inv, coords)


def test_packbits_c_oracle(bits_oracle):
    g = torch.rand(4096) * 2
    bits = O.packbits(g, 1.0)
    out = np.zeros(512, dtype=np.uint8)
    arr = g.numpy().copy()
    bits_oracle.oracle_packbits(_np_ptr(arr, ctypes.c_float), ctypes.c_float(1.0), _np_ptr(out, ctypes.c_uint8),
                                ctypes.c_size_t(4096))
    assert np.array_equal(out, bits.numpy())
    assert int(bits[0]) == sum((1 << k) for k in range(8) if g[k] > 1.0)


def test_level_table_matches_survey():
    lv = O.make_grid_levels()
    assert lv.n_rows == 6119864
    assert lv.resolutions[0] == 16 and lv.resolutions[-1] == 2048
    assert [lv.offsets[i + 1] - lv.offsets[i] for i in range(5)] == [4920, 13824, 32768, 85184, 216000]
    assert all(lv.offsets[i + 1] - lv.offsets[i] == 2 ** 19 for i in range(5, 16))


def test_grid_index_c_oracle(bits_oracle):
    lv = O.make_grid_levels()
    rng = np.random.RandomState(1)
    bits_oracle.oracle_grid_index.restype = ctypes.c_uint32
    for l in (0, 3, 4, 5, 9, 15):
        res = lv.resolutions[l]
        hs = lv.offsets[l + 1] - lv.offsets[l]
        verts = rng.randint(0, res + 1, size=(2000, 3)).astype(np.int32)
        got = O.grid_corner_indices(torch.from_numpy(verts).long(), res, hs).numpy()
        out = np.zeros(len(verts), dtype=np.uint32)
        bits_oracle.oracle_grid_indices(_np_ptr(verts, ctypes.c_int32), _np_ptr(out, ctypes.c_uint32),
                                        ctypes.c_size_t(len(verts)), ctypes.c_uint32(res), ctypes.c_uint32(hs))
        assert np.array_equal(out.astype(np.int64), got)
        assert got.max() < hs
        if l < 5:  # dense levels are collision-free
            assert len(np.unique(got)) == len(np.unique(verts, axis=0))


def test_grid_encode_partition_of_unity_and_vertex_values():
    lv = O.make_grid_levels(num_levels=4, base_resolution=4, desired_resolution=32, log2_hashmap_size=10)
    x = torch.rand(500, 3)
    const = torch.full((lv.n_rows, 2), 0.75)
    f = O.grid_encode(x, const, lv)
    assert torch.allclose(f, torch.full_like(f, 0.75), atol=1e-6)
    # a sample exactly on a vertex of a dense level reads that vertex
    table = torch.randn(lv.n_rows, 2)
    l = 0
    res, scale = lv.resolutions[l], lv.scales[l]
    v = torch.tensor([[1, 2, 3]])
    xv = (v.float() - 0.5) / scale
    f = O.grid_encode(xv, table, lv)
    row = O.grid_corner_indices(v, res, lv.offsets[1] - lv.offsets[0]) + lv.offsets[0]
    assert torch.allclose(f[0, :2], table[row[0]], atol=1e-5)


def _small_scene(G=32, N=256, seed=0):
    torch.manual_seed(seed)
    grid = O.sphere_density_grid(G=G, radius=0.5)
    bits = O.packbits(grid.reshape(-1), 0.01)
    H = W = int(math.isqrt(N))
    f = H / (2 * math.tan(math.radians(55) / 2))
    c2w = O.pose_from_angles(math.radians(60), 0.3, 1.25)
    ro, rd = O.get_rays(c2w, f, f, W / 2, H / 2, H, W)
    return grid, bits, ro[0], rd[0]


@pytest.mark.parametrize("dt_gamma", [0.0, 1.0 / 64])
def test_march_properties(dt_gamma):
    G = 32
    grid, bits, ro, rd = _small_scene(G)
    nears, fars = O.near_far_from_aabb(ro, rd, [-1, -1, -1, 1, 1, 1], 0.1)
    max_steps = 256
    xyzs, dirs, deltas, rays, M = O.march_rays_train(ro, rd, nears, fars, bits, 1.0, 1, G, max_steps, dt_gamma,
                                                     torch.rand(ro.shape[0]))
    assert M == xyzs.shape[0] == int(rays[:, 2].sum()) and M > 0
    assert int(rays[:, 2].max()) <= max_steps
    # every sample sits in an occupied cell, inside the sphere's cell hull
    idx = O.march_cell_index(xyzs, deltas[:, 0], 1.0, 1, G)
    assert bool(((bits.long()[idx >> 3] >> (idx & 7)) & 1).all())
    # offsets are the exclusive scan of counts; t increases along each ray; x = o + t d
    cnt = rays[:, 2].long()
    assert torch.equal(rays[:, 1].long(), torch.cumsum(cnt, 0) - cnt)
    for n in torch.nonzero(cnt > 1)[:20, 0].tolist():
        o, c = int(rays[n, 1]), int(rays[n, 2])
        t = deltas[o:o + c, 1]
        assert bool((t[1:] > t[:-1]).all())
        assert torch.allclose(xyzs[o:o + c], ro[n] + t[:, None] * rd[n], atol=1e-6)
        assert bool((t >= nears[n]).all()) and bool((t < fars[n]).all())
    # rays that miss the box have no samples
    assert int(cnt[nears >= fars].sum()) == 0


def test_apply_capacity_keeps_all_or_drops_all():
    G = 32
    _, bits, ro, rd = _small_scene(G)
    nears, fars = O.near_far_from_aabb(ro, rd, [-1, -1, -1, 1, 1, 1], 0.1)
    rays, M = O.march_rays_train(ro, rd, nears, fars, bits, 1.0, 1, G, 256, 0.0, None)[3:]
    live = int((rays[:, 2] > 0).sum())
    assert M > 0 and 0 < live < rays.shape[0]
    for cap in (M, M + 1, 10 * M):   # room for everything: the input, untouched
        out, m, lv, dr = O.apply_capacity(rays, cap)
        assert torch.equal(out, rays) and (m, lv, dr) == (M, live, 0)
    out, m, lv, dr = O.apply_capacity(rays, 0)   # room for nothing: every non-empty ray goes, empty ones stay as they are
    assert (m, lv, dr) == (0, 0, live) and int(out[:, 2].sum()) == 0
    empty = rays[:, 2] == 0
    assert torch.equal(out[empty], rays[empty]) and int(out[~empty, 1].abs().sum()) == 0
    assert torch.equal(out[:, 0], rays[:, 0])


def test_march_max_steps_cap():
    # bound 2 (two cascades), fully occupied: the lattice has up to 2x max_steps points per ray,
    # so the per-ray sample cap binds
    G = 32
    full = torch.ones(2, G ** 3)
    bits = O.packbits(full.reshape(-1), 0.5)
    _, _, ro, rd = _small_scene(G, N=64)
    nears, fars = O.near_far_from_aabb(ro, rd, [-2, -2, -2, 2, 2, 2], 0.1)
    xyzs, dirs, deltas, rays, M = O.march_rays_train(ro, rd, nears, fars, bits, 2.0, 2, G, 64, 0.0, None)
    assert int(rays[:, 2].max()) == 64 and int(rays[:, 2].min()) > 0
    assert float(xyzs.abs().max()) <= 2.0


def test_composite_matches_sequential_definition_and_manual_gradient():
    torch.manual_seed(3)
    N, C = 7, 4
    cnts = torch.tensor([0, 5, 1, 70, 3, 0, 130])
    offs = torch.cumsum(cnts, 0) - cnts
    M = int(cnts.sum())
    rays = torch.stack([torch.tensor([3, 0, 6, 1, 5, 2, 4]), offs, cnts], -1).int()
    sig = (torch.rand(M) * 30).double().float().requires_grad_()
    rgb = torch.randn(M, C).requires_grad_()
    dl = torch.stack([torch.full((M,), 0.01), torch.rand(M) + 0.2], -1)
    bg = torch.rand(N, C)
    ws, dp, img = O.composite_rays_train(sig, rgb, dl, rays, 1e-4, bg)
    # sequential reference (the loop a per-ray thread would run)
    for r in range(N):
        rid, o, c = [int(v) for v in rays[r]]
        T, w_sum, d_sum, acc = 1.0, 0.0, 0.0, torch.zeros(C)
        for i in range(o, o + c):
            if T < 1e-4:
                break
            a = 1 - math.exp(-float(sig[i]) * float(dl[i, 0]))
            w = a * T
            w_sum += w; d_sum += w * float(dl[i, 1]); acc += w * rgb[i].detach()
            T *= 1 - a
        assert abs(float(ws[rid]) - w_sum) < 1e-5
        assert abs(float(dp[rid]) - d_sum) < 1e-5
        assert torch.allclose(img[rid], acc + (1 - w_sum) * bg[rid], atol=1e-5)
    # manual gradient (formula implemented by csrc/composite.hip) vs autograd
    g_ws, g_dp, g_img = torch.randn(N), torch.randn(N), torch.randn(N, C)
    (ws * g_ws).sum().add((dp * g_dp).sum()).add((img * g_img).sum()).backward()
    dsig = torch.zeros(M); drgb = torch.zeros(M, C)
    for r in range(N):
        rid, o, c = [int(v) for v in rays[r]]
        if c == 0:
            continue
        s, dt, t = sig[o:o + c].detach(), dl[o:o + c, 0], dl[o:o + c, 1]
        tau = s * dt
        excl = torch.cumsum(tau, 0) - tau
        T = torch.exp(-excl)
        keep = T >= 1e-4
        w = torch.where(keep, (1 - torch.exp(-tau)) * T, torch.zeros(1))
        g = g_ws[rid] + g_dp[rid] * t + ((rgb[o:o + c].detach() - bg[rid]) * g_img[rid]).sum(-1)
        total = (g * w).sum()
        pinc = torch.cumsum(g * w, 0)
        dtau = torch.where(keep, g * T * torch.exp(-tau) - (total - pinc), torch.zeros(1))
        dsig[o:o + c] = dt * dtau
        drgb[o:o + c] = w[:, None] * g_img[rid]
    assert torch.allclose(dsig, sig.grad, rtol=1e-4, atol=1e-6)
    assert torch.allclose(drgb, rgb.grad, rtol=1e-5, atol=1e-7)


def test_render_frame_small_and_grad_flow():
    G = 32
    grid, bits, ro, rd = _small_scene(G, N=64)
    lv = O.make_grid_levels(num_levels=16, base_resolution=4, desired_resolution=64, log2_hashmap_size=10)
    table = (torch.randn(lv.n_rows, 2) * 0.1).requires_grad_()
    mp = {k: v.requires_grad_() for k, v in O.init_mlp_params().items()}
    out = O.render_frame(ro, rd, table, mp, lv, bits, G=G, max_steps=128, bg_color=torch.rand(64, 4))
    assert out["image"].shape == (64, 4) and out["M"] > 0
    out["image"].backward(torch.randn(64, 4))
    assert table.grad.abs().sum() > 0 and all(v.grad is not None for v in mp.values())
    # rays that miss keep exactly the background
    miss = out["rays"][:, 2] == 0
    assert bool((out["weights_sum"][miss] == 0).all())


def test_trunc_exp_and_adam():
    x = torch.tensor([0.0, 10.0, 20.0], requires_grad=True)
    y = O.trunc_exp(x)
    y.sum().backward()
    assert torch.allclose(x.grad, torch.exp(torch.tensor([0.0, 10.0, 15.0])))
    p = torch.randn(100); g = torch.randn(100)
    ref = p.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=1e-2, betas=(0.9, 0.99), eps=1e-15)
    m = torch.zeros(100); v = torch.zeros(100); q = p.clone()
    for step in range(1, 4):
        ref.grad = g.clone()
        opt.step()
        q, m, v = O.adam_step(q, g, m, v, step, 1e-2)
    assert torch.allclose(q, ref.detach(), atol=1e-6)


def _infer_scene(N=400, seed=3, bound=2.0, miss_every=5):
    """Rays from a sphere of radius 2.5*bound towards jittered points inside the box; every `miss_every`-th ray
    points away from the box (near = far = FLT_MAX)."""
    g = torch.Generator().manual_seed(seed)
    eye = torch.randn(N, 3, generator=g)
    ro = 2.5 * bound * eye / eye.norm(dim=-1, keepdim=True)
    tgt = (torch.rand(N, 3, generator=g) - 0.5) * bound
    rd = tgt - ro
    rd[::miss_every] = ro[::miss_every]
    rd = rd / rd.norm(dim=-1, keepdim=True)
    return ro.float(), rd.float()


def _march_in_chunks(n_step, ro, rd, nears, fars, bits, bound, cascade, G, max_steps, dt_gamma):
    """Drive march_rays_infer the way the eval loop does (sigma 0: no ray dies before its padding), collecting the
    samples of every ray across the calls."""
    N = ro.shape[0]
    alive = torch.arange(N, dtype=torch.int32)
    rays_t = nears.clone()
    per_ray = [[] for _ in range(N)]
    ws, depth, image, T = torch.zeros(N), torch.zeros(N), torch.zeros(N, 1), torch.ones(N)
    step = 0
    while step < max_steps and alive.shape[0] > 0:
        k = min(n_step, max_steps - step)
        xyzs, dirs, deltas = O.march_rays_infer(alive, k, rays_t, ro, rd, fars, bits, bound, cascade, G, max_steps,
                                                dt_gamma)
        rows = torch.cat([xyzs, dirs, deltas], -1).reshape(alive.shape[0], k, 8)
        for i, n in enumerate(alive.tolist()):
            per_ray[n] += [r for r in rows[i] if float(r[7]) >= 0]
        new_alive, rays_t, ws, depth, image, T = O.composite_rays_infer(
            alive, k, rays_t, torch.zeros(alive.shape[0] * k), torch.zeros(alive.shape[0] * k, 1), deltas, ws, depth,
            image, T)
        alive = O.compact_rays(new_alive, alive.shape[0])
        step += k
    return per_ray


def _assert_same_ray_samples(got, want, dt_gamma):
    """Rows (xyz, dir, dt, t) of one ray from the inference march in chunks against the training march's.  With
    dt_gamma > 0 both walk the recurrence: bit for bit.  At dt_gamma = 0 the training march takes lattice point k in
    closed form, fl(fl(k dt) + t0), and the inference march by k additions, so t is the same number only up to their
    roundings: the step and the direction are bit for bit, t within (k / 2 + 1) 2^-24 t (half an ulp per addition
    against two roundings), x within that times |d| plus the two roundings of o + t d on either side."""
    if dt_gamma > 0:
        assert torch.equal(got, want)
        return
    assert torch.equal(got[:, 3:7], want[:, 3:7])
    g, w = got.double(), want.double()
    k = torch.round(w[:, 7] / w[:, 6])           # at most t / dt lattice points lie before a sample (near >= 0)
    tol_t = (k / 2 + 1) * 2.0 ** -24 * w[:, 7].clamp_min(1.0)
    assert bool(((g[:, 7] - w[:, 7]).abs() <= tol_t).all()), float(((g[:, 7] - w[:, 7]).abs() / tol_t).max())
    tol_x = w[:, 3:6].abs() * tol_t[:, None] + 2.0 ** -23 * (w[:, :3].abs() + (w[:, 7:8] * w[:, 3:6]).abs())
    assert bool(((g[:, :3] - w[:, :3]).abs() <= tol_x).all())


@pytest.mark.parametrize("bound,cascade,dt_gamma,G,max_steps", [
    pytest.param(1.0, 1, 1.0 / 64, 16, 96, id="1.0-1-0.015625"),
    pytest.param(2.0, 2, 1.0 / 128, 16, 96, id="2.0-2-0.0078125"),
    # dt_min > dt_max (max_steps < G / 2^(cascade-1)): one step rule, dt_max, in both marches -- at dt_gamma = 0 too
    pytest.param(1.0, 1, 0.0, 64, 16, id="inverted-64-16"),
    pytest.param(1.0, 1, 0.0, 128, 64, id="inverted-128-64"),
    pytest.param(1.0, 1, 1.0 / 64, 64, 16, id="inverted-64-16-gamma"),
])
def test_infer_march_in_chunks_equals_training_march(bound, cascade, dt_gamma, G, max_steps):
    """With dt_gamma > 0 both marches walk t = t + clamp(t*dt_gamma, dt_min, dt_max) from near: the inference march,
    restarted from the handed-over rays_t every n_step samples, emits exactly the training march's samples.  At
    dt_gamma = 0 they emit the same samples with the same step, t to the rounding of the two lattice forms
    (_assert_same_ray_samples)."""
    g = torch.Generator().manual_seed(11)
    bits = O.packbits((torch.rand(cascade * G ** 3, generator=g) < 0.8).float(), 0.5)
    ro, rd = _infer_scene(N=120, bound=bound)
    nears, fars = O.near_far_from_aabb(ro, rd, [-bound] * 3 + [bound] * 3, 0.1)
    xyzs, dirs, deltas, rays, M = O.march_rays_train(ro, rd, nears, fars, bits, bound, cascade, G, max_steps,
                                                     dt_gamma, None)
    # rays span several calls of every n_step, and with bound 2 (or a small max_steps) the per-ray cap binds
    assert int(rays[:, 2].max()) == max_steps if (bound > 1 or max_steps < 96) else int(rays[:, 2].max()) > 3 * 8
    assert int((rays[:, 2] == 0).sum()) >= 120 // 5  # and the misses have no samples
    if max_steps < G:   # the inverted regime: every step is dt_max
        dt_max = torch.tensor(2.0 * O.SQRT3 * (2 ** (cascade - 1)) / G, dtype=torch.float32)
        assert 2.0 * O.SQRT3 / max_steps > float(dt_max) and bool((deltas[:, 0] == dt_max).all())
    want = torch.cat([xyzs, dirs, deltas], -1)
    for n_step in (1, 3, 8):
        per_ray = _march_in_chunks(n_step, ro, rd, nears, fars, bits, bound, cascade, G, max_steps, dt_gamma)
        for n in range(ro.shape[0]):
            o, c = int(rays[n, 1]), int(rays[n, 2])
            assert len(per_ray[n]) == c, (n_step, n, len(per_ray[n]), c)
            if c:
                _assert_same_ray_samples(torch.stack(per_ray[n]), want[o:o + c], dt_gamma)


def test_infer_march_padding_and_dead_entries():
    G, bound = 16, 1.0
    bits = O.packbits(torch.ones(G ** 3), 0.5)
    ro, rd = _infer_scene(N=16, bound=bound, miss_every=4)
    nears, fars = O.near_far_from_aabb(ro, rd, [-bound] * 3 + [bound] * 3, 0.1)
    alive = torch.tensor([5, -1, 0, 3, -1, 4], dtype=torch.int32)
    xyzs, dirs, deltas = O.march_rays_infer(alive, 4, nears, ro, rd, fars, bits, bound, 1, G, 64, 0.0)
    pad = torch.tensor([0.0, 0, 0, 0, 0, 1, 0, -1])
    rows = torch.cat([xyzs, dirs, deltas], -1).reshape(6, 4, 8)
    for i, n in enumerate(alive.tolist()):
        if n < 0 or n % 4 == 0:   # dead entry, or a ray that misses the box: padding only
            assert torch.equal(rows[i], pad.expand(4, 8)), i
        else:
            assert bool((rows[i, :, 7] >= nears[n]).all()) and bool((rows[i, :, 6] > 0).all())
    assert torch.equal(O.compact_rays(alive, 6), torch.tensor([5, 0, 3, 4], dtype=torch.int32))
    assert torch.equal(O.compact_rays(alive, 2), torch.tensor([5], dtype=torch.int32))


def _fake_field(x):
    """Deterministic elementwise field (mul/add only): low density in a shell, higher near the centre."""
    r2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
    sigma = 0.25 + 16.0 / (1.0 + 4.0 * r2)
    rgb = torch.stack([0.5 + 0.25 * x[:, 0], 0.5 - 0.25 * x[:, 1], 0.25 + 0.125 * x[:, 2], 0.125 * r2], -1)
    return sigma, rgb


def test_render_frame_infer_is_independent_of_the_chunking():
    """The eval loop's per-call state (rays_t, T, weights_sum, depth, image) is carried so that how the samples of a
    ray are split over calls does not change a bit of its result; no ray takes more than max_steps samples."""
    G, bound, cascade, max_steps = 16, 2.0, 2, 48
    bits = O.packbits(torch.ones(cascade * G ** 3), 0.5)
    ro, rd = _infer_scene(N=200, bound=bound)
    bg = torch.rand(200, 4, generator=torch.Generator().manual_seed(2))
    kw = dict(bitfield=bits, bound=bound, cascade=cascade, G=G, max_steps=max_steps, dt_gamma=1.0 / 128, bg_color=bg)
    ref = O.render_frame_infer(ro, rd, _fake_field, **kw)
    assert int(ref["counts"].max()) == max_steps                   # the cap binds on some rays,
    assert bool((ref["transmittance"] < 1e-4).any())               # some die by T_thresh,
    assert int((ref["counts"] == 0).sum()) >= 200 // 5             # and the misses take no sample
    scheds = [lambda N, a, s: 1, lambda N, a, s: min(3, max_steps - s), lambda N, a, s: min(8, max_steps - s),
              lambda N, a, s: O.renderer_schedule(N, a, s, max_steps),
              lambda N, a, s: min(1 + (s % 7), max_steps - s)]
    for sched in scheds:
        out = O.render_frame_infer(ro, rd, _fake_field, schedule=sched, **kw)
        for k in ("image", "depth", "weights_sum", "transmittance", "counts"):
            assert torch.equal(out[k], ref[k]), k
