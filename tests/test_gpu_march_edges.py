"""The training march on the GPU at its geometric edges (tests/march_reference.py): every case through the table form
and the `_aabb` form into poisoned buffers -- equal to the oracle bit for bit, accepted by the float64 lattice-point
reference, nothing written outside the kept spans --, one case per configuration again under capacity M // 3, and the
inference march in chunks against the training march where dt_min > dt_max.  Run with `pytest -m gpu` on an MI355X."""
import pytest
import torch

from oracle import nerf_oracle as O
from tests import march_reference as R

pytestmark = pytest.mark.gpu

_POISON = 0x7FC0BEEF   # a NaN no march computes (test_gpu_parity._poisoned_buffers)
_SLACK = 64            # rows behind the last sample that must stay poisoned


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _poisoned_buffers(dev, N, capacity):
    from src.latent_nerf.raymarching import backend as B, raymarching as rm
    buf = lambda c: torch.full((capacity, c), _POISON, dtype=torch.int32, device=dev).view(torch.float32)
    return rm.MarchResult(buf(3), buf(3), buf(2), torch.empty(N, 3, dtype=torch.int32, device=dev),
                          torch.zeros(int(B.get_lib().lnerf_march_counter_len(N)), dtype=torch.int32, device=dev), capacity)


def _gpu_march(dev, case, form, size, capacity):
    """The GPU march of a case into poisoned buffers of `size` rows under `capacity` -> MarchOut of CPU tensors."""
    from src.latent_nerf.raymarching import raymarching as rm
    bound, cascade, G, max_steps, dt_gamma = case.cfg
    N = case.ro.shape[0]
    out = _poisoned_buffers(dev, N, size)
    out.capacity = capacity
    kw = dict(dt_gamma=dt_gamma, max_steps=max_steps, capacity=capacity, noises=case.noises.to(dev), out=out)
    if form == "table":
        nears, fars = O.near_far_from_aabb(case.ro, case.rd, list(case.box), R.MIN_NEAR)
        res = rm.march_rays_train(case.ro.to(dev), case.rd.to(dev), bound, case.bits.to(dev), cascade, G, nears.to(dev),
                                  fars.to(dev), **kw)
    else:
        res = rm.march_rays_train(case.ro.to(dev), case.rd.to(dev), bound, case.bits.to(dev), cascade, G, None, None,
                                  aabb=list(case.box), min_near=R.MIN_NEAR, **kw)
    assert res.xyzs.data_ptr() == out.xyzs.data_ptr() and res.xyzs.shape[0] == size   # marched into the poisoned buffers
    return R.MarchOut(res.rays.cpu(), res.xyzs.cpu(), res.dirs.cpu(), res.deltas.cpu(), res.counter.cpu())


def _assert_is_the_oracles(got, want, want_rays):
    """Kept spans hold the oracle's samples bit for bit; every other row of the buffers is still poison."""
    assert torch.equal(got.rays, want_rays)
    written = torch.zeros(got.xyzs.shape[0], dtype=torch.bool)
    source = torch.zeros(want.xyzs.shape[0], dtype=torch.bool)
    for (o, c), (wo, _) in zip(want_rays[:, 1:].tolist(), want.rays[:, 1:].tolist()):
        written[o:o + c] = True          # (a kept ray keeps the offset of the march without a capacity)
        source[wo:wo + c] = True
        assert c == 0 or o == wo
    assert int(written.sum()) == int(want_rays[:, 2].sum())
    for g, w in ((got.xyzs, want.xyzs), (got.dirs, want.dirs), (got.deltas, want.deltas)):
        gi, wi = g.contiguous().view(torch.int32), w.contiguous().view(torch.int32)
        assert torch.equal(gi[written], wi[source])
        assert bool((gi[~written] == _POISON).all())


@pytest.mark.parametrize("name", R.case_names())
def test_march_edge_case(dev, name):
    case, want = R.build_case(name), R.oracle_march(name)
    M = int(want.rays[:, 2].sum())
    for form in ("table", "aabb"):
        got = _gpu_march(dev, case, form, M + _SLACK, M + _SLACK)
        st = R.assert_case(name, got, capacity=M + _SLACK)
        _assert_is_the_oracles(got, want, want.rays)
        assert got.counter[:4].tolist() == [M, int((want.rays[:, 2] > 0).sum()), 0, M]
        s = case.ref.stats
        print("%-28s %-5s lattice %7d free %6.3f%% must %6.2f%% of occupied; samples %6d, on free points %d" % (
            name, form, s["lattice"], 100 * s["free_share"], 100 * s["must_share"], st["samples"], st["on_free"]))
        assert st["samples"] == M


@pytest.mark.parametrize("name", R.capacity_case_names())
def test_march_edge_case_under_capacity(dev, name):
    case, want = R.build_case(name), R.oracle_march(name)
    cap = int(want.rays[:, 2].sum()) // 3
    rays, m, live, dropped = O.apply_capacity(want.rays, cap)
    assert live > 0 and dropped > 0
    for form in ("table", "aabb"):
        got = _gpu_march(dev, case, form, cap + _SLACK, cap)
        R.assert_case(name, got, capacity=cap, raw_rays=want.rays)
        _assert_is_the_oracles(got, want, rays)
        assert got.counter[:4].tolist() == [m, live, dropped, m | (1 << 30)]


def _infer_in_chunks(dev, case, n_step):
    """lnerf_march_rays driven as the eval loop drives it (no ray dies before its padding): n_step samples per call
    from the handed-over rays_t = t + dt of the last sample, max_steps in all.  Per-ray [count, 8] rows."""
    from src.latent_nerf.raymarching import raymarching as rm
    bound, cascade, G, max_steps, dt_gamma = case.cfg
    N = case.ro.shape[0]
    nears, fars = O.near_far_from_aabb(case.ro, case.rd, list(case.box), R.MIN_NEAR)
    ro, rd, fars_d, bits = case.ro.to(dev), case.rd.to(dev), fars.to(dev), case.bits.to(dev)
    alive = torch.arange(N, dtype=torch.int32)
    rays_t = nears.clone()
    per_ray = [[] for _ in range(N)]
    step = 0
    while step < max_steps and alive.shape[0] > 0:
        k = min(n_step, max_steps - step)
        xyzs, dirs, deltas = rm.march_rays(alive.shape[0], k, alive.to(dev), rays_t.to(dev), ro, rd, bound, bits,
                                           cascade, G, fars_d, dt_gamma, max_steps)
        rows = torch.cat([xyzs, dirs, deltas], -1).cpu().reshape(alive.shape[0], k, 8)
        full = rows[:, :, 7] >= 0
        for i, n in enumerate(alive.tolist()):
            per_ray[n].append(rows[i][full[i]])
        keep = full.all(1)                         # a padded row: the ray has run past far
        last = rows[:, k - 1]
        rays_t[alive[keep].long()] = (last[:, 7] + last[:, 6])[keep]
        alive = alive[keep]
        step += k
    return [torch.cat(r, 0) for r in per_ray]


@pytest.mark.parametrize("n_step", [1, 5])
@pytest.mark.parametrize("name", ["inverted16-random30", "inverted64-random30", "inverted64-full", "plain-random30"])
def test_infer_march_in_chunks_equals_training_march_on_the_gpu(dev, name, n_step):
    """lnerf_march_rays in chunks emits the training march's samples where dt_min > dt_max too (both step by dt_max;
    `plain` is the usual regime beside them): the same rays, no jitter.  Both outputs pass the float64 reference, take
    the same lattice points except FREE ones (the diagonal ray steps from cell corner to cell corner), and on a common
    point the step and the direction agree bit for bit.  t is the same number only up to the rounding of the two lattice
    forms at dt_gamma = 0 -- fl(fl(k dt) + t0) against k additions --: within (k / 2 + 1) 2^-24 max(t, 1), and x within
    that times |d| plus the two roundings of o + t d on either side."""
    import numpy as np
    case = R.build_case(name)
    zero = torch.zeros_like(case.noises)
    ref = R.build_reference(case.ro, case.rd, zero, case.bits, case.cfg, case.box)
    case = case._replace(noises=zero, ref=ref)
    N, max_steps = case.ro.shape[0], case.cfg[3]
    cap = N * max_steps
    train = _gpu_march(dev, case, "table", cap, cap)
    kt = R.assert_march(ref, train.rays, train.xyzs, train.dirs, train.deltas, train.counter, cap)["matched"]
    per_ray = _infer_in_chunks(dev, case, n_step)
    counts = torch.tensor([r.shape[0] for r in per_ray])
    offsets = torch.cumsum(counts, 0) - counts
    rows = torch.cat(per_ray, 0)
    rays = torch.stack([torch.arange(N), offsets, counts], -1).to(torch.int32)
    counter = torch.tensor([int(counts.sum()), int((counts > 0).sum()), 0], dtype=torch.int32)
    ki = R.assert_march(ref, rays, rows[:, :3].contiguous(), rows[:, 3:6].contiguous(), rows[:, 6:8].contiguous(),
                        counter, cap)["matched"]
    assert int(counts.max()) > 2 * n_step and int(counts.sum()) > 500
    dt_min, dt_max = R.step_constants(case.cfg[1], case.cfg[2], max_steps)
    assert bool((rows[:, 6] == min(dt_min, dt_max)).all()) and bool((train.deltas[:int(train.counter[0]), 0] == min(dt_min, dt_max)).all())
    want = torch.cat([train.xyzs, train.dirs, train.deltas], -1)
    differing = 0
    for n in range(N):
        a, b = kt[n], ki[n]
        # up to the earlier of the two last samples (a cap ends the ray there), a point taken by one march only is FREE
        lim = min(a[-1] if len(a) == max_steps else 1 << 30, b[-1] if len(b) == max_steps else 1 << 30)
        only = np.setxor1d(a, b)
        only = only[only <= lim]
        assert bool((ref.cls[n, only] == R.FREE).all()), (n, only, ref.cls[n, only])
        differing += len(only) > 0
        common, ia, ib = np.intersect1d(a, b, return_indices=True)
        if len(common) == 0:
            continue
        w = want[int(train.rays[n, 1]) + torch.from_numpy(ia)].double()
        g = per_ray[n][torch.from_numpy(ib)].double()
        assert torch.equal(g[:, 3:7], w[:, 3:7]), n
        tol_t = (torch.from_numpy(common).double() / 2 + 1) * 2.0 ** -24 * w[:, 7].clamp_min(1.0)
        assert bool(((g[:, 7] - w[:, 7]).abs() <= tol_t).all()), (n, float(((g[:, 7] - w[:, 7]).abs() / tol_t).max()))
        tol_x = w[:, 3:6].abs() * tol_t[:, None] + 2.0 ** -23 * (w[:, :3].abs() + (w[:, 7:8] * w[:, 3:6]).abs())
        assert bool(((g[:, :3] - w[:, :3]).abs() <= tol_x).all()), n
    assert differing <= 2, differing   # the diagonal ray; every other ray takes the same lattice points in both marches
