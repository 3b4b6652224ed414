"""The occupancy refresh (update_extra_state() and the kernels of csrc/occupancy.hip) at production
sizes and in its steady state, against oracle/nerf_oracle.py and tests/occupancy_reference.py.  Every comparison is on
bits (tensor.view(torch.int32)) but two: the device mean of a grid that is not integer-valued is held to the rounding
bound derived from its size (occupancy_reference.mean_rel_bound), and the one cell of the special-value table whose
result is a zero of either sign is compared by value.

Which size reaches which loop trip:
  * compaction (k_occ_count / k_occ_fill, 4096 cells per workgroup): 257 * 4096 + 37 cells = 258 workgroups -- the second
    trip of the earlier-workgroups loop (b += 256) in workgroups 257.., and a last workgroup of 37 cells; 128^3 = 512
    workgroups (second trip in half of them); 4097 cells = a second workgroup of one cell; 5 cells = one partial workgroup
  * decayed maximum (k_occ_update_max / k_occ_update_apply, grid capped at 4096 x 256 threads): 4096 * 256 + 3 candidates
    -- three threads take a second trip; with and without an index list
  * mean (k_occ_mean_partial / k_occ_apply_mean, 256 x 256 threads): 5 and 65536 cells = one trip (most threads idle /
    none idle), 65537 = one thread's second trip, 3 * 65536 + 77 = three full trips and a ragged fourth, 128^3 = 32 trips,
    2 * 128^3 = 64 trips

Measured on the MI355X: worst mean error / derived bound 0.025 over the random grids (n = 2 * 128^3; 0.002 .. 0.012 at
the smaller sizes), 0.045 inside the replayed refreshes.

Each test fails for its own reason on a broken kernel.  Mutations tried (in a scratch copy), and what caught them:
  * k_occ_fill adds only the first trip of the earlier-workgroups sum (break instead of b += 256): the list check of
    test_occ_sample_compaction_and_draw at 258 and 512 workgroups (ragged_7pct, ragged_one_draw, full_level_*).  With this
    one the list's last entries are never written, and a refresh that draws from them indexes out of bounds: the list
    check is what stands between that bug and a memory fault
  * the same break in the loop that sums the total: the total word, same cases and ragged_last_37
  * the i < n_cells guard cut down to the full workgroups (the ragged tail is lost): every case with a ragged last
    workgroup (ragged_*, block_plus_1*, five_cells*)
  * one element too many in the strata of the second half of k_occ_draw: the index comparison of nearly every case,
    test_occ_sample_depends_on_seed_and_step, and every replayed refresh
  * > changed to >= in k_packbits: test_packbits_at_the_threshold (all three), test_packbits_with_the_mean_the_device_computed
  * | 0x80000000u removed in k_occ_update_max: test_occ_update_special_values, the second-trip test, update_mean with
    candidates, every refresh test and test_shadow_extra_state (its shadow never changes)
  * s >= 0.f changed to !(s < 0.f) (a NaN becomes a candidate): test_occ_update_special_values alone
  * k_occ_update_max without its strided trip: test_occ_update_second_trip_of_the_candidate_loop alone
  * k_occ_apply_mean without its strided trips: test_occ_update_mean_is_update_then_mean, the exact and the random mean
    from 65537 cells on, the fused half of the second-trip test, the G = 128 refresh
  * k_occ_mean_final started at b = 1: every mean test at every size (one-hot at cell 0 among them), the packbits chain,
    every refresh test
  * update_extra_state(): the step without "+ cas" -> the two-cascade refreshes; density_scale dropped in the steady
    state -> the density_scale case alone; iter_density not advanced, the bitfield packed without the mean -> every
    refresh test; the unfused mean taken over the first cascade only -> the two-cascade refreshes, sampled on the device
    and by torch
  * shadow_extra_state(): __exit__ that leaves the shadow in place, __enter__ that clones again on every entry ->
    test_shadow_extra_state
"""
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import occupancy_reference as R

pytestmark = pytest.mark.gpu

BLOCK = 4096                      # cells per workgroup of the compaction (csrc/occupancy.hip OCC_BLOCK_CELLS)
RAGGED = 257 * BLOCK + 37         # 258 workgroups, the last one of 37 cells


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _B():
    from src.latent_nerf.raymarching import backend as B
    return B


def _ps():
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    return _p, _stream


def _same_bits(a, b, what=""):
    a, b = R.bits(a), R.bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bool(bad.any()), "%s: %d of %d elements differ in bits, first at %s" % (
        what, int(bad.sum()), bad.numel(), torch.nonzero(bad)[0].tolist())


# ================================================================================================ 1. compaction and draw
def _sample(dev, level, cas, bound, n_rand, G=128, seed=0x5EED, step=37):
    """lnerf_occ_sample on a flat level -> (indices, points, per-workgroup counts, total, the whole list area)."""
    B = _B()
    _p, _stream = _ps()
    n_cells = level.numel()
    n_blocks = -(-n_cells // BLOCK)
    nb = B.get_lib().lnerf_occ_sample_scratch_bytes(n_cells)
    assert nb == 4 * (n_blocks + 1 + n_cells)
    scratch = torch.full((nb // 4,), -7, dtype=torch.int32, device=dev)          # poisoned: untouched words stay -7
    idx = torch.full((2 * n_rand,), -1, dtype=torch.int32, device=dev)
    xyz = torch.full((2 * n_rand, 3), float("nan"), device=dev)
    lv = level.to(dev)
    B.call("lnerf_occ_sample", _p(lv), n_cells, cas, G, bound, n_rand, seed, step, _p(scratch), _p(idx), _p(xyz), _stream())
    torch.cuda.synchronize()
    s = scratch.cpu()
    return idx.cpu().long(), xyz.cpu(), s[:n_blocks], int(s[n_blocks]), s[n_blocks + 1:]


def _random_level(n_cells, seed, frac=0.07):
    g = torch.Generator().manual_seed(seed)
    level = torch.where(torch.rand(n_cells, generator=g) < frac, torch.rand(n_cells, generator=g) + 0.01,
                        torch.zeros(n_cells))
    level[torch.randint(0, n_cells, (min(9, n_cells // 2),), generator=g)] = -1.0      # untrained cells: not occupied
    return level


def _only(n_cells, cells):
    level = torch.zeros(n_cells)
    level[cells] = 1.5
    return level


_SAMPLE_CASES = {
    # name: (level, cascade level, bound, n_rand)
    "ragged_7pct": lambda: (_random_level(RAGGED, 1), 0, 1.0, RAGGED // 4),
    "ragged_last_37": lambda: (_only(RAGGED, slice(RAGGED - 37, RAGGED)), 0, 1.0, RAGGED // 4),
    "ragged_cell_0": lambda: (_only(RAGGED, slice(0, 1)), 0, 1.0, RAGGED // 4),
    "ragged_empty": lambda: (torch.zeros(RAGGED), 0, 1.0, RAGGED // 4),
    "ragged_one_draw": lambda: (_random_level(RAGGED, 2), 0, 1.0, 1),
    "block_plus_1": lambda: (_random_level(BLOCK + 1, 3, 0.3), 0, 1.0, (BLOCK + 1) // 4),
    "block_plus_1_last_only": lambda: (_only(BLOCK + 1, slice(BLOCK, BLOCK + 1)), 0, 1.0, 64),
    "five_cells": lambda: (torch.tensor([0.0, 2.0, -1.0, 0.5, 0.0]), 0, 1.0, 1),
    "five_cells_more_draws_than_cells": lambda: (torch.tensor([0.0, 2.0, -1.0, 0.5, 0.0]), 0, 1.0, 13),
    "block_plus_1_more_draws_than_cells": lambda: (_random_level(BLOCK + 1, 4, 0.3), 0, 1.0, 2 * BLOCK + 5),
    "full_level_cascade_0": lambda: (_random_level(128 ** 3, 5), 0, 2.0, 128 ** 3 // 4),
    "full_level_cascade_1": lambda: (_random_level(128 ** 3, 6), 1, 2.0, 128 ** 3 // 4),
}


@pytest.mark.parametrize("case", list(_SAMPLE_CASES))
def test_occ_sample_compaction_and_draw(dev, case):
    """Indices and points of lnerf_occ_sample against O.occ_sample, bit for bit, on levels of 258 and 512 workgroups, a
    ragged last workgroup, single partial workgroups, one draw, and more draws than cells; and the compaction itself:
    the per-workgroup counts, the total word, the WHOLE list (the draw alone passes with a list that is wrong in entries
    nobody drew) and nothing written behind it."""
    level, cas, bound, n_rand = _SAMPLE_CASES[case]()
    n_cells = level.numel()
    idx, xyz, counts, total, area = _sample(dev, level, cas, bound, n_rand)
    occ = R.occupied_list(level)
    want_counts = [int((level[b:b + BLOCK] > 0).sum()) for b in range(0, n_cells, BLOCK)]
    assert counts.tolist() == want_counts
    assert total == occ.numel() == int((level > 0).sum())
    assert torch.equal(area[:total].long(), occ), "compacted list is not torch.nonzero(level > 0) in ascending order"
    assert bool((area[total:] == -7).all()), "words behind the list were written"
    ref_idx, ref_xyz = O.occ_sample(level, cas, 128, bound, n_rand, 0x5EED, 37)
    assert torch.equal(idx, ref_idx), (case, int((idx != ref_idx).sum()))
    _same_bits(xyz, ref_xyz, case + " points")
    # what the cases are there for, asserted on the oracle's own result so that a wrong oracle cannot hide behind a
    # kernel that is wrong the same way
    first, second = ref_idx[:n_rand], ref_idx[n_rand:]
    assert bool(((first >= 0) & (first < n_cells)).all())
    assert bool((first[1:] >= first[:-1]).all()) and bool((second[1:] >= second[:-1]).all())
    j = torch.arange(n_rand)
    lo, hi = j * n_cells // n_rand, (j + 1) * n_cells // n_rand      # stratum j (of less than one element: its one cell)
    assert bool((first >= lo).all()) and bool(((first < hi) | ((hi == lo) & (first == lo))).all())
    if total > 0:
        assert bool((level[second] > 0).all())                         # the second half sits in occupied cells
        assert len(set(second.tolist())) == min(total, n_rand)         # fewer occupied cells than draws: ALL of them
    else:                                                              # empty grid: the second half is uniform too
        assert bool((second >= lo).all()) and bool(((second < hi) | ((hi == lo) & (second == lo))).all())
        assert len(set(second.tolist())) == min(n_rand, n_cells)
    if case == "ragged_last_37":
        assert sorted(set(second.tolist())) == list(range(RAGGED - 37, RAGGED))
    if case == "ragged_cell_0":
        assert set(second.tolist()) == {0}
    if case == "block_plus_1_last_only":
        assert set(second.tolist()) == {BLOCK}
    if n_rand > n_cells:
        assert len(set(first.tolist())) == n_cells                     # strata of less than one element: every cell
    # points lie inside their cells
    b = min(2.0 ** cas, bound)
    coords = O.morton3d_invert(ref_idx).float()
    lo = ((coords / 128) * 2 - 1) * b
    hi = (((coords + 1) / 128) * 2 - 1) * b
    assert bool((xyz >= lo - 1e-6).all()) and bool((xyz <= hi + 1e-6).all())


def test_occ_sample_depends_on_seed_and_step(dev):
    """The step number and the seed reach the generator: the same level gives other cells and other jitter, each again
    the oracle's."""
    level = _random_level(BLOCK + 1, 8, 0.3)
    n_rand = 512
    seen = []
    for seed, step in ((0x5EED, 16 * 8), (0x5EED, 16 * 8 + 1), (0x5EED, 17 * 8), (0x0CC3, 16 * 8), (0xFFFFFFFF, 0x7FFFFFF9)):
        idx, xyz, *_ = _sample(dev, level, 0, 1.0, n_rand, seed=seed, step=step)
        ref_idx, ref_xyz = O.occ_sample(level, 0, 128, 1.0, n_rand, seed, step)
        assert torch.equal(idx, ref_idx)
        _same_bits(xyz, ref_xyz, "seed %x step %d" % (seed, step))
        seen.append(xyz)
    for a in range(len(seen)):
        for b in range(a + 1, len(seen)):
            assert not torch.equal(seen[a], seen[b])


# ================================================================================================ 2. decayed maximum
def _update(dev, grid, idx, sig, n_cells=None, fused=False):
    """lnerf_occ_update (or lnerf_occ_update_mean) on level 0 of grid [1, n_cells] -> (new grid on the host, mean or None);
    asserts the scratch words are all zero afterwards."""
    B = _B()
    _p, _stream = _ps()
    n_cells = grid.shape[1] if n_cells is None else n_cells
    gg, sig_d = grid.to(dev), sig.to(dev)
    idx_d = None if idx is None else idx.to(torch.int32).to(dev)
    cells = torch.zeros(n_cells, dtype=torch.int32, device=dev)
    mean = None
    if fused:
        mean, part = torch.full((1,), float("nan"), device=dev), torch.full((256,), float("nan"), device=dev)
        B.call("lnerf_occ_update_mean", _p(gg[0]), n_cells, _p(idx_d), sig.numel(), _p(sig_d), R.DECAY, _p(cells),
               _p(mean), _p(part), _stream())
    else:
        B.call("lnerf_occ_update", _p(gg[0]), _p(idx_d), sig.numel(), _p(sig_d), R.DECAY, _p(cells), _stream())
    torch.cuda.synchronize()
    assert int(cells.count_nonzero()) == 0, "scratch words are not all zero after the call"
    return gg.cpu(), (None if mean is None else mean.cpu())


def _mean(dev, grid_d):
    B = _B()
    _p, _stream = _ps()
    mean, part = torch.full((1,), float("nan"), device=dev), torch.full((256,), float("nan"), device=dev)
    B.call("lnerf_occ_mean", _p(grid_d), grid_d.numel(), _p(mean), _p(part), _stream())
    return mean.cpu()


def _candidates(n_cells, n, seed):
    g = torch.Generator().manual_seed(seed)
    grid = torch.rand(1, n_cells, generator=g) * 3
    grid[0, torch.randint(0, n_cells, (max(n_cells // 50, 1),), generator=g)] = -1.0
    grid[0, torch.randint(0, n_cells, (max(n_cells // 50, 1),), generator=g)] = 0.0
    idx = torch.randint(0, n_cells, (n,), generator=g)
    sig = torch.rand(n, generator=g) * 5
    if n:
        k = n // 20
        idx[:k] = idx[k:2 * k]                      # forced duplicates ...
        idx[n - k:] = idx[:k]                       # ... also between the first trip and the strided one
        sig[n - k:n - k + k // 2] = sig[:k // 2]     # exact ties between the duplicates of a cell
        sig[::7] = 0.0
        sig[3::11] = -1.0
    return grid, idx, sig


def test_occ_update_second_trip_of_the_candidate_loop(dev):
    """4096 * 256 + 3 candidates on a 128^3 level: the grid of both update kernels is capped at 4096 x 256 threads, so
    three threads take the strided trip -- with an index list (random cells, forced duplicates, also between the two
    trips) and without one (candidate i is cell i, on a level of that many cells)."""
    n = 4096 * 256 + 3
    grid, idx, sig = _candidates(128 ** 3, n, 11)
    idx[-3:] = torch.tensor([5, idx[0].item(), 128 ** 3 - 1])       # the strided trip's cells: fresh, shared, the last
    sig[-3:] = torch.tensor([9.0, 9.5, 0.0])
    ref = O.update_density_grid(grid, idx, 0, sig, R.DECAY)
    assert float(ref[0, 5]) == 9.0 or float(grid[0, 5]) < 0                 # (the strided trip decides these cells)
    out = [_update(dev, grid, idx[p], sig[p])[0] for p in (torch.arange(n), torch.randperm(n, generator=torch.Generator().manual_seed(1)))]
    _same_bits(out[0], ref, "update, second trip")
    _same_bits(out[1], ref, "update, second trip, shuffled")
    fused, _ = _update(dev, grid, idx, sig, fused=True)
    _same_bits(fused, ref, "update_mean, second trip")
    # no index list
    g = torch.Generator().manual_seed(12)
    grid2 = torch.rand(1, n, generator=g) * 3
    grid2[0, ::13] = -1.0
    grid2[0, n - 2] = 0.5
    sig2 = sig.clone()
    sig2[-3:] = torch.tensor([9.0, 0.0, 9.5])
    ref2 = O.update_density_grid(grid2, torch.arange(n), 0, sig2, R.DECAY)
    assert float(ref2[0, n - 2]) == float(np.float32(0.5) * np.float32(R.DECAY))
    _same_bits(_update(dev, grid2, None, sig2)[0], ref2, "update, no index list")
    _same_bits(_update(dev, grid2, None, sig2, fused=True)[0], ref2, "update_mean, no index list")


@pytest.mark.parametrize("fused", [False, True])
def test_occ_update_special_values(dev, fused):
    """+inf, NaN, -0.0, 0.0 and -1.0 candidates and equal maxima among the duplicates of a cell, on old cells of -1, 0,
    +inf and a positive value (occupancy_reference.SPECIAL_ROWS: every row listed twice, in both orders): the oracle's
    bits, the hand-written expectations, and the same bits from the reversed and from a shuffled list.  Bit 31 of the
    scratch word marks "touched", so a NaN (sign or no sign) must leave its cell alone and a -0.0 must decay it."""
    grid, idx, sig, cells, exp = R.special_value_case()
    ref = O.update_density_grid(grid, idx, 0, sig, R.DECAY)
    z = int(cells[R.SIGNED_ZERO])
    keep = torch.ones(grid.shape[1], dtype=torch.bool)
    keep[z] = False      # old 0 touched only by -0.0: the oracle's maximum may give -0.0, the kernel +0.0 -- by value
    hard = torch.ones(len(R.SPECIAL_ROWS), dtype=torch.bool)
    hard[R.SIGNED_ZERO] = False
    m = idx.numel()
    orders = (torch.arange(m), torch.arange(m - 1, -1, -1), torch.randperm(m, generator=torch.Generator().manual_seed(2)))
    for perm in orders:
        out, _ = _update(dev, grid, idx[perm], sig[perm], fused=fused)
        _same_bits(out[0, keep], ref[0, keep], "special values")
        _same_bits(out[0, cells][hard], exp[hard], "special values against the table")
        assert float(out[0, z]) == 0.0 and float(ref[0, z]) == 0.0
    # NaNs that carry a sign bit are no candidates either
    neg_nan = torch.tensor([0xFFC00000 - (1 << 32), 0xFF800001 - (1 << 32), 0x7F800001], dtype=torch.int32).view(torch.float32)
    g3 = torch.tensor([[2.0, 2.0, 2.0, 0.0]])
    out, _ = _update(dev, g3, torch.tensor([0, 1, 2]), neg_nan, fused=fused)
    _same_bits(out, g3, "NaN payloads")


@pytest.mark.parametrize("n_cells", [3 * 65536 + 77, 128 ** 3])
@pytest.mark.parametrize("n", ["none", "half"])
def test_occ_update_mean_is_update_then_mean(dev, n_cells, n):
    """lnerf_occ_update_mean = lnerf_occ_update followed by lnerf_occ_mean: grid bits (also the oracle's) and mean bits,
    where the streaming pass over the cells takes strided trips and a ragged one, with candidates and with none."""
    n = 0 if n == "none" else n_cells // 2
    grid, idx, sig = _candidates(n_cells, n, 21)
    ref = O.update_density_grid(grid, idx, 0, sig, R.DECAY) if n else grid
    a, _ = _update(dev, grid, idx, sig)
    mean_a = _mean(dev, a.to(dev))
    b, mean_b = _update(dev, grid, idx, sig, fused=True)
    _same_bits(a, ref, "update")
    _same_bits(b, ref, "update_mean")
    _same_bits(mean_b, mean_a, "mean of update_mean against update + mean")
    assert R.mean_ratio(mean_a.item(), ref) <= 1.0


# ================================================================================================ 3. the mean
def _both_means(dev, grid_d):
    """The mean of a device grid from lnerf_occ_mean and from lnerf_occ_update_mean without candidates."""
    B = _B()
    _p, _stream = _ps()
    n = grid_d.numel()
    before = grid_d.clone()
    cells = torch.zeros(n, dtype=torch.int32, device=grid_d.device)
    mean, part = torch.full((1,), float("nan"), device=grid_d.device), torch.full((256,), float("nan"), device=grid_d.device)
    B.call("lnerf_occ_update_mean", _p(grid_d), n, None, 0, None, R.DECAY, _p(cells), _p(mean), _p(part), _stream())
    m1 = _mean(dev, grid_d)
    assert torch.equal(grid_d.view(torch.int32), before.view(torch.int32))       # no candidates: the grid stays
    return m1, mean.cpu()


MEAN_SIZES = [5, 65536, 65537, 3 * 65536 + 77, 2 * 128 ** 3]


@pytest.mark.parametrize("n", MEAN_SIZES)
def test_occ_mean_exact_on_integer_grids(dev, n):
    """Values in {0, 1, 2, 3} and some -1 cells (counted as 0): every float32 partial sum is an integer below 2^24, exact
    in any order, so the mean is float32(S) / float32(n) bit for bit.  One-hot grids (a single 1.0 at the first cell, on
    both sides of the first stride, at both ends of the ragged tail and at the last cell) prove that every one of those
    cells is counted exactly once."""
    g = torch.Generator().manual_seed(n)
    grid = torch.randint(0, 4, (n,), generator=g).float()
    grid[torch.rand(n, generator=g) < 0.05] = -1.0
    want = torch.tensor([R.mean_exact(grid)])
    for m in _both_means(dev, grid.to(dev)):
        _same_bits(m, want, "integer grid of %d cells" % n)
    hot = torch.zeros(n, device=dev)
    one = torch.tensor([np.float32(1) / np.float32(n)])
    for c in R.one_hot_cells(n):
        hot[c] = 1.0
        for m in _both_means(dev, hot):
            _same_bits(m, one, "one-hot at cell %d of %d" % (c, n))
        hot[c] = 0.0
    # a grid of -1 cells alone has mean 0
    for m in _both_means(dev, torch.full((n,), -1.0, device=dev)):
        _same_bits(m, torch.zeros(1), "all cells -1")


@pytest.mark.parametrize("n", MEAN_SIZES)
def test_occ_mean_random_grid_within_the_derived_bound(dev, n):
    """A random grid against its float64 mean: all terms are non-negative, so the float32 result is within a relative
    K u / (1 - K u) of it, u = 2^-24, K = ceil(n / 65536) + 6 + 3 + 256 + 1 roundings on the longest path (the thread's
    chain, wave_sum's six steps, the four waves, the serial loop over the partials, the division).  Three calls give
    identical bits, and both entry points the same ones."""
    g = torch.Generator().manual_seed(100 + n)
    grid = torch.rand(n, generator=g) * 5
    grid[torch.rand(n, generator=g) < 0.1] = -1.0
    grid_d = grid.to(dev)
    means = []
    for _ in range(3):
        means.extend(_both_means(dev, grid_d))
    for m in means[1:]:
        _same_bits(m, means[0], "repeated mean")
    ratio = R.mean_ratio(means[0].item(), grid)
    print("occ mean, n = %d: K = %d, error / bound = %.4f" % (n, R.mean_roundings(n), ratio))
    assert ratio <= 1.0, (n, ratio)
    # (the float32 emulation of the same order gives the same bits: the order is the documented one)
    if n <= 3 * 65536 + 77:
        _same_bits(means[0], torch.tensor([R.mean_emulate_f32(grid)]), "mean against the emulated order")


# ================================================================================================ 4. packbits
def _packbits(dev, grid_d, thresh, mean_dev=None):
    from src.latent_nerf.raymarching import raymarching as rm
    bits = torch.full((grid_d.numel() // 8,), 0xAA, dtype=torch.uint8, device=dev)
    rm.packbits(grid_d, thresh, bits, mean_dev)
    return bits.cpu()


def _edge_grid(th, seed=0):
    """Cells around th: exactly th (strict comparison: off), one step above and below, -1, +inf, both zeros, randoms."""
    th32 = np.float32(th)
    up, dn = float(np.nextafter(th32, np.float32(np.inf))), float(np.nextafter(th32, np.float32(-np.inf)))
    if th32 == 0:                                   # (no denormals: the smallest normal numbers on either side of 0)
        up, dn = float(np.finfo(np.float32).tiny), -float(np.finfo(np.float32).tiny)
    g = torch.Generator().manual_seed(seed)
    n = 8 * 517
    grid = torch.rand(n, generator=g) * 2 * max(abs(float(th32)), 0.5)
    special = torch.tensor([float(th32), up, dn, -1.0, float("inf"), 0.0, -0.0, float(th32)])
    for r in range(8):                              # every value at every bit position of a byte
        grid[64 * r:64 * r + 64].view(8, 8)[:] = torch.roll(special, r)[None, :]
    grid[n - 8:] = float(th32)                      # a last byte of cells all equal to the threshold
    grid[n - 16:n - 8] = up
    return grid, float(th32), up, dn


@pytest.mark.parametrize("th", [0.37, 0.0, 10.0])
def test_packbits_at_the_threshold(dev, th):
    """A cell exactly equal to the threshold is off (the comparison is strict), its float32 neighbours are on and off;
    -1 cells are off under a threshold of 0; +inf cells are on.  Then min(thresh, *mean_dev) with a device mean below,
    equal to and above thresh."""
    grid, th, up, dn = _edge_grid(th)
    grid_d = grid.to(dev)
    got = _packbits(dev, grid_d, th)
    assert torch.equal(got, O.packbits(grid, th))
    assert got[-1].item() == 0 and got[-2].item() == 255
    on = ((got.long()[:, None] >> torch.arange(8)[None, :]) & 1).reshape(-1).bool()
    assert not bool(on[grid == th].any()) and bool(on[grid == up].all()) and not bool(on[grid == dn].any())
    assert not bool(on[grid == -1.0].any()) and bool(on[torch.isinf(grid)].all())
    if th == 0.0:
        assert not bool(on[grid == 0.0].any())                    # +0.0 and -0.0 alike
    for mean, eff in ((dn, dn), (th, th), (up, th)):
        mean_d = torch.tensor([mean], device=dev)
        for thresh in (th, up):                                   # the mean below / equal / above either
            want = O.packbits(grid, min(thresh, mean))
            assert torch.equal(_packbits(dev, grid_d, thresh, mean_d), want), (mean, thresh)
        assert torch.equal(_packbits(dev, grid_d, th, mean_d), O.packbits(grid, eff))


def test_packbits_with_the_mean_the_device_computed(dev):
    """mean -> threshold -> bits on the device: lnerf_occ_mean writes mean_dev, lnerf_packbits reads it.  The grid is
    integer-valued, so the mean is known exactly, and holds cells EQUAL to that mean: they are off."""
    n = 8 * 4096
    g = torch.Generator().manual_seed(5)
    grid = torch.randint(0, 5, (n,), generator=g).float() * 2          # even integers, mean near 4
    grid[:7] = -1.0
    grid[8] = 0.0                                                      # cell 8 takes what the sum lacks to 4 n
    need, k = 4 * n - int(grid.clamp(min=0).sum()), 16
    while need < 0:
        need, grid[k], k = need + int(grid[k]), 0.0, k + 1
    grid[8] = float(need)                                              # the sum is 4 n: the mean is exactly 4.0
    assert R.mean_exact(grid) == np.float32(4.0) and int((grid == 4.0).sum()) > 1000
    grid_d = grid.to(dev)
    mean_d = _mean(dev, grid_d).to(dev)
    assert float(mean_d) == 4.0
    for thresh, eff in ((10.0, 4.0), (4.0, 4.0), (2.0, 2.0)):
        got = _packbits(dev, grid_d, thresh, mean_d)
        assert torch.equal(got, O.packbits(grid, eff)), thresh
    on = ((_packbits(dev, grid_d, 10.0, mean_d).long()[:, None] >> torch.arange(8)[None, :]) & 1).reshape(-1).bool()
    assert not bool(on[grid == 4.0].any()) and bool(on[grid > 4.0].all())


# ================================================================================================ 5. update_extra_state()
def _make_net(dev, G, bound=1.0, seed=9, log2_T=12, **cfg_kw):
    """A renderer as tests/test_gpu_render.py::_make builds it, with a near-zero table: the density blob dominates."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(seed)
    cfg = RenderConfig(grid_size=G, train_h=16, train_w=16, bound=bound, **cfg_kw)
    net = NeRFNetwork(cfg, base_resolution=16, log2_hashmap_size=log2_T)
    net.encoder.embeddings.data.normal_(0, 1e-4)
    return net.to(dev)


def _sphere(x):
    return (x.norm(dim=-1) < 0.5).float() * 10.0


def _steady(net, how, seed=3):
    """Bring a renderer to the steady state of its refresh: 16 refreshes from an empty grid, or the analytic sphere with
    iter_density = 16 (and some untrained cells)."""
    net.reset_extra_state()
    net.occupancy_generator(seed=seed)
    if how == "sixteen":
        for _ in range(16):
            net.update_extra_state()
    else:
        net.seed_density_grid(_sphere)
        net.density_grid[:, 3::97] = -1.0
        net.iter_density = 16
    assert net.iter_density == 16


def _state(net):
    return (net.density_grid.cpu().clone(), net.density_bitfield.cpu().clone(), net.mean_density_dev.cpu().clone())


def _check_mean_and_bits(net, dev, what=""):
    """The mean is the device mean of the resulting grid (bits) and within the derived bound of its float64 mean; the
    bitfield is O.packbits of the grid at min(that mean, density_thresh)."""
    grid, bits, mean = _state(net)
    _same_bits(mean, _mean(dev, net.density_grid), what + " mean against lnerf_occ_mean of the grid")
    ratio = R.mean_ratio(mean.item(), grid)
    assert ratio <= 1.0, (what, ratio)
    assert torch.equal(bits, O.packbits(grid.reshape(-1), min(float(mean), float(net.density_thresh)))), what
    return ratio


def _replay_refresh(net, dev, before, it):
    """One steady-state refresh from its pieces -> (grid, (indices, points) of the last cascade)."""
    G3 = net.grid_size ** 3
    n_rand = G3 // 4
    ref, last = before.clone(), None
    for cas in range(net.cascade):
        idx, xyz = O.occ_sample(before[cas], cas, net.grid_size, net.bound, n_rand, net._occ_seed, it * 8 + cas)
        with torch.no_grad():
            sig, _ = net.field(xyz.to(dev).contiguous(), 2 * n_rand)     # as the refresh calls it
            sig = sig.contiguous() if net.density_scale == 1.0 else (sig * net.density_scale).contiguous()
        ref = O.update_density_grid(ref, idx, cas, sig.cpu(), 0.95)
        last = (idx, xyz)
    return ref, last


_REFRESH_CASES = {
    # name: (G, bound, how the steady state is reached, density_thresh, density_scale, refreshes)
    "g32_fused_after_16_refreshes": (32, 1.0, "sixteen", 10.0, 1.0, 3),
    "g32_fused_sphere": (32, 1.0, "sphere", 10.0, 1.0, 3),
    "g32_two_cascades": (32, 2.0, "sphere", 0.05, 1.0, 3),
    "g32_two_cascades_density_scale": (32, 2.0, "sphere", 10.0, 0.5, 3),
    "g128_fused_one_refresh": (128, 1.0, "sphere", 10.0, 1.0, 1),
}


@pytest.mark.parametrize("case", list(_REFRESH_CASES))
def test_steady_state_refresh_is_the_chain_of_its_pieces(dev, case):
    """update_extra_state() with iter_density >= 16 (lnerf_occ_sample -> field -> lnerf_occ_update_mean for one cascade;
    lnerf_occ_update per cascade, then lnerf_occ_mean over all of them, for two) replayed from the grid before it:
    O.occ_sample at step iter_density * 8 + cascade gives the workspace's cells and points, the field on those points and
    O.update_density_grid the grid, the mean and the bitfield follow from that grid.  A renderer in eval() mode goes
    through the same states."""
    G, bound, how, thresh, scale, refreshes = _REFRESH_CASES[case]
    net, twin = _make_net(dev, G, bound), _make_net(dev, G, bound)
    assert net.cascade == (1 if bound == 1.0 else 2)
    net.train()
    twin.eval()
    for m in (net, twin):
        m.density_thresh, m.density_scale = thresh, scale
        _steady(m, how)
    for a, b in zip(_state(net), _state(twin)):
        _same_bits(a.float(), b.float(), case + ": the two renderers start alike")
    worst = 0.0
    for r in range(refreshes):
        it = net.iter_density
        before = net.density_grid.cpu().clone()
        net.update_extra_state()
        twin.update_extra_state()
        assert net.iter_density == it + 1 == twin.iter_density
        ref, (idx, xyz) = _replay_refresh(net, dev, before, it)
        _, ws_idx, ws_xyz = net._occ_sample_ws
        assert torch.equal(ws_idx.cpu().long(), idx), case + ": cells of the last cascade"
        _same_bits(ws_xyz, xyz, case + ": points of the last cascade")
        _same_bits(net.density_grid, ref, "%s: grid after refresh %d" % (case, it))
        assert not torch.equal(ref, before)                               # (the refresh changed something)
        assert torch.equal(ref < 0, before < 0)                           # untrained cells stay untrained
        worst = max(worst, _check_mean_and_bits(net, dev, "%s refresh %d" % (case, it)))
        assert int(net._occ_cells.count_nonzero()) == 0
        for a, b in zip(_state(net), _state(twin)):
            _same_bits(a.float(), b.float(), case + ": eval() against train()")
    print("%s: worst mean error / bound = %.4f, threshold = min(%.4f, %.4f)"
          % (case, worst, float(net.mean_density_dev), thresh))
    if thresh < 1.0:
        assert float(net.mean_density_dev) > thresh                       # (this case runs the thresh side of the min)
    else:
        assert float(net.mean_density_dev) < thresh


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_steady_state_refresh_sampled_by_torch_keeps_its_invariants(dev, bound):
    """occ_device_sampling = False draws with torch.randint and cannot be replayed bit for bit: after each of three
    steady-state refreshes no -1 cell has changed, no cell is below its decayed old value, the mean and the bitfield
    are those of the resulting grid, and the update's scratch is zero."""
    net = _make_net(dev, 32, bound, occ_device_sampling=False)
    net.train()
    _steady(net, "sphere")
    for _ in range(3):
        it = net.iter_density
        before = net.density_grid.cpu().clone()
        net.update_extra_state()
        assert net.iter_density == it + 1
        after = net.density_grid.cpu()
        un = before < 0
        assert int(un.sum()) > 0 and torch.equal(R.bits(after[un]), R.bits(before[un]))
        assert bool((after[~un] >= before[~un] * 0.95).all())
        assert bool((after[~un] >= 0).all()) and not torch.equal(after, before)
        _check_mean_and_bits(net, dev, "torch-sampled refresh %d" % it)
        assert int(net._occ_cells.count_nonzero()) == 0
    assert net._occ_sample_ws is None                                    # (the device sampler was not used)


# ================================================================================================ 6. shadow_extra_state()
def _march_of(net, dev, HW=16):
    f = HW / (2 * math.tan(math.radians(55) / 2))
    c2w = O.pose_from_angles(math.radians(60.0), math.radians(20.0), 1.25)
    ro, rd = O.get_rays(c2w, f, f, HW / 2, HW / 2, HW, HW)
    with torch.no_grad():
        out = net.render(ro.to(dev), rd.to(dev), bg_color=None, perturb=False)
    M = int(out["counter"][0])
    # (the buffers belong to the march and are written again by the next one: copies; word 3 of the counter is the
    # running peak the sample budget reads and clears, not part of the march's result)
    return out["rays"].cpu().clone(), out["counter"][:3].cpu().clone(), out["xyzs"][:M].cpu().clone(), M


def test_shadow_extra_state(dev):
    """Inside shadow_extra_state() a refresh does all of its work on a shadow copy: the real grid, bitfield and mean keep
    their bits and are the same tensor objects afterwards, also when the body raises; on first entry the shadow holds
    what the same refresh gives on the real state of an identically seeded renderer; a training march afterwards is the
    one from before."""
    names = ("density_grid", "density_bitfield", "mean_density_dev")
    net, twin = _make_net(dev, 32), _make_net(dev, 32)
    for m in (net, twin):
        m.train()
        _steady(m, "sphere", seed=5)
    rays0, counter0, xyzs0, M0 = _march_of(net, dev)
    assert M0 > 0
    real = [getattr(net, n) for n in names]
    saved = [t.cpu().clone() for t in real]
    with net.shadow_extra_state() as inside:
        assert inside is net
        assert all(getattr(net, n) is not t for n, t in zip(names, real))
        net.update_extra_state()
        shadow = [getattr(net, n) for n in names]
    twin.update_extra_state()                                            # the same refresh, for real
    assert net.iter_density == twin.iter_density == 17
    for n, t, s, sh in zip(names, real, saved, shadow):
        assert getattr(net, n) is t and net._buffers[n] is t, n
        _same_bits(t.float(), s.float(), "real " + n + " after the context")
        _same_bits(sh.float(), getattr(twin, n).float(), "shadow " + n + " against a real refresh")
    assert not torch.equal(shadow[0].cpu(), saved[0])                    # (the refresh did change the shadow)
    assert set(net.state_dict()) >= set(names)
    # the march after the context is the march before it
    rays1, counter1, xyzs1, M1 = _march_of(net, dev)
    assert M1 == M0 and torch.equal(rays1, rays0) and torch.equal(counter1, counter0)
    _same_bits(xyzs1, xyzs0, "samples of the march after the context")
    # ... while the twin's scene did change
    assert not torch.equal(twin.density_bitfield.cpu(), saved[1])
    # a body that raises: the real state is back, untouched; the shadow is kept and goes on from where it was
    with pytest.raises(RuntimeError, match="inside"):
        with net.shadow_extra_state():
            assert net.density_grid is shadow[0]
            net.update_extra_state()
            raise RuntimeError("inside")
    twin.update_extra_state()
    for n, t, s, sh in zip(names, real, saved, shadow):
        assert getattr(net, n) is t, n
        _same_bits(t.float(), s.float(), "real " + n + " after a raising body")
        _same_bits(sh.float(), getattr(twin, n).float(), "shadow " + n + " after its second refresh")
