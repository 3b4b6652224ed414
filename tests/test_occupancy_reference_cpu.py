"""The restatements of tests/occupancy_reference.py against brute-force Python loops on tiny sizes, and the oracle's
occupancy functions on the special values the GPU test feeds them -- without a GPU.  tests/test_gpu_occupancy.py holds
the kernels to the same references."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import occupancy_reference as R


def test_special_value_table_is_what_the_rule_gives():
    """The hand-written expectations, the plain loop and the oracle agree on every row, bit for bit; the one signed-zero
    cell by value.  Every row is listed at least twice, in both orders."""
    grid, idx, sig, cells, exp = R.special_value_case()
    assert len(set(cells.tolist())) == len(R.SPECIAL_ROWS)
    for c, (_, cands, _) in zip(cells.tolist(), R.SPECIAL_ROWS):
        mine = sig[idx == c]
        assert mine.numel() == 2 * len(cands) >= 4
        assert R.bits(mine).tolist() == R.bits(torch.tensor(tuple(cands) + tuple(reversed(cands)))).tolist()
    olds = {r[0] for r in R.SPECIAL_ROWS}
    assert olds == {-1.0, 0.0, R.INF, 2.0}
    flat = [s for r in R.SPECIAL_ROWS for s in r[1]]
    assert any(s != s for s in flat) and R.INF in flat and -1.0 in flat
    assert any(s == 0 and np.signbit(s) for s in flat) and any(s == 0 and not np.signbit(s) for s in flat)
    ref = O.update_density_grid(grid, idx, 0, sig, R.DECAY)
    loop = R.update_loop(grid[0], idx, sig)
    hard = torch.ones(len(R.SPECIAL_ROWS), dtype=torch.bool)
    hard[R.SIGNED_ZERO] = False
    assert torch.equal(R.bits(ref[0, cells])[hard], R.bits(exp)[hard])
    assert torch.equal(R.bits(loop[cells])[hard], R.bits(exp)[hard])
    z = cells[R.SIGNED_ZERO]
    assert float(ref[0, z]) == 0.0 and float(loop[z]) == 0.0
    # every cell outside the table is untouched
    rest = torch.ones(grid.shape[1], dtype=torch.bool)
    rest[cells] = False
    assert torch.equal(R.bits(ref[0, rest]), R.bits(grid[0, rest]))
    assert torch.equal(R.bits(loop[rest]), R.bits(grid[0, rest]))
    # a reversed and a shuffled list give the same bits (again but for the signed zero)
    for perm in (torch.arange(idx.numel() - 1, -1, -1), torch.randperm(idx.numel(), generator=torch.Generator().manual_seed(1))):
        again = O.update_density_grid(grid, idx[perm], 0, sig[perm], R.DECAY)
        keep = torch.ones(grid.shape[1], dtype=torch.bool)
        keep[z] = False
        assert torch.equal(R.bits(again[0, keep]), R.bits(ref[0, keep]))


def test_update_oracle_is_the_loop_on_random_lists():
    g = torch.Generator().manual_seed(3)
    for n_cells, n in ((7, 40), (64, 200), (300, 90)):
        grid = torch.rand(1, n_cells, generator=g) * 3
        grid[0, ::5] = -1.0
        grid[0, 1::7] = 0.0
        idx = torch.randint(0, n_cells, (n,), generator=g)
        sig = torch.rand(n, generator=g) * 4
        sig[::3] = 0.0
        sig[1::4] = -1.0
        sig[2::9] = sig[0]                         # ties
        ref = O.update_density_grid(grid, idx, 0, sig, R.DECAY)
        assert torch.equal(R.bits(ref[0]), R.bits(R.update_loop(grid[0], idx, sig)))


@pytest.mark.parametrize("n", [5, 777, 65536, 65537, 3 * 65536 + 77])
def test_mean_exact_and_emulation(n):
    """mean_exact is the exactly rounded quotient of the integer sum; the float32 emulation of the device's order gives
    the same bits on integer grids and on every one-hot grid, and stays inside the derived bound on a random grid."""
    g = torch.Generator().manual_seed(n)
    grid = torch.randint(0, 4, (n,), generator=g).float()
    grid[torch.rand(n, generator=g) < 0.1] = -1.0
    S = 0
    for v in grid.tolist():                        # the brute-force loop
        S += int(v) if v > 0 else 0
    want = R.mean_exact(grid)                      # must be the float32 nearest to the rational S / n
    q = Fraction(S, n)
    for other in (np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(1))):
        assert abs(Fraction(float(want)) - q) <= abs(Fraction(float(other)) - q)
    assert want == np.float32(S) / np.float32(n)
    assert R.mean_emulate_f32(grid) == want
    for c in R.one_hot_cells(n):
        hot = torch.zeros(n)
        hot[c] = 1.0
        assert R.mean_emulate_f32(hot) == np.float32(1) / np.float32(n) == R.mean_exact(hot)
    rnd = torch.rand(n, generator=g) * 5
    rnd[::11] = -1.0
    assert abs(R.mean_f64(rnd) - sum(max(v, 0.0) for v in rnd.double().tolist()) / n) <= 1e-12 * R.mean_f64(rnd)
    ratio = R.mean_ratio(R.mean_emulate_f32(rnd), rnd)
    print("n = %d: emulated mean error / bound = %.4f" % (n, ratio))
    assert ratio <= 1.0


def test_mean_bound_counts_the_roundings():
    assert R.mean_roundings(5) == 1 + 6 + 3 + 256 + 1
    assert R.mean_roundings(65536) == 1 + 266 and R.mean_roundings(65537) == 2 + 266
    assert R.mean_roundings(2 * 128 ** 3) == 64 + 266
    K = R.mean_roundings(3 * 65536 + 77)
    assert K == 4 + 266 and R.mean_rel_bound(3 * 65536 + 77) == K * 2.0 ** -24 / (1 - K * 2.0 ** -24)
    # the bound covers (1 + u)^K - 1 and is not far above it
    for n in (5, 2 * 128 ** 3):
        K = R.mean_roundings(n)
        worst = float((Fraction(1) + Fraction(1, 1 << 24)) ** K - 1)
        assert worst <= R.mean_rel_bound(n) <= 1.001 * worst


def test_one_hot_cells_and_wave_sum_order():
    assert R.one_hot_cells(5) == [0, 4]
    assert R.one_hot_cells(65536) == [0, 65535]
    assert R.one_hot_cells(65537) == [0, 65535, 65536]
    n = 3 * 65536 + 77
    assert R.one_hot_cells(n) == [0, 65535, 65536, 3 * 65536 - 1, 3 * 65536, n - 1]
    # the wave sum on integers is the plain sum, and every lane is counted once
    v = np.arange(64, dtype=np.float32)[None]
    assert float(R._wave_sum_f32(v)[0]) == 63 * 64 / 2
    for lane in range(64):
        e = np.zeros((1, 64), dtype=np.float32)
        e[0, lane] = 1
        assert float(R._wave_sum_f32(e)[0]) == 1.0


def test_occupied_list_and_packbits_edges():
    """occupied_list against a loop; O.packbits against a loop at the threshold, one step on either side of it, -1 under a
    threshold of 0, and +inf."""
    level = torch.tensor([0.0, 1.0, -1.0, R.NAN, 1e-30, -0.0, R.INF, 0.5])
    assert R.occupied_list(level).tolist() == [i for i, v in enumerate(level.tolist()) if v > 0] == [1, 4, 6, 7]
    th = float(np.float32(0.37))
    up, dn = float(np.nextafter(np.float32(th), np.float32(1))), float(np.nextafter(np.float32(th), np.float32(0)))
    grid = torch.tensor([th, up, dn, -1.0, R.INF, 0.0, -0.0, th, 1.0, th, th, dn, up, up, dn, 0.0])
    for t in (th, 0.0):
        want = [sum((1 << k) for k in range(8) if grid[8 * b + k].item() > t) for b in range(2)]
        assert O.packbits(grid, t).tolist() == want
    assert O.packbits(grid, th).tolist() == [0b00010010, 0b00110001]
    assert O.packbits(grid, 0.0)[0].item() == 0b10010111       # -1, 0.0 and -0.0 are off under a threshold of 0
