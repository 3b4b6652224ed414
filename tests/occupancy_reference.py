"""Restatements for the occupancy-refresh tests (tests/test_gpu_occupancy.py), beyond oracle/nerf_oracle.py: the exact
mean of an integer-valued grid, the derived rounding bound of the device mean, a float32 emulation of the device's
summation order (to hold the bound to account without a GPU), the ascending list of occupied cells, and the hand-written
table of special values of the decayed-max update with its expected results.  tests/test_occupancy_reference_cpu.py
checks each of them against brute-force Python loops."""
import math

import numpy as np
import torch

MEAN_BLOCKS = 256              # workgroups of the mean pass (csrc/occupancy.hip OCC_MEAN_BLOCKS), 256 threads each
MEAN_STRIDE = MEAN_BLOCKS * 256
U = 2.0 ** -24                 # unit roundoff of float32
DECAY = 0.95


def bits(t: torch.Tensor) -> torch.Tensor:
    """float32 tensor -> its bit patterns (int32), on the host."""
    return t.detach().cpu().contiguous().view(torch.int32)


def occupied_list(level: torch.Tensor) -> torch.Tensor:
    """Ascending indices of the cells with level > 0 (-1 = untrained, 0 and NaN are not occupied)."""
    return torch.nonzero(level.reshape(-1) > 0).squeeze(-1)


# ------------------------------------------------------------------------------------------------ mean
def mean_exact(grid: torch.Tensor) -> np.float32:
    """Mean of max(grid, 0) of a grid whose values are integers (and -1) with S = sum < 2^24: every float32 partial sum
    is then an integer below 2^24, exact in any order, and the device's one division gives float32(S) / float32(n)."""
    g = grid.reshape(-1).to(torch.float64).clamp(min=0)
    assert bool((g == g.round()).all()), "mean_exact needs an integer-valued grid"
    S = int(g.sum().item())
    assert S < (1 << 24) and grid.numel() <= (1 << 24)
    return np.float32(S) / np.float32(grid.numel())


def mean_f64(grid: torch.Tensor) -> float:
    return float(grid.reshape(-1).to(torch.float64).clamp(min=0).mean())


def mean_roundings(n: int) -> int:
    """Roundings on the longest path of the device mean of n cells: the per-thread chain over the strided slice
    (ceil(n / 65536) additions), wave_sum's six steps, the four waves (3), the serial loop over the 256 partials, and the
    division."""
    return -(-n // MEAN_STRIDE) + 6 + 3 + MEAN_BLOCKS + 1


def mean_rel_bound(n: int) -> float:
    """All terms are non-negative, so K roundings move the result by at most a relative (1 + u)^K - 1 <= K u / (1 - K u)
    (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1)."""
    K = mean_roundings(n)
    return K * U / (1.0 - K * U)


def _wave_sum_f32(v: np.ndarray) -> np.ndarray:
    """v [..., 64] float32 -> what lane 63 of csrc/common.h wave_inclusive_sum holds: a shifted-add scan inside each row
    of 16 lanes (shifts 1, 2, 4, 8), row 0 into row 1 and row 2 into row 3, then lane 31 into lane 63."""
    v = v.astype(np.float32).reshape(v.shape[:-1] + (4, 16)).copy()
    for sh in (1, 2, 4, 8):
        add = np.zeros_like(v)
        add[..., sh:] = v[..., :-sh]
        v = (v + add).astype(np.float32)
    row = v[..., 15]
    lo = (row[..., 1] + row[..., 0]).astype(np.float32)
    hi = (row[..., 3] + row[..., 2]).astype(np.float32)
    return (hi + lo).astype(np.float32)


def mean_emulate_f32(grid: torch.Tensor) -> np.float32:
    """The device mean in numpy float32, operation by operation in the kernels' order (k_occ_mean_partial /
    k_occ_apply_mean, then k_occ_mean_final)."""
    g = np.maximum(grid.reshape(-1).numpy().astype(np.float32), np.float32(0))
    n = g.size
    trips = -(-n // MEAN_STRIDE)
    pad = np.zeros(trips * MEAN_STRIDE, dtype=np.float32)
    pad[:n] = g
    pad = pad.reshape(trips, MEAN_BLOCKS, 4, 64)            # cell = trip * 65536 + block * 256 + wave * 64 + lane
    s = np.zeros((MEAN_BLOCKS, 4, 64), dtype=np.float32)
    for k in range(trips):
        s = (s + pad[k]).astype(np.float32)
    w = _wave_sum_f32(s)                                     # [blocks, 4]
    part = (((w[:, 0] + w[:, 1]).astype(np.float32) + w[:, 2]).astype(np.float32) + w[:, 3]).astype(np.float32)
    tot = np.float32(0)
    for b in range(MEAN_BLOCKS):
        tot = np.float32(tot + part[b])
    return np.float32(tot / np.float32(n))


def mean_ratio(mean_f32, grid: torch.Tensor) -> float:
    """|mean - float64 mean| / (bound x float64 mean): <= 1 inside the derived bound (0 for an all-zero grid)."""
    ref = mean_f64(grid)
    err = abs(float(mean_f32) - ref)
    if ref == 0.0:
        return 0.0 if err == 0.0 else math.inf
    return err / (mean_rel_bound(grid.numel()) * ref)


def one_hot_cells(n: int):
    """Cells that hold the single 1.0 of the one-hot grids: the first, both sides of the first stride of the mean pass,
    the last, and both ends of the ragged tail behind the last full stride."""
    tail = (n // MEAN_STRIDE) * MEAN_STRIDE
    cells = {0, n - 1}
    for c in (MEAN_STRIDE - 1, MEAN_STRIDE, tail - 1, tail):
        if 0 <= c < n:
            cells.add(c)
    return sorted(cells)


# ------------------------------------------------------------------------------------------------ special values
INF, NAN = float("inf"), float("nan")

# (old value, candidates in list order, expected new value); None = compared by VALUE (see SIGNED_ZERO below)
# expected values are written by hand from the rule: candidates >= 0 (NaN and negatives are none; -0.0 is one, of value
# 0) mark the cell; a marked cell with old >= 0 becomes max(old * decay, largest candidate); everything else stays.
_D = float(np.float32(2.0) * np.float32(DECAY))      # 2.0 decayed once, in float32
SPECIAL_ROWS = [
    # old -1 (untrained): never changes
    (-1.0, (INF, 3.0), -1.0), (-1.0, (3.0, INF), -1.0), (-1.0, (NAN, -0.0), -1.0), (-1.0, (-0.0, NAN), -1.0),
    (-1.0, (0.0, -1.0), -1.0), (-1.0, (-1.0, 0.0), -1.0),
    # old 0
    (0.0, (INF, 5.0), INF), (0.0, (5.0, INF), INF), (0.0, (NAN, NAN), 0.0), (0.0, (0.0, 0.0), 0.0),
    (0.0, (-1.0, NAN), 0.0), (0.0, (NAN, -1.0), 0.0), (0.0, (-0.0, 5.0), 5.0), (0.0, (5.0, -0.0), 5.0),
    (0.0, (4.0, 4.0, 1.0), 4.0), (0.0, (1.0, 4.0, 4.0), 4.0), (0.0, (NAN, 3.0), 3.0), (0.0, (3.0, NAN), 3.0),
    # old +inf: decays to +inf when touched, untouched otherwise
    (INF, (1.0, 2.0), INF), (INF, (2.0, 1.0), INF), (INF, (NAN, NAN), INF), (INF, (-1.0, -1.0), INF),
    (INF, (INF, -0.0), INF), (INF, (-0.0, INF), INF),
    # old positive
    (2.0, (INF, 1.0), INF), (2.0, (1.0, INF), INF),
    (2.0, (NAN, NAN), 2.0),                          # a NaN candidate leaves the cell untouched: no decay
    (2.0, (NAN, 1.0), _D), (2.0, (1.0, NAN), _D),    # the NaN is no candidate, the 1.0 is: decays
    (2.0, (NAN, 7.0), 7.0), (2.0, (7.0, NAN), 7.0),
    (2.0, (-0.0, -0.0), _D),                         # touched only by -0.0: decays
    (2.0, (-0.0, 0.0), _D), (2.0, (0.0, -0.0), _D), (2.0, (0.0, 0.0), _D),
    (2.0, (-1.0, -1.0), 2.0),                        # negative candidates never touch
    (2.0, (-1.0, 0.0), _D), (2.0, (0.0, -1.0), _D),
    (2.0, (6.0, 6.0, 3.0), 6.0), (2.0, (3.0, 6.0, 6.0), 6.0), (2.0, (6.0, 3.0, 6.0), 6.0),   # two equal maxima
    (2.0, (1.5, 1.0), _D), (2.0, (1.0, 1.5), _D),    # candidates below the decayed old value
    # the one signed-zero cell: old 0, touched only by -0.0.  max(0 * decay, -0.0) is +0.0 or -0.0 depending on how a
    # maximum orders the two zeros; the kernels give +0.0
    (0.0, (-0.0, -0.0), None),
]
SIGNED_ZERO = len(SPECIAL_ROWS) - 1      # index (into the rows) of that cell


def special_value_case(n_cells: int = 4096 + 8, seed: int = 0):
    """The table above laid out on a level of n_cells cells -> (grid [1, n_cells], indices int64 [m], candidates [m],
    cells int64 [rows] (where each row sits), expected [rows] (NaN where the row is compared by value)).  The rows sit
    on cells scattered over the level, every other cell keeps a random positive value and is not listed.  Each row's
    candidates are listed twice, the second time in reverse order."""
    g = torch.Generator().manual_seed(seed)
    grid = torch.rand(1, n_cells, generator=g) * 3 + 0.5
    cells = torch.randperm(n_cells, generator=g)[:len(SPECIAL_ROWS)].sort().values
    idx, sig, exp = [], [], []
    for c, (old, cands, want) in zip(cells.tolist(), SPECIAL_ROWS):
        grid[0, c] = old
        for s in tuple(cands) + tuple(reversed(cands)):
            idx.append(c)
            sig.append(s)
        exp.append(NAN if want is None else want)
    return (grid, torch.tensor(idx, dtype=torch.int64), torch.tensor(sig, dtype=torch.float32), cells,
            torch.tensor(exp, dtype=torch.float32))


def update_loop(level, indices, sigmas, decay=DECAY):
    """Decayed-max update of one level as a plain Python loop over the candidates (float32 arithmetic through numpy)."""
    lvl = level.numpy().astype(np.float32).copy()
    best = {}
    for i, s in zip(indices.tolist(), sigmas.numpy().astype(np.float32)):
        if s >= 0:                                   # NaN and negatives: no candidate; -0.0 >= 0 holds
            s = np.float32(abs(s))                   # (-0.0 counts as 0)
            best[i] = s if i not in best or s > best[i] else best[i]
    for i, s in best.items():
        if lvl[i] >= 0:
            d = np.float32(lvl[i] * np.float32(decay))
            lvl[i] = d if d > s else s
    return torch.from_numpy(lvl)
