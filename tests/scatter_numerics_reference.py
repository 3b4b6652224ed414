"""The numeric contract of the two-pass bucketed scatter (csrc/grid_bin.hip pass 1, csrc/grid.hip pass 2) as a float64 /
integer reference, CPU only.  tests/test_scatter_numerics_cpu.py shows that the reference meets its own bound on every
input of tests/test_gpu_scatter_numerics.py; that module holds the kernels to it.  Bound 1 (x01 = (x + 1) / 2) throughout.

WHAT THE KERNELS COMPUTE (restated from the sources; positions, weights and rows as oracle/nerf_oracle.py grid_encode)
  addend    a[m, c, f] = ((wx * wy) * wz) * g[m, f] in f32, one per (sample, corner, feature), for row grid_corner_indices.
  record    non-merging level: one per (sample, corner) whose sample has a non-zero gradient; its values are the addends
            (12-byte records) or O.f26_round of them (8-byte records: 18 significant bits, ties away from zero).
            merging level (res <= scatter_compact_max_res): the samples of a wavefront (64 consecutive samples; an item is
            512 consecutive samples = 8 wavefronts) that follow each other in ONE cell form a run; the run's last lane emits
            one record per corner whose values are the f32 sums over the run (8-byte records: f26_round of the sum).
  bound     B_l = max |g| over the level's valid samples, times 64 (in f32) on a merging level; e_l its biased exponent
            (clamped to 1 .. 254), so |value| <= B_l < 2^(e_l - 126).
  bits      30 with 8-byte records, else min(44, 62 - lg), lg = the smallest integer >= 1 with 2^lg >= m_host.
  quantum   k = min(bits + 126 - e_l, 200), q_l = 2^-k (= 2^(e_l - 126 - bits) below the clamp): a record value v becomes the
            integer rne(v * 2^k) (the scaling is two exact f32 multiplications by powers of two), the integers of a row
            are added in int64 (wrapping), the sum S is converted to f32 once (round to nearest even) and multiplied by
            2^-(k / 2) and 2^-(k - k / 2) (C division).

THE RUN SUM (grid_bin.hip wave_run_sums_x16).  It is a SEGMENTED Hillis-Steele scan, not a difference of wave prefix sums
(grid_shared.h run_sum is the older form and has no caller in pass 1): six steps -- distances 1, 2, 4, 8 inside a row of 16
lanes, then "the previous row's last lane" for rows 1 and 3, then "lane 31" for rows 2 and 3 -- each one fused
multiply-add value += source * f with f = 1 where the source lane belongs to the lane's run, else 0.  source * f is exact,
so a step is one f32 addition, and a lane's result is a summation tree over the lanes of its run up to itself in which
every addend passes through at most SIX additions.  For such a tree |computed - exact| <= gamma_6 * sum |addend| with
gamma_6 = 6 u / (1 - 6 u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2; additions whose
result is subnormal are exact).  The absolute sum is the RUN's, not the wavefront's: nothing outside the run is ever added.
reference() executes the six steps as written (run_scan), so its records are meant to equal the kernel's.

THE ERROR BOUND per (row, feature), against truth = the exact sum of the row's f32 addends (8-byte records on a non-merging
level: of their f26_round, so that the record format's own rounding is not charged to the sums):
  E1 = n_row * q_l / 2                               round to nearest of each of the row's n_row non-zero record values
     + sum over the row's merged records of gamma_6 * (the run's sum of |addend|)           merging levels
     + sum over the row's merged records of (2^-18 * |run sum| + 2^-144)                    merging levels, 8-byte records:
                                                      half a unit of the 18th significant bit; 2^-144 = half the format's
                                                      spacing 2^-143 where the run sum is subnormal
  so |S * q_l - truth| <= E1 (the integer sum itself is exact; whether it can wrap is the head-room rule's business and
  is checked by reference()'s emulation, which reports any |S| >= 2^63: Reference.wrapped).  Then
  bound = E1 + 2^-24 * (|truth| + E1)                one rounding of S to f32: relative 2^-24 of |S| q_l <= |truth| + E1
        + 2^-149                                     the two un-scaling multiplications are exact unless their result is
                                                      subnormal; then each rounds by at most 2^-150 (k >= 0 there, so the
                                                      second factor is <= 1 and does not enlarge the first error)
The bound is evaluated in float64; it is multiplied by 1 + 2^-30 to cover that evaluation and nothing else.  Nothing in it
is fitted to kernel output.

EXACT SUMS.  truth is accumulated in float64 and PROVEN exact per row: with t the smallest unit in the last place among
the row's addends (every f32 is an integer multiple of 2^(exponent - 24)) and A the row's sum of |addend|, A < 2^(t + 52)
makes every partial sum an integer multiple of 2^t below 2^(t + 53), i.e. a float64.  Rows that fail the test (a few, where
addends 2^20 apart meet) are summed with fractions.Fraction and compared in exact arithmetic (Reference.abs_error).
"""
import fractions
import functools

import numpy as np
import torch

from oracle import nerf_oracle as O

WAVE, ITEM = 64, 512
BK_SHIFT = 12
U = 2.0 ** -24
SCAN_DEPTH = 6
GAMMA = SCAN_DEPTH * U / (1.0 - SCAN_DEPTH * U)
SLACK = 1.0 + 2.0 ** -30        # float64 evaluation of the bound itself
SLICE_RECS = 16384              # records per slice workgroup of pass 2 (grid.hip REDUCE_SLICE_RECS)

# ---- the table of tests/test_gpu_adam_skip.py
L, BASE, DESIRED, LOG2_T = 5, 16, 31, 13
OFFSETS = [0, 4920, 12920, 21112, 29304, 37496]
CAP_SLICED, CAP_PLAIN = 32768, 4096      # m_host: two slices planned per bucket / one
M = 4000                                 # samples of every case but the head-room one (m_dev; not a multiple of 64)
COMPACT_DEFAULT = 512


def levels(gridtype):
    lv = O.make_grid_levels(L, 2, BASE, DESIRED, LOG2_T, blocked=gridtype == "blocked")
    assert lv.offsets == OFFSETS, lv.offsets
    return lv


def fix_bits(m_host, rec8=False):
    """grid.hip fill_bucket_meta / FixBits."""
    if rec8:
        return 30
    lg = 1
    while (1 << lg) < m_host:
        lg += 1
    return min(44, 62 - lg)


def planned_slices(lv, l, m_host):
    nb = -(-(lv.offsets[l + 1] - lv.offsets[l]) // 4096)
    return max(1, min(64, (-(-8 * m_host // nb) + 65535) // 65536))


def f26(a):
    """O.f26_round on a numpy f32 array."""
    return O.f26_round(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))).numpy()


def geometry(x_world, lv):
    """Per level (w f32 [M, 8], rows int64 [M, 8] inside the level, cell int64 [M, 3]): grid_encode's arithmetic."""
    x = torch.as_tensor(x_world, dtype=torch.float32)
    x01 = (x + 1.0) / 2.0
    out = []
    for l in range(lv.num_levels):
        scale = torch.tensor(lv.scales[l], dtype=torch.float32)
        hs = lv.offsets[l + 1] - lv.offsets[l]
        pos = x01 * scale
        pos = pos + 0.5
        pg = torch.floor(pos)
        frac = pos - pg
        pg = pg.to(torch.int64)
        w, rows = [], []
        for c in range(8):
            bx, by, bz = c & 1, (c >> 1) & 1, (c >> 2) & 1
            wx = frac[:, 0] if bx else 1.0 - frac[:, 0]
            wy = frac[:, 1] if by else 1.0 - frac[:, 1]
            wz = frac[:, 2] if bz else 1.0 - frac[:, 2]
            w.append((wx * wy) * wz)
            corner = pg + torch.tensor([bx, by, bz], dtype=torch.int64)
            rows.append(O.grid_corner_indices(corner, lv.resolutions[l], hs, getattr(lv, "blocked", False),
                                              getattr(lv, "tiled", False)))
        out.append((torch.stack(w, 1).numpy(), torch.stack(rows, 1).numpy(), pg.numpy()))
    return out


def run_scan(V, d, start):
    """The six steps of wave_run_sums_x16 on V f32 [waves, 64, K]; d, start int [waves, 64]: lanes of the run before the
    lane / the run's first lane.  -> the inclusive run sums, every lane."""
    lane = np.arange(WAVE)
    V = V.copy()
    for dist in (1, 2, 4, 8):
        src = np.zeros_like(V)
        ok = (lane & 15) >= dist                      # (a source outside the row of 16 reads as zero)
        src[:, ok] = V[:, lane[ok] - dist]
        V = (V + src * (d >= dist)[..., None].astype(np.float32)).astype(np.float32)
    src = np.zeros_like(V)
    for r in (1, 3):
        src[:, 16 * r:16 * r + 16] = V[:, 16 * r - 1:16 * r]
    f = (d > (lane & 15)[None]) & np.isin(lane >> 4, (1, 3))[None]
    V = (V + src * f[..., None].astype(np.float32)).astype(np.float32)
    src = np.zeros_like(V)
    src[:, 32:] = V[:, 31:32]
    f = (start < 32) & (lane >= 32)[None]
    return (V + src * f[..., None].astype(np.float32)).astype(np.float32)


def exact_sums(idx, vals, n):
    """Exact per-index sums of f32 values.  -> (float64 [n]: exact where `proven`, else the nearest double; proven bool
    [n]; {index: Fraction} for the others)."""
    vals = vals.astype(np.float64)
    nz = vals != 0
    idx, vals = idx[nz], vals[nz]
    _, e = np.frexp(vals)
    ulp = np.maximum(e - 24, -149)
    t = np.full(n, 10000, dtype=np.int64)
    np.minimum.at(t, idx, ulp)
    A = np.bincount(idx, np.abs(vals), n)
    s = np.bincount(idx, vals, n)
    proven = (A == 0) | (np.ldexp(A, -(np.minimum(t, 2000) + 52).astype(np.int64)) < 1.0)
    exact = {}
    bad = np.nonzero(~proven)[0]
    if len(bad):
        sel = np.isin(idx, bad)
        for i, v in zip(idx[sel].tolist(), vals[sel].tolist()):
            exact[i] = exact.get(i, 0) + fractions.Fraction(v)
        for i, fr in exact.items():
            s[i] = float(fr)
    return s, proven, exact


class Reference:
    """Fields (rows are table rows, level offsets included): truth, bound float64 [rows, 2]; emu f32 [rows, 2]; n_rec
    int64 [rows, 2]; per level B (f32), e, bits, k, q; bucket_recs[l] = emitted records per bucket; wrapped = the
    emulation's |integer sum| reached 2^63 somewhere; records[l] = (rows [n, 8], values f32 [n, 8, 2]); addends[l]."""

    def abs_error(self, got):
        """|got - truth| float64 [rows, 2]; exact arithmetic where truth is no float64."""
        got = np.asarray(got, dtype=np.float64)
        err = np.abs(got - self.truth)
        flat = err.reshape(-1)
        for i, fr in self.exact.items():
            flat[i] = float(abs(fractions.Fraction(float(got.reshape(-1)[i])) - fr))
        return err

    def ratios(self, got):
        """Per level the worst |got - truth| / bound (0 / 0 = 0)."""
        err = self.abs_error(got)
        r = np.where(err == 0, 0.0, err / self.bound)
        return [float(r[a:b].max()) for a, b in zip(self.offsets[:-1], self.offsets[1:])]


def reference(x_world, dfeat, lv, m_host, rec8, merge, m=None, skip_zero=True, geom=None, bits=None):
    """x_world f32 [>= m, 3]; dfeat f32 [L, stride, 2] level-major; merge: per level, whether runs are merged (None: the
    default rule res <= 512); bits: overrides the head-room rule (the CPU test of the rule).  Finite gradients only."""
    x_world = np.asarray(x_world, dtype=np.float32)
    dfeat = np.asarray(dfeat, dtype=np.float32)
    m = x_world.shape[0] if m is None else m
    if merge is None:
        merge = [r <= COMPACT_DEFAULT for r in lv.resolutions]
    geom = geometry(x_world[:m], lv) if geom is None else geom
    n_rows = lv.offsets[-1]
    R = Reference()
    R.offsets, R.exact, R.wrapped = list(lv.offsets), {}, False
    R.truth, R.bound = np.zeros((n_rows, 2)), np.zeros((n_rows, 2))
    R.emu, R.n_rec = np.zeros((n_rows, 2), dtype=np.float32), np.zeros((n_rows, 2), dtype=np.int64)
    R.B, R.e, R.k, R.q, R.bucket_recs, R.records, R.addends = [], [], [], [], [], [], []
    R.bits = fix_bits(m_host, rec8) if bits is None else bits
    for l in range(lv.num_levels):
        w, rows, cell = geom[l]
        g = dfeat[l, :m]
        assert np.isfinite(g).all()
        hs = lv.offsets[l + 1] - lv.offsets[l]
        a = (w[:, :, None] * g[:, None, :]).astype(np.float32)            # [m, 8, 2]
        nzg = (g != 0).any(-1)
        B = np.float32(np.abs(g).max()) if m else np.float32(0)
        if merge[l]:
            B = np.float32(B * np.float32(64.0))
        e = min(max(int(B.view(np.uint32)) >> 23, 1), 254)
        k = min(R.bits + 126 - e, 200)
        q = 2.0 ** -k
        merge_err = None
        if not merge[l]:
            emit = nzg if skip_zero else np.ones(m, dtype=bool)
            rec_rows, rec_val = rows[emit], a[emit]
            if rec8:
                rec_val = f26(rec_val)
            t_rows, t_val = rec_rows, rec_val
        else:
            nw = -(-m // WAVE)
            pad = nw * WAVE - m
            valid = np.arange(nw * WAVE) < m
            cellp = np.concatenate([cell, np.full((pad, 3), -7, dtype=np.int64)])
            head = np.ones(nw * WAVE, dtype=bool)
            head[1:] = (cellp[1:] != cellp[:-1]).any(-1) | ~valid[1:] | ~valid[:-1]
            head[::WAVE] = True
            lane = np.tile(np.arange(WAVE), nw)
            run = np.cumsum(head) - 1
            start = np.maximum.accumulate(np.where(head, lane, 0).reshape(nw, WAVE), axis=1).reshape(-1)
            V = np.concatenate([a.reshape(m, 16), np.zeros((pad, 16), dtype=np.float32)]).reshape(nw, WAVE, 16)
            S = run_scan(V, (lane - start).reshape(nw, WAVE), start.reshape(nw, WAVE)).reshape(-1, 8, 2)
            tail = np.ones(nw * WAVE, dtype=bool)
            tail[:-1] = head[1:]
            nz_run = np.bincount(run, np.concatenate([nzg, np.zeros(pad, dtype=bool)]), run[-1] + 1) > 0
            emit = valid & tail & (nz_run[run] if skip_zero else True)
            rowsp = np.concatenate([rows, np.zeros((pad, 8), dtype=np.int64)])
            rec_rows, rec_val = rowsp[emit], S[emit]
            run_abs = np.zeros((run[-1] + 1, 16))
            np.add.at(run_abs, run[:m], np.abs(a.reshape(m, 16).astype(np.float64)))
            merge_err = GAMMA * run_abs[run[emit]].reshape(-1, 8, 2)
            if rec8:
                rec_val = f26(rec_val)
                merge_err = merge_err + 2.0 ** -18 * np.abs(S[emit].astype(np.float64)) + 2.0 ** -144
            t_rows, t_val = rows, a
        flat = lambda r: ((r[:, :, None] * 2) + np.arange(2)[None, None, :]).reshape(-1)   # noqa: E731  (row, feature) index
        truth, _, exact = exact_sums(flat(t_rows), t_val.reshape(-1), hs * 2)
        ridx, rval = flat(rec_rows), rec_val.reshape(-1).astype(np.float64)
        n_rec = np.bincount(ridx[rval != 0], minlength=hs * 2)
        E1 = n_rec * (q / 2)
        if merge_err is not None:
            E1 = E1 + np.bincount(ridx, merge_err.reshape(-1), hs * 2)
        bound = (E1 + U * (np.abs(truth) + E1) + 2.0 ** -149) * SLACK
        # the integer emulation: quantise, add in int64, convert once, un-scale in two steps
        qi = np.rint(np.ldexp(rval, k))
        if rec8:
            qi = np.clip(qi, -2.0 ** 31, 2.0 ** 31 - 1)                   # (__float2int_rn saturates; never reached)
        qi = qi.astype(np.int64)
        hi = np.bincount(ridx, (qi >> 22).astype(np.float64), hs * 2)     # (each below 2^53: exact)
        lo = np.bincount(ridx, (qi & ((1 << 22) - 1)).astype(np.float64), hs * 2)
        R.wrapped = R.wrapped or bool((np.abs(hi * 2.0 ** 22 + lo) >= 2.0 ** 63).any())
        tot = ((hi.astype(np.int64).astype(np.uint64) << np.uint64(22)) + lo.astype(np.int64).astype(np.uint64)).view(np.int64)
        ka = int(k / 2)                                                   # (C division: towards zero)
        emu = (tot.astype(np.float32) * np.float32(2.0 ** -ka)).astype(np.float32) * np.float32(2.0 ** -(k - ka))
        a0, a1 = lv.offsets[l], lv.offsets[l + 1]
        R.truth[a0:a1], R.bound[a0:a1] = truth.reshape(hs, 2), bound.reshape(hs, 2)
        R.emu[a0:a1], R.n_rec[a0:a1] = emu.astype(np.float32).reshape(hs, 2), n_rec.reshape(hs, 2)
        for i, fr in exact.items():
            R.exact[a0 * 2 + i] = fr
        R.B.append(B); R.e.append(e); R.k.append(k); R.q.append(q)
        R.bucket_recs.append(np.bincount(rec_rows.reshape(-1) >> BK_SHIFT, minlength=-(-hs // 4096)))
        R.records.append((rec_rows, rec_val))
        R.addends.append(a)
    return R


# ------------------------------------------------------------------------------------------------ the shared inputs
RAY_LEN, N_RAY_SAMPLES = 47, 2021       # 43 rays of 47 samples (runs of a few lanes), then 1979 scattered samples
MIN_NORMAL = 2.0 ** -62                 # a non-zero value must stay normal when scaled by 2^-64 ...
MAX_NORMAL = 2.0 ** 62                  # ... and finite when scaled by 2^64 (and by the 64 of a merged level's bound)
SCALES = (-64, -20, 20, 64)
RUN_LO, RUN_HI = 128, 176               # 48 samples at ONE point: a run over three 16-lane rows and lane 32 on every level


def _draw_positions(gen, n_rays):
    """x01 [M, 3]: z01 <= 0.8 keeps every record of level 0 in its first bucket (rows x + 17 y + 289 z < 4096)."""
    o = torch.rand(n_rays, 1, 3, generator=gen) * torch.tensor([0.5, 0.5, 0.4]) + 0.1
    d = torch.nn.functional.normalize(torch.randn(n_rays, 1, 3, generator=gen), dim=-1)
    t = torch.arange(RAY_LEN).view(1, RAY_LEN, 1) * 0.006
    rays = (o + d * t).reshape(-1, 3)
    rest = torch.rand(M - N_RAY_SAMPLES, 3, generator=gen) * torch.tensor([0.96, 0.96, 0.78]) + 0.02
    x01 = torch.cat([rays, rest])
    x01[RUN_LO:RUN_HI] = x01[RUN_LO].clone()
    x01[:, 2].clamp_(0.0, 0.8)
    return x01.clamp_(0.0, 1.0)


def _violations(x_world, g, lv):
    """Samples with an addend, a run sum or a record that is neither zero nor safely normal (merging on and off)."""
    bad = np.zeros(M, dtype=bool)
    for merge in (False, True):
        ref = reference(x_world, g, lv, CAP_PLAIN, True, [merge] * L)
        for l in range(L):
            a = np.abs(ref.addends[l].astype(np.float64)).reshape(M, -1)
            bad |= ((a != 0) & ((a < MIN_NORMAL) | (a > MAX_NORMAL))).any(-1)
            v = np.abs(ref.records[l][1].astype(np.float64))
            if bool(((v != 0) & ((v < MIN_NORMAL) | (v > MAX_NORMAL))).any()):
                bad |= True    # (a run sum that cancelled: not attributable to one sample -- redraw everything)
    return bad


@functools.lru_cache(maxsize=None)
def base_inputs():
    """(x_world f32 [M, 3], g f32 [L, M, 2]): the positions and the unit-magnitude gradients every case derives from.
    The last 6 samples of every ray have an exactly zero gradient (skipped records, runs with a zero tail).  A sample
    that would break the equivariance test's premise (every non-zero value normal at every scale) is drawn again."""
    gen = torch.Generator().manual_seed(20260)
    x01 = _draw_positions(gen, N_RAY_SAMPLES // RAY_LEN)
    g = torch.randn(L, M, 2, generator=gen)
    dead = (torch.arange(M) < N_RAY_SAMPLES) & ((torch.arange(M) % RAY_LEN) >= RAY_LEN - 6)
    g[:, dead] = 0.0
    lv = levels("hash")
    for attempt in range(1, 9):
        x = (x01 * 2.0 - 1.0).numpy()
        bad = _violations(x, g.numpy(), lv) | _violations(x, g.numpy(), levels("blocked"))
        if not bad.any():
            return x, g.numpy()
        fresh = torch.rand(M, 3, generator=torch.Generator().manual_seed(20260 + attempt)) * torch.tensor([0.96, 0.96, 0.78]) + 0.02
        x01[torch.from_numpy(bad)] = fresh[torch.from_numpy(bad)]
    raise AssertionError("no admissible sample set in 8 draws")


BIG_SAMPLES = (3, 40, 41, 700, 1999, 2500, 2501, 3999)     # the few samples 2^20 above the rest (rays and scattered ones)
MAGNITUDES = (-40, -20, 0, 20)


def bound_inputs():
    """[(name, g f32 [L, M, 2])] of the bound test: four magnitudes, per-level magnitudes 2^10 apart, a few large samples, a
    long run at the level's maximum."""
    _, g = base_inputs()
    out = [("2^%d" % s, np.ldexp(g, s).astype(np.float32)) for s in MAGNITUDES]
    out.append(("levels 2^10 apart", np.ldexp(g, (10 * (np.arange(L) - 2))[:, None, None]).astype(np.float32)))
    big = g.copy()
    big[:, list(BIG_SAMPLES)] = np.ldexp(big[:, list(BIG_SAMPLES)], 20)
    out.append(("8 samples 2^20 above", big))
    # the 48-lane run with every gradient AT the level's maximum: its sum is at least 48 / 8 = 6 times the largest |g| (one
    # corner of a cell has weight >= 1 / 8), which only the 64 in a merging level's bound makes room for
    top = g.copy()
    top[:, RUN_LO:RUN_HI] = np.abs(g).max(axis=(1, 2))[:, None, None]
    out.append(("a 48-lane run at the maximum", top))
    return out


def as_bf16(g):
    return torch.from_numpy(g).to(torch.bfloat16).float().numpy()


# ---- the head-room input: one dense level of its own, every sample exactly on one lattice vertex
HR_M = (1 << 19) + 512
HR_OFFSETS, HR_SCALE, HR_RES = [0, 5832], 16.0, 17         # 18^3 vertices
HR_G = float(np.float32(2.0) - np.float32(2.0 ** -23))     # the largest f32 below 2


def headroom_levels():
    return O.GridLevels(1, 2, HR_RES, HR_RES, 16, list(HR_OFFSETS), [HR_SCALE], [HR_RES])


def headroom_inputs(sign):
    """x = 7 / 16 - 1 on every axis: pos = 16 * (7 / 32) + 0.5 = 4 exactly, corner 0 has weight 1, the others 0.
    sign: +1, -1, or 0 = alternating +, -, ... (the exact sum is 0)."""
    x = np.full((HR_M, 3), 7.0 / 16.0 - 1.0, dtype=np.float32)
    s = np.where(np.arange(HR_M) % 2 == 0, 1.0, -1.0) if sign == 0 else np.full(HR_M, float(sign))
    g = (s * HR_G).astype(np.float32)[None, :, None].repeat(2, axis=2)
    return x, np.ascontiguousarray(g)


def headroom_geometry():
    w = np.zeros((HR_M, 8), dtype=np.float32)
    w[:, 0] = 1.0
    st = HR_RES + 1
    corner = 4 + np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])
    rows = (corner[:, 0] + corner[:, 1] * st + corner[:, 2] * st * st)[None].repeat(HR_M, axis=0)
    return [(w, rows.astype(np.int64), np.full((HR_M, 3), 4, dtype=np.int64))]


@functools.lru_cache(maxsize=None)
def base_geometry(gridtype):
    return geometry(base_inputs()[0], levels(gridtype))


def base_reference(g, gridtype, rec8, merge_on, m_host=CAP_PLAIN):
    """reference() of gradients g on the shared positions (every level of the table has res <= 512: merging is all or
    nothing, scatter_compact_max_res = 512 or 0)."""
    return reference(base_inputs()[0], g, levels(gridtype), m_host, rec8, [bool(merge_on)] * L, geom=base_geometry(gridtype))


@functools.lru_cache(maxsize=None)
def bound_reference(kind, bf16, gridtype, rec8, merge_on):
    """The reference of bound_inputs()[kind] (shared by the tests that need it; do not modify).  The capacity does not
    enter: fix_bits is 44 at both."""
    assert fix_bits(CAP_PLAIN) == fix_bits(CAP_SLICED) == 44
    g = bound_inputs()[kind][1]
    return base_reference(as_bf16(g) if bf16 else g, gridtype, rec8, merge_on)
