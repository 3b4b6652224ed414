"""The bucketed scatter's fixed-point sums (csrc/grid_bin.hip pass 1, csrc/grid.hip pass 2) against their numeric contract,
tests/scatter_numerics_reference.py (derivation of the bound in its docstring; tests/test_scatter_numerics_cpu.py shows on
the CPU that the reference meets every condition below on these very inputs):
  a. power-of-two equivariance, bit for bit (scale arithmetic away from exponent 127, f32 and bf16 wire output);
  b. a level's rows do not depend on the other levels' magnitudes (one bound per level, every level grouping);
  c. nothing leaks from the previous call through the workspace header (own clear, and the step tail's clear);
  d. |result - exact sum of the f32 addends| <= the derived bound, every row, magnitudes 2^-40 .. 2^20, per-level and
     in-level magnitude steps, merging on and off, sliced and unsliced, f32 and bf16-valued gradients;
  e. head-room: 2^19 + 512 addends at the level's bound on one row (the int64 sum wraps with a fixed 44 bits);
  f. non-finite gradients: the other levels and reproducibility, and nothing else.
The table is the small one of tests/test_gpu_adam_skip.py (dense and hashed levels, full and partial buckets, two slices
per bucket at capacity 32768); 4000 samples, 43 short rays (runs) and scattered ones.  The scatter takes f32 gradients
only (the C ABI refuses anything else): "bf16" gradients are bf16 values widened to f32, as the bf16 MLP hands them over.
Tuning goes through `tuning(...)`, which restores the whole default table."""
import contextlib
import types

import numpy as np
import pytest
import torch

from tests import exact_grid as X
from tests import scatter_numerics_reference as R

pytestmark = pytest.mark.gpu

CONFIGS = [(g, v) for g in ("hash", "blocked") for v in (2, 3)]
MERGE = (0, R.COMPACT_DEFAULT)          # scatter_compact_max_res: run merging off / on (every level has res <= 31)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


def _set(key, value):
    from src.latent_nerf.raymarching import backend as B
    B.call("lnerf_set_tuning", key.encode(), int(value))


def _restore_defaults():
    for k, v in X.TUNING_DEFAULTS.items():
        _set(k, v)


@contextlib.contextmanager
def tuning(**overrides):
    assert not set(overrides) - set(X.TUNING_DEFAULTS)
    try:
        for k, v in overrides.items():
            _set(k, v)
        yield
    finally:
        _restore_defaults()


def _levels(gridtype):
    from src.latent_nerf.models import encoding as E
    lv = E.GridLevels(R.L, 2, R.BASE, R.DESIRED, R.LOG2_T, gridtype=gridtype)
    assert lv.offsets == R.OFFSETS, lv.offsets
    return lv


class _Scene:
    """The shared positions on the device at one capacity (rows beyond M zero, never read: m_dev = M)."""

    def __init__(self, dev, gridtype, cap):
        self.dev, self.lv, self.cap = dev, _levels(gridtype), cap
        x = torch.zeros(cap, 3)
        x[:R.M] = torch.from_numpy(R.base_inputs()[0])
        self.x = x.to(dev)
        self.m_dev = torch.tensor([R.M], dtype=torch.int32, device=dev)

    def dfeat(self, g):
        d = torch.zeros(R.L, self.cap, 2)
        d[:, :R.M] = torch.as_tensor(g)
        return d.to(self.dev)

    def add(self, d, variant, flags=0):
        """dtable = 0 + scatter(d) through lnerf_grid_encode_backward."""
        from src.latent_nerf.models import encoding as E
        out = torch.zeros(self.lv.n_rows, 2, device=self.dev)
        E.grid_encode_backward(self.x, 1.0, d, self.lv, self.cap, self.m_dev, self.cap, out, variant=variant | flags)
        return out

    def wire(self, d, variant):
        """The bf16 wire output (lnerf_grid_encode_backward_bf16 through a GradSink)."""
        from src.latent_nerf.models import encoding as E
        enc = types.SimpleNamespace(levels=self.lv, grad_sink=E.GradSink(torch.empty(self.lv.n_rows, 2, device=self.dev)))
        enc.grad_sink.wire.fill_(7.0)                     # (every row is written)
        E.grid_encode_backward_bf16(self.x, 1.0, d, enc, self.cap, self.m_dev, self.cap, variant)
        return enc.grad_sink.wire


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _diff(got, want, offsets):
    bad = (_bits(got) != _bits(want)).any(-1)
    per = [int(bad[a:b].sum()) for a, b in zip(offsets[:-1], offsets[1:])]
    first = torch.nonzero(bad).flatten()[:6].tolist()
    pairs = [(got[i].float().tolist(), want[i].float().tolist()) for i in first[:2]]
    return "rows that differ per level %s, first %s: (got, want) %s" % (per, first, pairs)


def _really_sliced(gridtype, merge):
    """From the reference's row rule: level 0's first bucket gets more records than one slice workgroup takes."""
    ref = R.base_reference(R.base_inputs()[1], gridtype, False, merge > 0)
    return int(ref.bucket_recs[0][0]) > R.SLICE_RECS


# ------------------------------------------------------------------------------------------------ a. equivariance
@pytest.mark.parametrize("gridtype,variant", CONFIGS)
def test_power_of_two_scaling_of_the_gradients_scales_the_result_bit_for_bit(dev, gridtype, variant):
    """scatter(g * 2^s) == scatter(g) * 2^s for s in {-64, -20, 20, 64}: the level bound, the split scale factors, the
    quantisation, the un-scaling and (merging on) the 64 of a run's bound are all exact under a power of two while no
    value is subnormal or overflows -- which the CPU module asserts for these inputs."""
    _, g = R.base_inputs()
    failures = []
    for cap in (R.CAP_PLAIN, R.CAP_SLICED):
        sc = _Scene(dev, gridtype, cap)
        for merge in MERGE:
            assert cap == R.CAP_PLAIN or _really_sliced(gridtype, merge)
            with tuning(scatter_compact_max_res=merge):
                for name, run in (("f32 add", sc.add), ("bf16 wire", sc.wire)):
                    base = run(sc.dfeat(g), variant).clone()
                    assert float(base.float().abs().max()) > 0
                    for s in R.SCALES:
                        got = run(sc.dfeat(np.ldexp(g, s).astype(np.float32)), variant)
                        # (scaled on the host with numpy's ldexp, which is exact; a device pow(2, s) need not be)
                        want = torch.from_numpy(np.ldexp(base.float().cpu().numpy(), s)).to(base.dtype)
                        if not torch.equal(_bits(got), _bits(want)):
                            failures.append("cap %d merge %d %s s=%d: %s" % (cap, merge, name, s, _diff(got, want, R.OFFSETS)))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ b. levels
@pytest.mark.parametrize("groups", [1, 4])
@pytest.mark.parametrize("gridtype,variant", CONFIGS)
def test_a_level_does_not_see_the_other_levels_magnitudes(dev, gridtype, variant, groups):
    """Every level in turn: the other levels' gradients times 2^40, and times 2^-40, leave its rows bit-identical."""
    _, g = R.base_inputs()
    sc = _Scene(dev, gridtype, R.CAP_SLICED)
    failures = []
    for merge in MERGE:
        with tuning(scatter_compact_max_res=merge, scatter_level_groups=groups):
            base = sc.add(sc.dfeat(g), variant)
            for l in range(R.L):
                for s in (40, -40):
                    shift = np.full(R.L, s)
                    shift[l] = 0
                    got = sc.add(sc.dfeat(np.ldexp(g, shift[:, None, None]).astype(np.float32)), variant)
                    a, b = R.OFFSETS[l], R.OFFSETS[l + 1]
                    if not torch.equal(_bits(got[a:b]), _bits(base[a:b])):
                        failures.append("merge %d level %d others * 2^%d: %s" % (merge, l, s, _diff(got[a:b], base[a:b], [0, b - a])))
                    o = (l + 1) % R.L                          # (and the shifted levels did move)
                    assert not torch.equal(got[R.OFFSETS[o]:R.OFFSETS[o + 1]], base[R.OFFSETS[o]:R.OFFSETS[o + 1]])
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ c. calls
def _maxima(ws):
    return ws[:4096].view(torch.int32)[::32][:R.L].clone()


@pytest.mark.parametrize("gridtype,variant", CONFIGS)
def test_nothing_leaks_from_the_previous_call(dev, gridtype, variant):
    """Call A (gradients * 2^40), then call B (* 2^-20) through the same workspace: B equals B on a workspace whose header
    was zeroed -- by the ordinary entry, which clears the level maxima itself, and with LNERF_SCATTER_CLEARED behind a
    step tail that was asked to clear them (LNERF_TAIL_CLEAR_SCATTER).  With the flag and WITHOUT the clear B does come out
    different (A's maxima scale it: the documented precision drop), so the comparison can tell."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    _, g = R.base_inputs()
    sc = _Scene(dev, gridtype, R.CAP_SLICED)
    lv = sc.lv
    dA, dB = sc.dfeat(np.ldexp(g, 40).astype(np.float32)), sc.dfeat(np.ldexp(g, -20).astype(np.float32))
    ws = E.scatter_workspace(lv, sc.cap, dev)
    table = torch.zeros(lv.n_rows, 2, device=dev)
    m, v, zero = torch.zeros_like(table), torch.zeros_like(table), torch.zeros_like(table)
    step_dev = torch.tensor([1, 0], device=dev, dtype=torch.int32)
    for merge in MERGE:
        with tuning(scatter_compact_max_res=merge):
            ws[:B.SCATTER_ZERO_HEAD_BYTES].zero_()
            want = sc.add(dB, variant, B.SCATTER_CLEARED).clone()      # (the header IS clear: nothing but B's own maxima)
            small = _maxima(ws)
            assert float(want.abs().max()) > 0 and int(small.min()) > 0
            # the ordinary entry
            sc.add(dA, variant)
            assert bool((_maxima(ws) > small).all())                   # A's maxima are in the header now
            got = sc.add(dB, variant)
            assert torch.equal(_bits(got), _bits(want)), "merge %d, un-flagged: %s" % (merge, _diff(got, want, R.OFFSETS))
            assert torch.equal(_maxima(ws), small)
            # the step tail clears, the next call is flagged
            sc.add(dA, variant)
            B.call("lnerf_step_tail", lv.num_levels, lv.level_dim, lv.c_offsets, lv.c_scales, lv.c_res, sc.cap, variant,
                   _p(ws), ws.numel(), _p(zero), _p(table), _p(m), _p(v), None, 1e-2, None, 0, B.BF16, 5, None, None, None,
                   1e-3, None, 0.9, 0.99, 1e-15, 1, _p(step_dev), 1.0, B.TAIL_CLEAR_SCATTER, _stream())
            assert int(_maxima(ws).abs().max()) == 0
            got = sc.add(dB, variant, B.SCATTER_CLEARED)
            assert torch.equal(_bits(got), _bits(want)), "merge %d, tail clear: %s" % (merge, _diff(got, want, R.OFFSETS))
            # flagged without a clear: stale maxima
            sc.add(dA, variant)
            stale = sc.add(dB, variant, B.SCATTER_CLEARED)
            assert not torch.equal(_bits(stale), _bits(want))
    assert float(table.abs().max()) == 0.0
    E.ws_mark_dirty(dev)


# ------------------------------------------------------------------------------------------------ d. the bound
@pytest.mark.parametrize("cap", [R.CAP_PLAIN, R.CAP_SLICED])
@pytest.mark.parametrize("gridtype,variant", CONFIGS)
def test_sums_stay_within_the_derived_bound_of_the_exact_sum(dev, gridtype, variant, cap):
    """Every row of every level, against the exact sum of the f32 addends: four magnitudes, levels 2^10 apart, eight
    samples 2^20 above the rest (8-byte records: many small addends round to zero there, and the bound says so), a
    48-lane run whose gradients are all at the level's maximum (its sum needs the 64 in a merging level's bound); f32 and
    bf16-valued gradients, merging off and on.  12-byte records: no row whose exact sum is above its bound comes out zero.
    Worst |got - truth| / bound per level (printed whether it passes or not; copied into DESIGN.md):
      measured on an MI355X: see DESIGN.md "Numeric contract of the bucketed scatter"."""
    sc = _Scene(dev, gridtype, cap)
    failures = []
    for merge in MERGE:
        assert cap == R.CAP_PLAIN or _really_sliced(gridtype, merge)
        worst, unlike = [0.0] * R.L, 0
        with tuning(scatter_compact_max_res=merge):
            for kind, (name, g) in enumerate(R.bound_inputs()):
                for bf16 in (False, True):
                    got = sc.add(sc.dfeat(R.as_bf16(g) if bf16 else g), variant).cpu().numpy()
                    ref = R.bound_reference(kind, bf16, gridtype, variant == 3, merge > 0)
                    r = ref.ratios(got)
                    worst = [max(a, b) for a, b in zip(worst, r)]
                    unlike += int((got != ref.emu).any(-1).sum())      # (reported, not asserted: the emulation is a model)
                    if max(r) > 1.0 or not np.isfinite(got).all():
                        failures.append("merge %d, %s, %s: worst ratio per level %s" % (
                            merge, name, "bf16" if bf16 else "f32", ["%.3g" % x for x in r]))
                    if variant == 2:
                        lost = (got == 0) & (np.abs(ref.truth) > ref.bound)
                        if lost.any():
                            failures.append("merge %d, %s: %d rows lost" % (merge, name, int(lost.sum())))
        print("\nbound: %s variant %d cap %d merge %d: worst ratio per level %s; rows unlike the CPU emulation: %d" % (
            gridtype, variant, cap, merge, " ".join("%.4f" % x for x in worst), unlike))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ e. head-room
@pytest.mark.parametrize("merge", MERGE)
def test_half_a_million_addends_at_the_bound_on_one_row(dev, merge):
    """One dense level, m_host = M = 2^19 + 512 samples exactly on one vertex, gradients all +(2 - 2^-23), all negative,
    alternating: 12-byte records get 42 bits here, and with 44 the int64 sum of the un-merged records would wrap (CPU
    module).  Within the bound of the exact sum; the alternating case is exactly +0.0."""
    from src.latent_nerf.models import encoding as E
    lv = X.device_levels("hash", offsets=tuple(R.HR_OFFSETS), scale=R.HR_SCALE, res=R.HR_RES)
    olv, geom = R.headroom_levels(), R.headroom_geometry()
    row = 4 + 4 * 18 + 4 * 18 * 18
    with tuning(scatter_compact_max_res=merge):
        for sign in (+1, -1, 0):
            x, g = R.headroom_inputs(sign)
            out = torch.zeros(lv.n_rows, 2, device=dev)
            E.grid_encode_backward(torch.from_numpy(x).to(dev), 1.0, torch.from_numpy(g).to(dev), lv, R.HR_M, None, R.HR_M,
                                   out, variant=2)
            got = out.cpu().numpy()
            ref = R.reference(x, g, olv, R.HR_M, False, [merge > 0], geom=geom)
            assert ref.bits == 42 and not ref.wrapped
            r = ref.ratios(got)
            print("\nhead-room: merge %d sign %+d: got %r truth %r, ratio %.3f" % (merge, sign, got[row].tolist(),
                                                                               ref.truth[row].tolist(), r[0]))
            assert r[0] <= 1.0, (sign, got[row].tolist(), ref.truth[row].tolist(), ref.bound[row].tolist())
            assert int(np.count_nonzero(got)) == (0 if sign == 0 else 2)
            if sign == 0:
                assert int(np.abs(got.view(np.int32)).max()) == 0      # +0.0 everywhere


# ------------------------------------------------------------------------------------------------ f. non-finite
@pytest.mark.parametrize("gridtype,variant", CONFIGS)
def test_a_non_finite_gradient_stays_inside_its_level_and_is_reproducible(dev, gridtype, variant):
    """One NaN, one +inf, one -inf in one sample of level 2 (pass 1 raises that level's bound to 3e38 and packs the
    wavefront's records the careful way): the call returns, the other levels are bit-identical to the run without it,
    two runs give the same bits.  What level 2's own rows hold is unspecified (include/lnerf_hip.h) and not asserted."""
    _, g = R.base_inputs()
    sc = _Scene(dev, gridtype, R.CAP_SLICED)
    lvl, sample = 2, 100
    assert g[lvl, sample, 0] != 0
    a, b = R.OFFSETS[lvl], R.OFFSETS[lvl + 1]
    for merge in MERGE:
        with tuning(scatter_compact_max_res=merge):
            base = sc.add(sc.dfeat(g), variant)
            for bad in (float("nan"), float("inf"), float("-inf")):
                g2 = g.copy()
                g2[lvl, sample, 0] = bad
                d = sc.dfeat(g2)
                one, two = sc.add(d, variant), sc.add(d, variant)
                torch.cuda.synchronize()
                assert torch.equal(_bits(one), _bits(two)), "merge %d %r: two runs differ" % (merge, bad)
                for lo, hi in ((0, a), (b, R.OFFSETS[-1])):
                    assert torch.equal(_bits(one[lo:hi]), _bits(base[lo:hi])), "merge %d %r: %s" % (
                        merge, bad, _diff(one[lo:hi], base[lo:hi], [0, hi - lo]))
                own = one[a:b].cpu()
                print("\nnon-finite %r, %s variant %d merge %d: level %d holds %d NaN, %d inf, %d non-zero values %s, "
                      "%d rows zero that were not" % (bad, gridtype, variant, merge, lvl, int(own.isnan().sum()),
                                                      int(own.isinf().sum()), int((own != 0).sum()),
                                                      sorted(set(own[own != 0].tolist()))[:4],
                                                      int(((own == 0) & (base[a:b].cpu() != 0)).all(-1).sum())))
