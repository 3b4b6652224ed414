"""tests/scatter_numerics_reference.py against itself, before anything runs on a GPU: its integer emulation of the
bucketed scatter (quantise, add in int64, convert once, un-scale) stays within its own derived bound on every input of
tests/test_gpu_scatter_numerics.py, is equivariant under power-of-two scaling there, and the head-room input
discriminates between the head-room rule and a fixed 44 bits."""
import numpy as np
import pytest

from tests import scatter_numerics_reference as R

LAYOUTS = ("hash", "blocked")


def test_fix_bits_rule_gives_the_values_the_kernel_source_quotes():
    """grid.hip fill_bucket_meta: 44 bits up to 2^18 samples, 42 at the bench's 640 Ki, 39 with eight views in a batch."""
    assert R.fix_bits(1) == R.fix_bits(4096) == R.fix_bits(32768) == R.fix_bits(1 << 18) == 44
    assert R.fix_bits((1 << 18) + 1) == 43
    assert R.fix_bits(640 * 1024) == 42
    assert R.fix_bits(8 * 640 * 1024) == 39
    assert R.fix_bits(R.HR_M) == 42
    assert R.fix_bits(1 << 27, rec8=True) == 30
    for lg in range(1, 28):       # bits + ceil(log2 m_host) <= 62, whatever m_host
        for m_host in ((1 << lg) - 1, 1 << lg, (1 << lg) + 1):
            assert R.fix_bits(m_host) + int(np.ceil(np.log2(max(m_host, 2)))) <= 62


def test_run_scan_is_a_depth_six_summation():
    """The emulated segmented scan: exact on integers (any run layout, runs over the 16-lane rows and lane 32), and within
    gamma_6 * sum |addend| of the exact run sum on random values."""
    rng = np.random.default_rng(5)
    for trial in range(20):
        head = rng.random((3, 64)) < (0.02, 0.2, 0.6)[trial % 3]
        head[:, 0] = True
        lane = np.arange(64)[None].repeat(3, 0)
        start = np.maximum.accumulate(np.where(head, lane, 0), axis=1)
        ints = rng.integers(-1000, 1000, (3, 64, 2)).astype(np.float32)
        vals = rng.standard_normal((3, 64, 2)).astype(np.float32)
        for V, exact in ((ints, True), (vals, False)):
            S = R.run_scan(V, lane - start, start)
            for w in range(3):
                for i in range(64):
                    seg = V[w, start[w, i]:i + 1].astype(np.float64)
                    want, room = seg.sum(0), R.GAMMA * np.abs(seg).sum(0)
                    if exact:
                        assert (S[w, i] == want).all(), (trial, w, i)
                    else:
                        assert (np.abs(S[w, i] - want) <= room).all(), (trial, w, i)


def test_the_inputs_have_runs_zero_tails_partial_waves_and_real_slices():
    x, g = R.base_inputs()
    assert x.shape == (R.M, 3) and R.M % 64 != 0 and R.M % 512 != 0
    assert int(((g == 0).all(-1)).all(0).sum()) >= 200
    for gridtype in LAYOUTS:
        lv = R.levels(gridtype)
        assert all(r <= R.COMPACT_DEFAULT for r in lv.resolutions)
        assert all(R.planned_slices(lv, l, R.CAP_SLICED) == 2 and R.planned_slices(lv, l, R.CAP_PLAIN) == 1 for l in range(R.L))
        off, on = (R.base_reference(g, gridtype, False, m) for m in (False, True))
        for l in range(R.L):
            assert int(on.bucket_recs[l].sum()) < int(off.bucket_recs[l].sum())      # runs were merged
        # level 0's first bucket is really cut in two at the sliced capacity, merging on or off
        assert int(off.bucket_recs[0][0]) > R.SLICE_RECS and int(on.bucket_recs[0][0]) > R.SLICE_RECS
        # the long run: one cell on every level, its run sum above twice the largest |g| (what the 64 of B_l is for)
        top = R.bound_reference(6, False, gridtype, True, True)
        for l in range(R.L):
            assert float(np.abs(top.records[l][1]).max()) > 4 * float(top.B[l]) / 64
        # 8-byte records: small addends next to the large samples round to zero, and the bound says so
        big = R.bound_reference(5, False, gridtype, True, False)
        lost = (big.emu == 0) & (big.truth != 0)
        assert int(lost.sum()) > 0 and bool((np.abs(big.truth[lost]) <= big.bound[lost]).all())


@pytest.mark.parametrize("merge_on", [False, True])
@pytest.mark.parametrize("rec8", [False, True])
@pytest.mark.parametrize("gridtype", LAYOUTS)
def test_emulation_stays_within_the_derived_bound(gridtype, rec8, merge_on):
    """Every input of the GPU module's bound test, f32 and bf16 gradients: the emulation is inside the bound, no int64 sum
    wraps, and on merging levels the emulation does differ from the exact sum (the bound is not vacuous there)."""
    worst = 0.0
    for kind, (name, _) in enumerate(R.bound_inputs()):
        for bf16 in (False, True):
            ref = R.bound_reference(kind, bf16, gridtype, rec8, merge_on)
            assert not ref.wrapped
            assert np.isfinite(ref.bound).all() and (ref.bound > 0).all()
            r = ref.ratios(ref.emu)
            assert max(r) <= 1.0, (name, bf16, r)
            worst = max(worst, max(r))
    print("emulation, %s rec%d merge=%d: worst |emu - truth| / bound %.3f" % (gridtype, 8 if rec8 else 12, merge_on, worst))
    assert worst > 0.0


@pytest.mark.parametrize("merge_on", [False, True])
@pytest.mark.parametrize("rec8", [False, True])
@pytest.mark.parametrize("gridtype", LAYOUTS)
def test_emulation_is_equivariant_under_power_of_two_scaling(gridtype, rec8, merge_on):
    """emu(g * 2^s) == emu(g) * 2^s bit for bit for the scales of the GPU test, and its premise: every non-zero addend and
    record value is a normal float at every scale."""
    _, g = R.base_inputs()
    base = R.base_reference(g, gridtype, rec8, merge_on)
    assert max(base.ratios(base.emu)) <= 1.0
    for s in R.SCALES:
        ref = R.base_reference(np.ldexp(g, s).astype(np.float32), gridtype, rec8, merge_on)
        for l in range(R.L):
            for v in (ref.addends[l], ref.records[l][1]):
                v = np.abs(v.astype(np.float64))
                assert bool(((v == 0) | ((v >= 2.0 ** -126) & (v < 2.0 ** 127))).all()), (s, l)
            assert ref.e[l] == base.e[l] + s and ref.k[l] == base.k[l] - s
        want = np.ldexp(base.emu, s).astype(np.float32)
        assert np.array_equal(ref.emu.view(np.int32), want.view(np.int32)), s
        assert max(ref.ratios(ref.emu)) <= 1.0


def test_headroom_positions_sit_on_one_vertex():
    x, _ = R.headroom_inputs(+1)
    got = R.geometry(x[:130], R.headroom_levels())[0]
    want = R.headroom_geometry()[0]
    for a, b in zip(got, want):
        assert np.array_equal(a, b[:130])


@pytest.mark.parametrize("merge_on", [False, True])
def test_headroom_input_overflows_44_bits_and_not_the_rule(merge_on):
    """2^19 + 512 addends of +-(2 - 2^-23) on one row: with 44 bits the int64 sum passes 2^63 (and the wrapped result is
    far outside the bound), with the rule's 42 it does not and the emulation is inside the bound; the alternating case
    sums to exactly +0."""
    lv, geom = R.headroom_levels(), R.headroom_geometry()
    assert R.HR_M % 512 == 0 and R.HR_M > (1 << 19)
    for sign in (+1, -1, 0):
        x, g = R.headroom_inputs(sign)
        ok = R.reference(x, g, lv, R.HR_M, False, [merge_on], geom=geom)
        assert ok.bits == 42 and not ok.wrapped
        assert max(ok.ratios(ok.emu)) <= 1.0
        row = 4 + 4 * 18 + 4 * 18 * 18
        want = 0.0 if sign == 0 else sign * R.HR_M * R.HR_G
        assert ok.truth[row, 0] == want and ok.truth[row, 1] == want and float(np.abs(ok.truth).sum()) == 2 * abs(want)
        if sign == 0:
            assert int(ok.emu.view(np.int32)[row, 0]) == 0          # +0.0, not -0.0
        bad = R.reference(x, g, lv, R.HR_M, False, [merge_on], geom=geom, bits=44)
        # (merging on, a record stands for 64 samples and there are 64 times fewer: no sum comes near 2^63.  The case
        # that discriminates is merging off.)
        assert bad.wrapped == (sign != 0 and not merge_on)
        if bad.wrapped:
            assert max(bad.ratios(bad.emu)) > 1e6
