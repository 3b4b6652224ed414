"""The fused sigma/latent MLP, both precisions, against a plain float64 reference BIT FOR BIT (tests/exact_mlp.py).

On the exact inputs every MFMA operand is a bf16 value and every sum is exact in f32 in any order (asserted on the CPU by
tests/test_mlp_exact_inputs_cpu.py), so the latents, dfeat and the six parameter gradients of lnerf_mlp_forward /
lnerf_mlp_backward must EQUAL the reference -- in every work split, with and without a fragment workspace, for every
out_dim the ABI accepts, on f32 and bf16 features, at the tile edges (64 samples in f32, 128 in bf16), over persistent
tile loops and over more slabs than the reduction has lane groups.  A permuted k-order, a swapped weight fragment, a
dropped relu mask on one packed pair, a tile written by the wrong wave, one slab left out: each is a nonzero integer.
The one tolerance of the module is on sigma = expf(pre-activation): 4 ulp against the float64 exp of the SAME argument.
Outputs are pre-filled: rows at and beyond min(m_host, *m_dev) must keep the fill, gradients are written over NaN."""
import ctypes
import math

import pytest
import torch

from tests import exact_mlp as XM
from tests.test_gpu_tuning_paths import FILL, _restore_defaults, tuning

pytestmark = pytest.mark.gpu

SIGMA_RTOL = 2.0 ** -21        # 4 ulp of an f32: expf's own error plus the reference's rounding to f32
PRECISIONS = ["f32", "bf16"]
_sigma_err = {}                # precision -> largest relative error seen (printed by the module's last test)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


def _B():
    from src.latent_nerf.raymarching import backend as B
    return B


def _stream():
    from src.latent_nerf.raymarching.raymarching import _stream as s
    return s()


def _p(t, byte_offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + byte_offset)


def _tag(precision):
    return _B().BF16 if precision == "bf16" else _B().F32


def _ws_bytes(out_dim):
    return int(_B().get_lib().lnerf_mlp_backward_workspace_bytes(out_dim))


def _workspace(dev, out_dim, byte=0xFF):
    return torch.full((_ws_bytes(out_dim),), byte, device=dev, dtype=torch.uint8)


class Buffers:
    """One case on the device at capacity `stride` (= level_stride): rows >= M of every per-sample input hold `stale`."""

    def __init__(self, dev, case, stride, feat_dtype=torch.float32, stale=0.0):
        self.case, self.M, self.out_dim, self.stride, self.dev = case, case["M"], case["out_dim"], stride, dev
        self.feat = XM.level_major(case["x"], stride, stale, feat_dtype).to(dev)
        self.xyz = XM.padded(case["xyz"], stride, stale).to(dev)
        self.sigmas = XM.padded(case["sigmas"], stride, stale).to(dev)
        self.dsigmas = XM.padded(case["dsigmas"], stride, stale).to(dev)
        self.drgbs = XM.padded(case["drgbs"], stride, stale).to(dev)
        self.W = [case[k].to(dev) for k in XM.W_NAMES]
        self.feat_tag = _B().F32 if feat_dtype == torch.float32 else _B().BF16
        self.blob_scale = XM.BLOB_SCALE     # (tests/test_gpu_mlp_f32_bits.py runs with its own)

    def m_dev(self, value):
        return None if value is None else torch.tensor([value], dtype=torch.int32, device=self.dev)

    def forward_args(self, m_host, m_dev, sigmas, rgbs, tag, ws, out_dim=None, stride=None, blob_std=XM.BLOB_STD,
                     rgbs_offset=0, ws_bytes=None):
        return (_p(self.feat), self.feat_tag, int(self.stride if stride is None else stride), _p(self.xyz),
                *[_p(t) for t in self.W], int(self.out_dim if out_dim is None else out_dim), self.blob_scale, blob_std,
                int(m_host), _p(m_dev), _p(sigmas), _p(rgbs, rgbs_offset), tag, _p(ws),
                (0 if ws is None else ws.numel()) if ws_bytes is None else ws_bytes, _stream())

    def forward(self, precision, m_host, m_dev=None, ws=None, ready=False):
        """-> (sigmas [stride], rgbs [stride, out_dim - 1]) written over FILL."""
        sigmas = torch.full((self.stride,), FILL, device=self.dev)
        rgbs = torch.full((self.stride, self.out_dim - 1), FILL, device=self.dev)
        tag = _tag(precision) | (_B().MLP_FRAGMENTS_READY if ready else 0)
        count = self.m_dev(m_dev)       # (held until the call has been made)
        _B().call("lnerf_mlp_forward", *self.forward_args(m_host, count, sigmas, rgbs, tag, ws))
        return sigmas, rgbs

    def backward_args(self, m_host, m_dev, dfeat, grads, accumulate, ws, tag, clear=None, clear_bytes=0, out_dim=None,
                      stride=None, blob_std=XM.BLOB_STD, drgbs_offset=0, ws_bytes=None):
        return (_p(self.feat), self.feat_tag, int(self.stride if stride is None else stride), _p(self.xyz),
                *[_p(t) for t in self.W], int(self.out_dim if out_dim is None else out_dim), self.blob_scale, blob_std,
                int(m_host), _p(m_dev), _p(self.sigmas), _p(self.dsigmas), _p(self.drgbs, drgbs_offset), _p(dfeat),
                *[_p(g) for g in grads], int(accumulate), _p(ws), ws.numel() if ws_bytes is None else ws_bytes, tag,
                _p(clear), clear_bytes, _stream())

    def backward(self, precision, m_host, m_dev=None, ws=None, flags=0, accumulate=0, grads=None, clear=None,
                 clear_bytes=0):
        """-> (dfeat [16, stride, 2] written over FILL, the six gradients written over NaN unless `grads` is given)."""
        dfeat = torch.full((16, self.stride, 2), FILL, device=self.dev)
        if grads is None:
            grads = [torch.full_like(t, math.nan) for t in self.W]
        ws = _workspace(self.dev, self.out_dim) if ws is None else ws
        count = self.m_dev(m_dev)       # (held until the call has been made)
        _B().call("lnerf_mlp_backward", *self.backward_args(m_host, count, dfeat, grads, accumulate, ws,
                                                            _tag(precision) | flags, clear, clear_bytes))
        return dfeat, grads


def _check_forward(ctx, ref, M, sigmas, rgbs, precision, failures):
    """Latents of rows < M equal the reference, sigma within 4 ulp, rows >= M keep FILL."""
    sigmas, rgbs = sigmas.cpu(), rgbs.cpu()
    msg = XM.first_diff("latent", rgbs[:M], ref["h"][:M, 1:])
    if msg:
        failures.append("%s: %s" % (ctx, msg))
    want = ref["sigma"][:M]
    rel = ((sigmas[:M].double() - want) / want).abs()
    rel[~torch.isfinite(sigmas[:M])] = math.inf
    _sigma_err[precision] = max(_sigma_err.get(precision, 0.0), float(rel.max()))
    if float(rel.max()) > SIGMA_RTOL:
        i = int(rel.argmax())
        failures.append("%s: sigma[%d]: got %r want %r (relative error %.3g = %.2f ulp > 4 ulp)" % (
            ctx, i, float(sigmas[i]), float(want[i]), float(rel[i]), float(rel[i]) * 2.0 ** 23))
    for name, t in (("sigmas", sigmas), ("rgbs", rgbs)):
        if not bool((t[M:] == FILL).all()):
            row = M + int(torch.nonzero((t[M:] != FILL).reshape(t.shape[0] - M, -1).any(-1))[0])
            failures.append("%s: %s row %d (>= M = %d) was written" % (ctx, name, row, M))


def _check_backward(ctx, ref, M, dfeat, grads, failures, want_grads=None):
    """dfeat rows < M and the six gradients equal the reference, dfeat rows >= M keep FILL."""
    dfeat = dfeat.cpu()
    msg = XM.first_diff("dfeat[sample, feature]", XM.sample_major(dfeat, M), ref["dfeat"][:M])
    if msg:
        failures.append("%s: %s" % (ctx, msg))
    if not bool((dfeat[:, M:] == FILL).all()):
        row = M + int(torch.nonzero((dfeat[:, M:] != FILL).any(0).any(-1))[0])
        failures.append("%s: dfeat row %d (>= M = %d) was written" % (ctx, row, M))
    if grads is not None:
        for k, g in zip(XM.W_NAMES, grads):
            msg = XM.first_diff("d" + k, g, ref[k] if want_grads is None else want_grads[k])
            if msg:
                failures.append("%s: %s" % (ctx, msg))


def _size_forms(M):
    """(name, m_host, m_dev, stride): the count on the device below the capacity, and the count on the host alone."""
    return (("m_dev", M + 7, M, M + 7), ("m_host", M, None, M + 7))


FEATS = pytest.mark.parametrize("feat", ["f32", "bf16"])
OUT_DIMS = pytest.mark.parametrize("out_dim", XM.OUT_DIMS)
PREC = pytest.mark.parametrize("precision", PRECISIONS)


def _feat_dtype(feat):
    return torch.float32 if feat == "f32" else torch.bfloat16


# ------------------------------------------------------------------------------ forward
@PREC
@FEATS
@OUT_DIMS
def test_forward_exact(dev, precision, feat, out_dim):
    """M at and around the tile edges, both size forms.  out_dim 2, 4, 8: the generic store arm; 5: the 16-byte row
    store.  bf16 precision: per-workgroup fragment build (no workspace), the build launch (workspace), and a second call
    with LNERF_MLP_FRAGMENTS_READY on that workspace -- the same bits, each equal to the reference."""
    failures = []
    for M in XM.SMALL_M:
        ref = XM.exact_reference(M, out_dim)
        for form, m_host, m_dev, stride in _size_forms(M):
            b = Buffers(dev, XM.exact_case(M, out_dim), stride, _feat_dtype(feat))
            ctx = "M=%d %s" % (M, form)
            s0, r0 = b.forward(precision, m_host, m_dev)
            _check_forward(ctx, ref, M, s0, r0, precision, failures)
            if precision == "bf16":
                ws = _workspace(dev, out_dim)
                for name, ready in (("workspace", False), ("fragments ready", True)):
                    s, r = b.forward(precision, m_host, m_dev, ws=ws, ready=ready)
                    _check_forward(ctx + " " + name, ref, M, s, r, precision, failures)
                    if not torch.equal(s, s0):      # (sigma has a bound against the reference, not between the forms)
                        failures.append("%s %s: %s" % (ctx, name, XM.first_diff("sigma vs no workspace", s, s0)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("out_dim", XM.BIG_OUT_DIMS)
@FEATS
def test_forward_bf16_persistent_work_splits(dev, feat, out_dim):
    """M = 700 (6 tiles): k_mlp_forward_bf16<2> and <3> with 1, 2 and 768 persistent workgroups -- six, three and one
    tile per workgroup, the next tile's features prefetched.  Each equals the REFERENCE, not only the other splits."""
    M = XM.M_PERSISTENT
    ref = XM.exact_reference(M, out_dim)
    failures = []
    for form, m_host, m_dev, stride in _size_forms(M):
        b = Buffers(dev, XM.exact_case(M, out_dim), stride, _feat_dtype(feat))
        for wps in (2, 3):
            for blocks in (1, 2, 768):
                with tuning(mlp_fwd_wps=wps, mlp_fwd_blocks=blocks):
                    s, r = b.forward("bf16", m_host, m_dev)
                _check_forward("%s wps=%d blocks=%d" % (form, wps, blocks), ref, M, s, r, "bf16", failures)
    assert not failures, "\n".join(failures)


def test_forward_f32_several_tiles(dev):
    """The f32 forward over 11 tiles of 64 (M = 700), both feature types."""
    M, failures = XM.M_PERSISTENT, []
    for out_dim in XM.BIG_OUT_DIMS:
        for feat in ("f32", "bf16"):
            b = Buffers(dev, XM.exact_case(M, out_dim), M + 7, _feat_dtype(feat))
            s, r = b.forward("f32", M + 7, M)
            _check_forward("out_dim=%d feat=%s" % (out_dim, feat), XM.exact_reference(M, out_dim), M, s, r, "f32", failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------ backward
@PREC
@FEATS
@OUT_DIMS
def test_backward_exact(dev, precision, feat, out_dim):
    """The same grid of cases: dfeat and dw1 .. db3 (accumulate = 0, written over NaN) equal the reference.  out_dim 2,
    4, 8: the generic arm of load_upstream; 5: the 16-byte row load.  bf16 precision: with its own fragment build, and
    with LNERF_MLP_FRAGMENTS_READY after a forward on the same workspace."""
    failures = []
    for M in XM.SMALL_M:
        ref = XM.exact_reference(M, out_dim)
        for form, m_host, m_dev, stride in _size_forms(M):
            b = Buffers(dev, XM.exact_case(M, out_dim), stride, _feat_dtype(feat))
            ctx = "M=%d %s" % (M, form)
            dfeat, grads = b.backward(precision, m_host, m_dev)
            _check_backward(ctx, ref, M, dfeat, grads, failures)
            if precision == "bf16":
                ws = _workspace(dev, out_dim)
                b.forward(precision, m_host, m_dev, ws=ws)
                dfeat, grads = b.backward(precision, m_host, m_dev, ws=ws, flags=_B().MLP_FRAGMENTS_READY)
                _check_backward(ctx + " fragments ready", ref, M, dfeat, grads, failures)
    assert not failures, "\n".join(failures)


@PREC
@pytest.mark.parametrize("out_dim", XM.BIG_OUT_DIMS)
def test_backward_slab_reduction(dev, precision, out_dim):
    """M = 4229 (34 bf16 / 67 f32 tiles) with mlp_bwd_blocks 1, 3, 17, 512: lnerf_mlp_backward_slabs is min(blocks,
    tiles); persistent workgroups walk up to 67 tiles; with 17, 34 or 67 slabs the 16 lane groups of k_mlp_reduce_slabs
    sum unequal numbers of slabs.  Every setting equals the reference."""
    M = XM.M_SLABS
    ref = XM.exact_reference(M, out_dim)
    tiles = 34 if precision == "bf16" else 67
    failures = []
    b = Buffers(dev, XM.exact_case(M, out_dim), M + 7, _feat_dtype(precision))
    for blocks in (1, 3, 17, 512):
        with tuning(mlp_bwd_blocks=blocks):
            slabs = _B().get_lib().lnerf_mlp_backward_slabs(M + 7, _tag(precision))
            assert slabs == min(blocks, tiles), (blocks, slabs)
            dfeat, grads = b.backward(precision, M + 7, M)
        _check_backward("blocks=%d" % blocks, ref, M, dfeat, grads, failures)
    assert _B().get_lib().lnerf_mlp_backward_slabs(M + 7, _tag(precision)) == tiles      # the default is back
    assert not failures, "\n".join(failures)


@PREC
@pytest.mark.parametrize("out_dim", [2, 5, 8])
def test_backward_accumulates(dev, precision, out_dim):
    """accumulate != 0: result == pattern + reference; dw3 / db3 live in buffers of all 16 padded rows whose tail beyond
    out_dim holds a sentinel: nothing outside dw3[:out_dim] / db3[:out_dim] is written (accumulate 1 and 0)."""
    M = 300
    case, ref = XM.exact_case(M, out_dim), XM.exact_reference(M, out_dim)
    b = Buffers(dev, case, M + 7, _feat_dtype(precision))
    g = torch.Generator().manual_seed(5)
    failures = []
    for accumulate in (1, 7, 0):
        pattern = {k: torch.randint(-9, 10, case[k].shape, generator=g).float() for k in XM.W_NAMES}
        big = {"w3": torch.full((XM.MLP_OUTP, XM.MLP_HID), -77.0), "b3": torch.full((XM.MLP_OUTP,), -77.0)}
        for k in big:
            big[k][:out_dim] = pattern[k]
        held = {k: (big[k] if k in big else pattern[k]).clone().to(dev) for k in XM.W_NAMES}
        dfeat, _ = b.backward(precision, M + 7, M, accumulate=accumulate, grads=[held[k] for k in XM.W_NAMES])
        want = {k: (pattern[k].double() + ref[k]) if accumulate else ref[k] for k in XM.W_NAMES}
        got = [held[k][:out_dim] if k in big else held[k] for k in XM.W_NAMES]
        _check_backward("accumulate=%d" % accumulate, ref, M, dfeat, got, failures, want)
        for k in big:
            if not bool((held[k][out_dim:] == -77.0).all()):
                failures.append("accumulate=%d: d%s rows >= out_dim were written" % (accumulate, k))
    assert not failures, "\n".join(failures)


@PREC
def test_backward_clears_the_named_region(dev, precision):
    """clear_ptr / clear_bytes: a 4004-byte region between two sentinels is all zero afterwards, the sentinels are
    intact, the gradients are those of the call without a region."""
    M, out_dim = 300, 5
    ref = XM.exact_reference(M, out_dim)
    b = Buffers(dev, XM.exact_case(M, out_dim), M + 7, _feat_dtype(precision))
    buf = torch.full((64 + 4004 + 64,), 0xA5, device=dev, dtype=torch.uint8)
    dfeat, grads = b.backward(precision, M + 7, M, clear=buf[64:], clear_bytes=4004)
    failures = []
    _check_backward("with a clear region", ref, M, dfeat, grads, failures)
    assert not failures, "\n".join(failures)
    buf = buf.cpu()
    assert bool((buf[64:64 + 4004] == 0).all()), "byte %d of the region is not zero" % int(torch.nonzero(buf[64:4068])[0])
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + 4004:] == 0xA5).all()), "a sentinel was overwritten"


@PREC
@pytest.mark.parametrize("M,blocks", [(300, 512), (XM.M_SLABS, 17)])
def test_backward_deferred_reduce_slabs(dev, precision, M, blocks):
    """LNERF_MLP_DEFER_REDUCE with all six d* pointers NULL: the first lnerf_mlp_backward_slabs() slabs of the workspace
    (behind the fragment image), summed on the host in float64 through the layout restated in tests/exact_mlp.py, equal
    the reference; the padded rows of dW3 / db3 are zero; dfeat as ever."""
    out_dim = 5
    ref = XM.exact_reference(M, out_dim)
    b = Buffers(dev, XM.exact_case(M, out_dim), M + 7, _feat_dtype(precision))
    ws = _workspace(dev, out_dim)
    assert ws.numel() == XM.FRAGMENT_BYTES + XM.BWD_MAX_BLOCKS * XM.SLAB * 4
    with tuning(mlp_bwd_blocks=blocks):
        n = _B().get_lib().lnerf_mlp_backward_slabs(M + 7, _tag(precision))
        dfeat, _ = b.backward(precision, M + 7, M, ws=ws, flags=_B().MLP_DEFER_REDUCE, grads=[None] * 6)
    assert n == min(blocks, -(-(M + 7) // (128 if precision == "bf16" else 64)))
    slabs = ws[XM.FRAGMENT_BYTES:XM.FRAGMENT_BYTES + n * XM.SLAB * 4].view(torch.float32).reshape(n, XM.SLAB).cpu()
    sums = XM.slab_sums(slabs)
    failures = []
    _check_backward("deferred", ref, M, dfeat, None, failures)
    for k in XM.W_NAMES:
        want = ref[k]
        if k in ("w3", "b3"):
            want = torch.zeros((XM.MLP_OUTP,) + tuple(ref[k].shape[1:]), dtype=torch.float64)
            want[:out_dim] = ref[k]
        msg = XM.first_diff("slab sum d" + k, sums[k], want)
        if msg:
            failures.append(msg)
    # (the workspace was 0xFF bytes: beyond the slabs in use nothing was written)
    tail = ws[XM.FRAGMENT_BYTES + n * XM.SLAB * 4:]
    assert bool((tail == 0xFF).all()), "the workspace beyond %d slabs was written" % n
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------ stale rows and device counts
@PREC
@pytest.mark.parametrize("M", [1, 129])
def test_stale_rows_do_not_reach_any_result(dev, precision, M):
    """Buffers are capacity-sized and rows in [M, m_host) hold whatever the last step left: with NaN in rows >= M of
    feat, xyz, sigmas, dsigmas and drgbs (m_host = level_stride = M + 133, *m_dev = M) the forward outputs, dfeat and
    all six gradients are those of the clean run bit for bit -- and equal the reference."""
    out_dim, stride = 5, M + 133
    ref = XM.exact_reference(M, out_dim)
    failures = []
    for feat in ("f32", "bf16"):
        runs = {}
        for name, stale in (("clean", 0.0), ("stale", math.nan)):
            b = Buffers(dev, XM.exact_case(M, out_dim), stride, _feat_dtype(feat), stale)
            s, r = b.forward(precision, stride, M)
            dfeat, grads = b.backward(precision, stride, M)
            ctx = "feat=%s %s" % (feat, name)
            _check_forward(ctx, ref, M, s, r, precision, failures)
            _check_backward(ctx, ref, M, dfeat, grads, failures)
            runs[name] = [s, r, dfeat] + grads
        for what, a, c in zip(("sigmas", "rgbs", "dfeat") + tuple("d" + k for k in XM.W_NAMES), runs["stale"], runs["clean"]):
            msg = XM.first_diff(what + " (stale vs clean)", a, c)
            if msg:
                failures.append("feat=%s: %s" % (feat, msg))
    assert not failures, "\n".join(failures)


@PREC
def test_device_count_zero_and_beyond_m_host(dev, precision):
    """*m_dev = 0 (m_host = 129): forward outputs and dfeat keep FILL; the six gradients are exactly 0 with
    accumulate = 0 and unchanged with accumulate = 1.  *m_dev = m_host + 50: behaves as m_host."""
    M, out_dim = 129, 5
    case, ref = XM.exact_case(M, out_dim), XM.exact_reference(M, out_dim)
    b = Buffers(dev, case, M + 64, _feat_dtype(precision))
    s, r = b.forward(precision, M, 0)
    assert bool((s == FILL).all()) and bool((r == FILL).all()), "forward outputs written at *m_dev = 0"
    dfeat, grads = b.backward(precision, M, 0)
    assert bool((dfeat == FILL).all()), "dfeat written at *m_dev = 0"
    for k, g in zip(XM.W_NAMES, grads):
        assert XM.first_diff("d%s at *m_dev = 0" % k, g, torch.zeros_like(g)) is None, XM.first_diff("d" + k, g, torch.zeros_like(g))
    pattern = [torch.full_like(t, 3.0) for t in b.W]
    dfeat, grads = b.backward(precision, M, 0, accumulate=1, grads=[p.clone() for p in pattern])
    assert bool((dfeat == FILL).all())
    for k, g, p in zip(XM.W_NAMES, grads, pattern):
        assert torch.equal(g, p), XM.first_diff("d%s (accumulate, *m_dev = 0)" % k, g, p)
    failures = []
    s, r = b.forward(precision, M, M + 50)
    _check_forward("*m_dev = m_host + 50", ref, M, s, r, precision, failures)
    dfeat, grads = b.backward(precision, M, M + 50)
    _check_backward("*m_dev = m_host + 50", ref, M, dfeat, grads, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------ the trunc-exp clamp
@PREC
def test_trunc_exp_clamp(dev, precision):
    """d sigma / d pre-activation = min(sigma, exp(15)) on sigmas 2^22 (clamped), +inf (clamped) and 2^21 (kept), three
    live rows: db3[0] and dw3[0, :] are exact sums of dsigma * min(sigma, f32(exp(15))) over rows whose h2 is 0 or 1 (the
    bf16 path rounds that one factor to bf16, restated in XM.clamp_reference); everything is finite."""
    case = XM.clamp_case()
    M = case["M"]
    dw3_row, db3_0 = XM.clamp_reference(precision == "bf16")
    for feat in ("f32", "bf16"):
        b = Buffers(dev, case, M + 7, _feat_dtype(feat))
        dfeat, grads = b.backward(precision, M + 7, M)
        g = dict(zip(XM.W_NAMES, grads))
        assert XM.first_diff("dw3[0]", g["w3"][0], dw3_row) is None, XM.first_diff("dw3[0]", g["w3"][0], dw3_row)
        assert float(g["b3"][0]) == float(db3_0), "db3[0]: got %r want %r" % (float(g["b3"][0]), float(db3_0))
        for k in XM.W_NAMES:
            assert bool(torch.isfinite(g[k]).all()), "d%s is not finite" % k
        assert bool(torch.isfinite(dfeat[:, :M]).all()), "dfeat is not finite"


# ------------------------------------------------------------------------------ the fragment maps as a layout
@pytest.mark.parametrize("out_dim", [2, 5, 8])
def test_fragment_maps_invert_the_built_image(dev, out_dim):
    """lnerf_mlp_fragment_maps against the image lnerf_mlp_forward builds at the head of a workspace, on weights with
    pairwise distinct non-zero bf16 values within each tensor: image[map[2 i]] and image[map[2 i + 1]] hold bf16(w[i]),
    the first in the forward slots (< 14 * 512), the second in the transposed ones; all entries are distinct and inside
    the 30 weight slots; every element of those slots that no map names is 0."""
    g = torch.Generator().manual_seed(out_dim)
    shapes = {"w1": (XM.MLP_HID, XM.MLP_IN), "w2": (XM.MLP_HID, XM.MLP_HID), "w3": (out_dim, XM.MLP_HID)}
    case = dict(XM.exact_case(129, out_dim))
    bits = {}
    for k, shape in shapes.items():
        n = shape[0] * shape[1]
        # bit patterns 0x3000 + (a permutation of 0 .. n-1): distinct positive normal bf16 values below 2
        pat = (0x3000 + torch.randperm(n, generator=g)).to(torch.int16)
        bits[k] = pat
        case[k] = pat.view(torch.bfloat16).float().reshape(shape)
        assert len(set(pat.tolist())) == n and bool((case[k] > 0).all())
    b = Buffers(dev, case, 129 + 7, torch.bfloat16)
    ws = _workspace(dev, out_dim)
    b.forward("bf16", 129 + 7, 129, ws=ws)
    n_img = XM.F_ALL * XM.F_ELEMS
    image = ws[:2 * n_img].view(torch.int16).cpu()
    maps = {k: torch.full((2 * shapes[k][0] * shapes[k][1],), -7, dtype=torch.int32, device=dev) for k in shapes}
    _B().call("lnerf_mlp_fragment_maps", out_dim, _p(maps["w1"]), _p(maps["w2"]), _p(maps["w3"]), _stream())
    torch.cuda.synchronize()
    named = torch.zeros(n_img, dtype=torch.bool)
    for k in ("w1", "w2", "w3"):
        m = maps[k].cpu().long().reshape(-1, 2)
        fwd, tr = m[:, 0], m[:, 1]
        assert bool(((fwd >= 0) & (fwd < XM.F_FWD * XM.F_ELEMS)).all()), "%s: a forward entry outside the forward slots" % k
        assert bool(((tr >= XM.F_FWD * XM.F_ELEMS) & (tr < n_img)).all()), "%s: a transposed entry outside its slots" % k
        for name, idx in (("forward", fwd), ("transposed", tr)):
            bad = torch.nonzero(image[idx] != bits[k]).flatten()
            assert bad.numel() == 0, "%s[%d] (row %d, column %d): %s image[%d] holds bits %#x, want %#x" % (
                k, int(bad[0]), int(bad[0]) // shapes[k][1], int(bad[0]) % shapes[k][1], name, int(idx[bad[0]]),
                int(image[idx[bad[0]]]) & 0xFFFF, int(bits[k][bad[0]]) & 0xFFFF)
        assert not bool(named[m.flatten()].any()), "%s: an image element is named twice" % k
        assert len(set(m.flatten().tolist())) == m.numel(), "%s: an image element is named twice" % k
        named[m.flatten()] = True
    unnamed = torch.nonzero(~named).flatten()
    bad = unnamed[image[unnamed] != 0]
    assert unnamed.numel() > 0 and bad.numel() == 0, "image element %d (slot %d) is named by no map and holds %#x" % (
        int(bad[0]), int(bad[0]) // XM.F_ELEMS, int(image[bad[0]]) & 0xFFFF)


# ------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_alone(dev):
    """LNERF_ERR_INVALID_ARG before any launch: outputs pre-filled with FILL are untouched."""
    B = _B()
    lib = B.get_lib()
    M, stride = 129, 136
    b = Buffers(dev, XM.exact_case(M, 5), stride, torch.bfloat16)
    m_dev = b.m_dev(M)
    ws = _workspace(dev, 5)
    need = _ws_bytes(5)
    sigmas = torch.full((stride + 1,), FILL, device=dev)
    rgbs = torch.full((stride + 1, 4), FILL, device=dev)
    dfeat = torch.full((16, stride, 2), FILL, device=dev)
    grads = [torch.full_like(t, FILL) for t in b.W]
    clear = torch.full((16,), 0xA5, device=dev, dtype=torch.uint8)

    def fwd(tag=B.BF16, ws_=None, **kw):
        return lib.lnerf_mlp_forward(*b.forward_args(stride, m_dev, sigmas, rgbs, tag, ws_, **kw))

    def bwd(tag=B.BF16, **kw):
        return lib.lnerf_mlp_backward(*b.backward_args(stride, m_dev, dfeat, grads, 0, ws, tag, **kw))

    refused = {
        "forward out_dim 1": fwd(out_dim=1), "forward out_dim 9": fwd(out_dim=9),
        "backward out_dim 1": bwd(out_dim=1), "backward out_dim 9": bwd(out_dim=9),
        "forward level_stride < m_host": fwd(stride=stride - 1), "backward level_stride < m_host": bwd(stride=stride - 1),
        "forward FRAGMENTS_READY without a workspace": fwd(tag=B.BF16 | B.MLP_FRAGMENTS_READY),
        "backward DEFER_REDUCE with clear_bytes": bwd(tag=B.BF16 | B.MLP_DEFER_REDUCE, clear=clear, clear_bytes=16),
        "backward f32 DEFER_REDUCE with clear_bytes": bwd(tag=B.F32 | B.MLP_DEFER_REDUCE, clear=clear, clear_bytes=16),
        "backward workspace one byte short": bwd(ws_bytes=need - 1),
        "backward f32 workspace one byte short": bwd(tag=B.F32, ws_bytes=need - 1),
        "forward bf16 out_dim 5 rgbs off by 4 bytes": fwd(rgbs_offset=4),
        "backward bf16 out_dim 5 drgbs off by 4 bytes": bwd(drgbs_offset=4),
        "forward blob_std 0": fwd(blob_std=0.0), "backward blob_std 0": bwd(blob_std=0.0),
        "forward f32 blob_std 0": fwd(tag=B.F32, blob_std=0.0),
    }
    torch.cuda.synchronize()
    wrong = {k: rc for k, rc in refused.items() if rc != -1}        # LNERF_ERR_INVALID_ARG
    assert not wrong, wrong
    for name, t in [("sigmas", sigmas), ("rgbs", rgbs), ("dfeat", dfeat)] + [("d" + k, g) for k, g in zip(XM.W_NAMES, grads)]:
        assert bool((t == FILL).all()), "%s was written by a refused call" % name
    assert bool((clear == 0xA5).all()) and bool((ws == 0xFF).all())
    # the same arguments without the fault are accepted (the refusals above are the faults', not the harness's)
    assert fwd() == 0 and bwd() == 0
    assert fwd(tag=B.F32, rgbs_offset=4) == 0       # the alignment rule is the bf16 row store's alone
    torch.cuda.synchronize()


def test_measured_sigma_error(dev):
    """Prints the largest relative error of sigma the module saw (DESIGN.md quotes it); the bound is asserted per call."""
    assert set(_sigma_err) == set(PRECISIONS), "the forward tests did not run before this one"
    for precision, err in sorted(_sigma_err.items()):
        print("sigma, %s path: largest relative error %.4g = %.3f ulp (bound 4 ulp)" % (precision, err, err * 2.0 ** 23))
        assert err <= SIGMA_RTOL
