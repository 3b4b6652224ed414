"""The one-step-ahead prefetch of the bf16 MLP kernels: rows that belong to the NEXT step of a persistent workgroup.

k_mlp_forward_bf16 and k_mlp_backward_bf16 request the inputs of their next 128-sample step -- features and positions,
features and the upstream gradient -- at the top of a step, from EVERY lane, with rows clamped into the valid samples, and
consume them a step later (csrc/mlp_bf16.hip; tests/test_mlp_isa_cpu.py reads the compiled loops).  What can go wrong
with that is a row: a prefetch that reads past min(m_host, *m_dev), a clamp that picks the wrong row, the validity of a
lane judged with the row base of the wrong step, a select applied to the values of the other step, a last (clamped)
prefetch that leaks into a result.  So every case here
  * runs with mlp_fwd_blocks / mlp_bwd_blocks = 1 and = 2 (lnerf_set_tuning; restored afterwards): a workgroup walks up
    to four steps and ends on a clamped prefetch;
  * has its count on the DEVICE, below m_host = level_stride = M + 133, and NaN in rows >= M of the features, the
    positions, sigmas, dsigmas and drgbs: one NaN that reaches an MFMA poisons a weight gradient;
  * pre-fills the outputs: rows >= M must keep the fill;
  * compares rows < M of the latents and of dfeat, and the six parameter gradients (written over NaN, and once more as
    the float64 sum of the slabs of a deferred reduction), BIT FOR BIT with the float64 exact-input reference of
    tests/exact_mlp.py -- never with a second run of the library.  sigma = expf(.) keeps that module's bound of 4 ulp
    against the float64 exp of the same argument: expf is not correctly rounded, and the argument itself is exact.
The positions are NOT those of XM.exact_case (0 on even rows, 100 on odd ones: a period that the 16-row tiles and the
128-row steps preserve, so that the blob of the wrong tile or the wrong step would be the right one): every row draws at
random whether it lies at the origin (blob exactly 2) or 100 away along a random axis (blob exactly 0), which keeps the
argument of expf exact and makes a blob taken from another row wrong by a factor e^2 on every second row.  The reference
of such a case is XM.reference() of the local copy.
M in {1, 16, 17, 127, 128, 129, 3 * 128 + 5}: one lane, one 16-sample tile and one lane of the next, the step edge, four
steps with a ragged last one.  out_dim 5 (the raw 16-byte upstream row, the row store) and 4 (the generic arms); bf16
and f32 features (raw words / converted where they are loaded)."""
import functools
import math

import pytest
import torch

from tests import exact_mlp as XM
from tests.test_gpu_mlp_exact import Buffers, _B, _check_backward, _check_forward, _workspace
from tests.test_gpu_tuning_paths import FILL, _restore_defaults, tuning

pytestmark = pytest.mark.gpu

SIZES = (1, 16, 17, 127, 128, 129, 3 * 128 + 5)
BLOCKS = (1, 2)
EXTRA = 133                    # rows of NaN behind the valid ones: more than one whole step


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    _B().get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case_and_reference(M, out_dim):
    """XM.exact_case with row-random positions (a copy: the cached case is not touched) and its float64 reference."""
    case = dict(XM.exact_case(M, out_dim))
    g = torch.Generator().manual_seed(977 * M + out_dim)
    far = torch.randint(0, 2, (M,), generator=g).float()
    axis = torch.randint(0, 3, (M,), generator=g)
    xyz = torch.zeros(M, 3)
    xyz[torch.arange(M), axis] = 100.0 * far
    case["xyz"] = xyz
    return case, XM.reference(case)


def _feat_dtype(feat):
    return torch.float32 if feat == "f32" else torch.bfloat16


def _deferred_slab_sums(b, m_host, m_dev):
    """dfeat and the float64 sums of the slabs of a backward with LNERF_MLP_DEFER_REDUCE (all 16 padded rows of dW3 / db3)."""
    ws = _workspace(b.dev, b.out_dim)
    n = _B().get_lib().lnerf_mlp_backward_slabs(m_host, _B().BF16)
    dfeat, _ = b.backward("bf16", m_host, m_dev, ws=ws, flags=_B().MLP_DEFER_REDUCE, grads=[None] * 6)
    slabs = ws[XM.FRAGMENT_BYTES:XM.FRAGMENT_BYTES + n * XM.SLAB * 4].view(torch.float32).reshape(n, XM.SLAB).cpu()
    tail = ws[XM.FRAGMENT_BYTES + n * XM.SLAB * 4:]
    return dfeat, XM.slab_sums(slabs), n, bool((tail == 0xFF).all())


def _padded_rows(ref, k, out_dim):
    if k not in ("w3", "b3"):
        return ref[k]
    want = torch.zeros((XM.MLP_OUTP,) + tuple(ref[k].shape[1:]), dtype=torch.float64)
    want[:out_dim] = ref[k]
    return want


@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("feat", ["bf16", "f32"])
def test_next_step_rows(dev, feat, out_dim):
    """Every M of SIZES with one and with two persistent workgroups, forward and backward."""
    failures = []
    for M in SIZES:
        case, ref = _case_and_reference(M, out_dim)
        stride = M + EXTRA
        b = Buffers(dev, case, stride, _feat_dtype(feat), math.nan)
        steps = -(-stride // 128)
        for blocks in BLOCKS:
            ctx = "M=%d blocks=%d" % (M, blocks)
            with tuning(mlp_fwd_blocks=blocks, mlp_bwd_blocks=blocks):
                s, r = b.forward("bf16", stride, M)
                dfeat, grads = b.backward("bf16", stride, M)
                dfeat_d, sums, n, tail_clean = _deferred_slab_sums(b, stride, M)
            _check_forward(ctx, ref, M, s, r, "bf16", failures)
            _check_backward(ctx, ref, M, dfeat, grads, failures)
            _check_backward(ctx + " deferred", ref, M, dfeat_d, None, failures)
            if n != min(blocks, steps):
                failures.append("%s: %d slabs, want %d" % (ctx, n, min(blocks, steps)))
            if not tail_clean:
                failures.append("%s: the workspace beyond %d slabs was written" % (ctx, n))
            for k in XM.W_NAMES:
                msg = XM.first_diff("slab sum d" + k, sums[k], _padded_rows(ref, k, out_dim))
                if msg:
                    failures.append("%s: %s" % (ctx, msg))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("feat", ["bf16", "f32"])
def test_device_count_zero(dev, feat, out_dim):
    """*m_dev = 0 with m_host = 128 and NaN in EVERY row of every input: the first prefetch is a clamped one (row 0).  No
    output row is written; the six gradients are exactly zero (the reference of an empty case)."""
    case, ref = XM.exact_case(0, out_dim), XM.exact_reference(0, out_dim)
    failures = []
    b = Buffers(dev, case, 128, _feat_dtype(feat), math.nan)
    for blocks in BLOCKS:
        ctx = "blocks=%d" % blocks
        with tuning(mlp_fwd_blocks=blocks, mlp_bwd_blocks=blocks):
            s, r = b.forward("bf16", 128, 0)
            dfeat, grads = b.backward("bf16", 128, 0)
        _check_backward(ctx, ref, 0, dfeat, grads, failures)
        for name, t in (("sigmas", s), ("rgbs", r), ("dfeat", dfeat)):
            if not bool((t == FILL).all()):
                failures.append("%s: %s was written at *m_dev = 0" % (ctx, name))
    assert not failures, "\n".join(failures)


def test_tuning_is_restored(dev):
    """The persistent grid sizes are the defaults again: M = 700 needs 6 slabs."""
    assert _B().get_lib().lnerf_mlp_backward_slabs(XM.M_PERSISTENT, _B().BF16) == 6
