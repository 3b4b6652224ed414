"""The prologue of the bf16 MLP kernels: weight fragments requested, then the first step's inputs, then the LDS writes.

k_mlp_forward_bf16 and k_mlp_backward_bf16 (csrc/mlp_bf16.hip) load the launch's cached weight fragments into registers,
request the inputs of the workgroup's FIRST step behind them as soon as min(m_host, *m_dev) is known, and only then write
fragments and biases to LDS (tests/test_mlp_prologue_isa_cpu.py reads the compiled order).  What can go wrong with that:
a fragment word written to the wrong place or left out at the ragged end of the copy (14 and 30 KiB over 256 threads: the
last round is half a workgroup), a bias taken from the wrapped index, a first-step row that is not clamped -- above all in
a workgroup WITHOUT a tile, whose first request is all there is --, and an input that the fragment copy overtakes.  So
every case here
  * runs with mlp_fwd_blocks = mlp_bwd_blocks = 2, 3 and 4 (lnerf_set_tuning; restored afterwards), so that these edges
    appear at a few hundred samples;
  * has its count on the DEVICE, below m_host = level_stride = M + 133, and NaN in rows >= M of the features, the
    positions, sigmas, dsigmas and drgbs (as tests/test_gpu_mlp_prefetch.py): the grid is sized by m_host, so that small M
    leave workgroups without a tile, and one NaN that reaches an MFMA poisons a weight gradient;
  * takes the forward with the cached fragments (a workspace) AND without (every workgroup builds its own: the arm that
    was kept as it is); the backward always has the cache;
  * compares with the float64 exact-input reference of tests/test_gpu_mlp_prefetch.py at its tolerance -- bit for bit,
    sigma = expf(.) within 4 ulp -- and runs everything twice: the two runs must be bit-identical.
M in {1, 31, 32, 33, 127, 128, 129} and 128 * blocks - 1, 128 * blocks + 1 (the last workgroup's first step holds one
row short of a full step / the first workgroup's second step one row, every other prefetch of it clamped); bf16 features;
out_dim 5 (the raw 16-byte rows) and 4 (the generic arms)."""
import math

import pytest
import torch

from tests import exact_mlp as XM
from tests.test_gpu_mlp_exact import Buffers, _B, _check_backward, _check_forward, _workspace
from tests.test_gpu_mlp_prefetch import EXTRA, _case_and_reference
from tests.test_gpu_tuning_paths import _restore_defaults, tuning

pytestmark = pytest.mark.gpu

BLOCKS = (2, 3, 4)
SMALL = (1, 31, 32, 33, 127, 128, 129)


def _sizes(blocks):
    return SMALL + (128 * blocks - 1, 128 * blocks + 1)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    _B().get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


def _same(ctx, what, a, b, failures):
    """Bit equality of two runs (NaN-free by the first run's comparison with the reference, fills included)."""
    if not torch.equal(a, b):
        failures.append("%s: %s differs between two runs" % (ctx, what))


@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("blocks", BLOCKS)
def test_forward_prologue(dev, blocks, out_dim):
    failures = []
    for M in _sizes(blocks):
        case, ref = _case_and_reference(M, out_dim)
        stride = M + EXTRA
        b = Buffers(dev, case, stride, torch.bfloat16, math.nan)
        with tuning(mlp_fwd_blocks=blocks):
            for form in ("cached", "built"):
                ctx = "M=%d blocks=%d fragments %s" % (M, blocks, form)
                runs = [b.forward("bf16", stride, M, ws=_workspace(dev, out_dim) if form == "cached" else None)
                        for _ in range(2)]
                _check_forward(ctx, ref, M, runs[0][0], runs[0][1], "bf16", failures)
                _same(ctx, "sigmas", runs[0][0], runs[1][0], failures)
                _same(ctx, "rgbs", runs[0][1], runs[1][1], failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("blocks", BLOCKS)
def test_backward_prologue(dev, blocks, out_dim):
    failures = []
    for M in _sizes(blocks):
        case, ref = _case_and_reference(M, out_dim)
        stride = M + EXTRA
        b = Buffers(dev, case, stride, torch.bfloat16, math.nan)
        ctx = "M=%d blocks=%d" % (M, blocks)
        with tuning(mlp_bwd_blocks=blocks):
            runs = [b.backward("bf16", stride, M) for _ in range(2)]
        _check_backward(ctx, ref, M, runs[0][0], runs[0][1], failures)
        _same(ctx, "dfeat", runs[0][0], runs[1][0], failures)
        for k, g0, g1 in zip(XM.W_NAMES, runs[0][1], runs[1][1]):
            _same(ctx, "d" + k, g0, g1, failures)
    assert not failures, "\n".join(failures)


def test_tuning_is_restored(dev):
    """The persistent grid sizes are the defaults again: M = 700 needs 6 slabs."""
    assert _B().get_lib().lnerf_mlp_backward_slabs(XM.M_PERSISTENT, _B().BF16) == 6
