"""The exact-f32 MLP (csrc/mlp.hip) on ORDINARY inputs, bit for bit against tests/golden/mlp_f32_bits.npz.

The exact inputs of tests/test_gpu_mlp_exact.py have sums that are exact in any order, so a reordered fma chain or a
reordered bias / slab sum passes there.  Here the inputs are randn-like (tests/golden/make_mlp_f32_golden.py, which also
wrote the file, once, with the library of the commit named in it) and every stored tensor must be EQUAL: tolerance zero.
That is derived, not measured: a restructuring that keeps every MFMA chain's accumulator, k order and operands, the
order of the gb* sums and the wave order of the slab fold reorders no sum; the build has -ffp-contract=off; the slab
reduction is deterministic by construction.  A mismatch means an order changed: fix the kernel.

M = 150 of m_host = 157 (level_stride 160): two full 64-sample tiles, then wave 0 full, wave 1 with 6 samples, waves
2-3 empty; with mlp_bwd_blocks = 2 one workgroup walks tiles 0 and 2 and its accumulators carry across tiles.  Sigmas on
both sides of exp(15) are in every case (asserted here on the stored sigmas)."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from tests import exact_mlp as XM
from tests.test_gpu_tuning_paths import FILL, _restore_defaults

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location(
    "make_mlp_f32_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_mlp_f32_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(G.PATH) as f:
        return {k: f[k] for k in f.files}


@pytest.mark.parametrize("out_dim,feat,blocks", G.CASES, ids=[G.case_name(*c) for c in G.CASES])
def test_f32_mlp_equals_the_stored_bits(dev, golden, out_dim, feat, blocks):
    name = G.case_name(out_dim, feat, blocks)
    case = G.make_case(out_dim, feat)
    assert G.input_digest(case) == str(golden[name + "/input_sha256"]), \
        "%s: the regenerated INPUTS differ from the ones the file was written from (not a kernel fault)" % name
    from src.latent_nerf.raymarching import backend as B
    try:
        _, out = G.run_case(dev, out_dim, feat, blocks)
    finally:
        B.call("lnerf_set_tuning", b"mlp_bwd_blocks", G.BWD_BLOCKS_DEFAULT)
    assert B.get_lib().lnerf_mlp_backward_slabs(64 * 1000, B.F32) == G.BWD_BLOCKS_DEFAULT     # the default is back
    want_s = torch.from_numpy(golden[name + "/sigmas"])
    assert bool((want_s > math.exp(15.0)).any()) and bool((want_s < math.exp(15.0)).any())
    failures = []
    for k in G.OUTPUTS:
        got, want = G.valid_rows(k, out[k]), torch.from_numpy(golden[name + "/" + k])
        if not torch.equal(got, want):
            failures.append(XM.first_diff(k, got, want) or "%s: differs in shape or dtype" % k)
    for k in ("sigmas", "rgbs"):
        if not bool((out[k][G.M:] == FILL).all()):
            failures.append("%s: a row >= M = %d was written" % (k, G.M))
    if not bool((out["dfeat"][:, G.M:] == FILL).all()):
        failures.append("dfeat: a row >= M = %d was written" % G.M)
    assert not failures, "%s (file written by %s, %s):\n%s" % (
        name, str(golden["commit"]), str(golden["build_info"]), "\n".join(failures))
