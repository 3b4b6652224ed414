"""Freeze what the exact-f32 MLP (csrc/mlp.hip) computes on ORDINARY inputs, bit for bit, so that a restructuring of its
kernels which reorders one fma chain or one sum no longer goes unnoticed (tests/test_gpu_mlp_f32_bits.py).

    LNERF_HIP_LIB=<library built from the commit to pin> python tests/golden/make_mlp_f32_golden.py --commit <its id>

Run once, on the GPU, against the library of the commit whose results are to be kept; rewrites
tests/golden/mlp_f32_bits.npz.  Only the C ABI is used (lnerf_mlp_forward, lnerf_mlp_backward, lnerf_set_tuning), so
the same script runs against any build.  The exact inputs of tests/exact_mlp.py cannot see a reordered chain -- their
sums are exact in any order; these can: weights and biases randn at the initialiser's scale (1 / sqrt(fan in)), features
randn (rounded to bf16 where the features are bf16), positions uniform in the box under a blob of scale 5, std 0.2,
upstream gradients randn with about a quarter exact zeros.

M = 150 valid rows of m_host = 157 (level_stride 160): two full 64-sample tiles and a third whose wave 0 is full, wave 1
holds 6 samples and waves 2-3 hold none.  With mlp_bwd_blocks = 2 one workgroup walks tiles 0 and 2: its accumulators
carry across tiles.  b3[0] is shifted by B3_SHIFT so that the sigmas straddle exp(15) in every case: both arms of the
trunc-exp clamp are in the file, which main() asserts.

Per case the file holds sigmas, rgbs, dfeat (rows < M) and the six parameter gradients, and a SHA-256 of the input
bytes: the test regenerates the inputs from the seed and reports a drift of the INPUTS as such."""
import argparse
import hashlib
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from tests import exact_mlp as XM  # noqa: E402

PATH = os.path.join(HERE, "mlp_f32_bits.npz")
M, M_HOST, STRIDE = 150, 157, 160
BLOB_SCALE, BLOB_STD = 5.0, 0.2
BWD_BLOCKS_DEFAULT = 512
# (out_dim, feature type, mlp_bwd_blocks or None for the default)
CASES = ((5, "f32", None), (5, "bf16", 2), (2, "f32", 2), (8, "bf16", None))
B3_SHIFT = 15.0     # added to b3[0]: the pre-activations of sigma then span about 13.3 .. 18.6 over the four cases
OUTPUTS = ("sigmas", "rgbs", "dfeat") + tuple("d" + k for k in XM.W_NAMES)
INPUTS = ("x", "xyz") + XM.W_NAMES + ("dsigmas", "drgbs")


def case_name(out_dim, feat, blocks):
    return "out%d_%s_%s" % (out_dim, feat, "default" if blocks is None else "blocks%d" % blocks)


def make_case(out_dim, feat):
    """The inputs of one case, f32 CPU tensors from a seeded CPU generator (elementwise operations only: the same bits
    on every machine)."""
    g = torch.Generator().manual_seed(20261021 + 16 * out_dim + (feat == "bf16"))

    def randn(*shape):
        return torch.randn(*shape, generator=g)

    def sparse(*shape):
        v = randn(*shape)
        v[torch.rand(*shape, generator=g) < 0.25] = 0.0
        return v

    c = dict(M=M, out_dim=out_dim)
    x = randn(M, XM.MLP_IN)
    c["x"] = x.to(torch.bfloat16).float() if feat == "bf16" else x
    c["xyz"] = torch.rand(M, 3, generator=g) * 2.0 - 1.0
    for w, b, n_out, n_in in (("w1", "b1", XM.MLP_HID, XM.MLP_IN), ("w2", "b2", XM.MLP_HID, XM.MLP_HID),
                              ("w3", "b3", out_dim, XM.MLP_HID)):
        c[w], c[b] = randn(n_out, n_in) / math.sqrt(n_in), randn(n_out) / math.sqrt(n_in)
    c["b3"][0] += B3_SHIFT
    c["dsigmas"], c["drgbs"] = sparse(M), sparse(M, out_dim - 1)
    c["sigmas"] = torch.zeros(M)        # (the backward is handed the forward's own output: run_case)
    return c


def input_digest(case):
    h = hashlib.sha256()
    for k in INPUTS:
        t = case[k].contiguous()
        assert t.dtype == torch.float32
        h.update(k.encode() + bytes(str(tuple(t.shape)), "ascii") + t.numpy().tobytes())
    return h.hexdigest()


def run_case(dev, out_dim, feat, blocks):
    """-> (the case, name -> CPU tensor of every output at FULL capacity: rows >= M of sigmas, rgbs and dfeat keep the
    pre-fill).  Forward, then the backward on the forward's sigmas, precision f32; mlp_bwd_blocks is back at its
    default afterwards whatever happens."""
    from src.latent_nerf.raymarching import backend as B
    from tests.test_gpu_mlp_exact import Buffers
    case = make_case(out_dim, feat)
    b = Buffers(dev, case, STRIDE, torch.float32 if feat == "f32" else torch.bfloat16)
    b.blob_scale = BLOB_SCALE
    assert XM.BLOB_STD == BLOB_STD
    try:
        if blocks is not None:
            B.call("lnerf_set_tuning", b"mlp_bwd_blocks", blocks)
        sigmas, rgbs = b.forward("f32", M_HOST, M)
        b.sigmas = sigmas
        dfeat, grads = b.backward("f32", M_HOST, M)
        torch.cuda.synchronize()
    finally:
        B.call("lnerf_set_tuning", b"mlp_bwd_blocks", BWD_BLOCKS_DEFAULT)
    out = dict(sigmas=sigmas.cpu(), rgbs=rgbs.cpu(), dfeat=dfeat.cpu())
    out.update({"d" + k: g.cpu() for k, g in zip(XM.W_NAMES, grads)})
    return case, out


def valid_rows(name, t):
    """The part of an output the file keeps: rows < M of the per-sample ones (dfeat sample-major), the gradients whole."""
    if name == "dfeat":
        return XM.sample_major(t, M).contiguous()
    return t[:M] if name in ("sigmas", "rgbs") else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="id of the commit the loaded library was built from")
    ap.add_argument("--out", default=PATH)
    args = ap.parse_args()
    from src.latent_nerf.raymarching import backend as B
    assert torch.cuda.is_available(), "the golden file is written on the GPU"
    dev = torch.device("cuda:0")
    store = {"build_info": np.array(B.get_lib().lnerf_build_info().decode()), "commit": np.array(args.commit)}
    e15 = math.exp(15.0)
    for out_dim, feat, blocks in CASES:
        name = case_name(out_dim, feat, blocks)
        case, out = run_case(dev, out_dim, feat, blocks)
        s = out["sigmas"][:M]
        above, below = int((s > e15).sum()), int((s < e15).sum())
        print("%s: %d sigmas above exp(15), %d below; all finite: %s" % (
            name, above, below, all(bool(torch.isfinite(valid_rows(k, out[k])).all()) for k in OUTPUTS)))
        assert above >= 1 and below >= 1, "both arms of the trunc-exp clamp must be in the file: adjust B3_SHIFT"
        store[name + "/input_sha256"] = np.array(input_digest(case))
        for k in OUTPUTS:
            store[name + "/" + k] = valid_rows(k, out[k]).numpy()
    np.savez(args.out, **store)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
