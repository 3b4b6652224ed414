"""Shared inputs of tests/test_gpu_mlp_exact.py and tests/test_mlp_exact_inputs_cpu.py.

exact_case()      EXACT-ARITHMETIC inputs of the fused sigma/latent MLP (32 -> 64 -> 64 -> out_dim): small integers, so
                  that every MFMA operand of BOTH precisions -- features, weights, hidden activations, the three
                  pre-activation gradients -- is a bf16 value, and every dot product and every sum over samples is an
                  integer (an eighth, in the sigma row) below 2^24: exact in f32 in ANY order of addition.  A kernel must
                  then equal a plain float64 evaluation BIT FOR BIT -- no rounding model, no tolerance for a wrongly
                  masked pair, a swapped fragment, a tile owned by the wrong wave or a slab left out to hide in.  Only
                  sigma = expf(.) keeps a bound.  Why it is exact:
                    * x, w1, w2, w3[1:], dsigmas, drgbs in {-1, 0, 1}; biases in {-2 .. 2};
                    * w3[0] (the sigma row) in {-1, 0, 1} / 8: |h0| stays small enough for expf;
                    * the sigmas HANDED TO THE BACKWARD are in {8, 16} (an input of lnerf_mlp_backward, independent of
                      the forward's output): dsigma * sigma * w3[0][.] is an integer;
                    * xyz alternates between 0 and (100, 0, 0): with blob_scale 2, blob_std 0.2 the density blob is
                      exactly 2 (expf(-0) = 1) or exactly 0 (expf(-125000) underflows), so h0 + blob is exact.
                  tests/test_mlp_exact_inputs_cpu.py asserts these properties on every case the GPU module uses.
reference()       float64, plain matmuls, relu and masks; NO bf16 rounding anywhere.
clamp_case()      the trunc-exp clamp: three live rows with sigmas 2^22, +inf, 2^21 handed to the backward.
The references are computed once per process and must not be modified by a test."""
import functools
import itertools
import math

import torch

BLOB_SCALE, BLOB_STD = 2.0, 0.2
W_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")

# ---- restated from csrc/mlp_shared.h / csrc/mlp_bf16.hip (tests/test_mlp_exact_inputs_cpu.py parses the sources)
MLP_IN, MLP_HID, MLP_OUTP = 32, 64, 16
# one gradient slab, in floats: dW1 [64*32] | db1 [64] | dW2 [64*64] | db2 [64] | dW3 [16*64] | db3 [16]
SL_W1, SL_B1, SL_W2, SL_B2, SL_W3, SL_B3, SLAB = 0, 2048, 2112, 6208, 6272, 7296, 7312
BWD_MAX_BLOCKS = 512
FRAGMENT_BYTES = 36 * 1024          # the bf16 weight-fragment image at the head of the workspace; the slabs follow it
F_FWD, F_ALL, F_ELEMS = 14, 30, 512  # forward fragment slots, all weight-fragment slots, bf16 elements per slot

# ---- the shapes of the GPU module: the tile edges are 64 (f32) and 128 (bf16, forward and backward)
SMALL_M = (1, 127, 128, 129, 300)
OUT_DIMS = (2, 4, 5, 8)
M_PERSISTENT = 700                  # 6 bf16 tiles: persistent loops with their one-step prefetch
M_SLABS = 4229                      # 34 bf16 / 67 f32 tiles: more than 16 slabs, unequal numbers per lane group
BIG_OUT_DIMS = (5, 8)               # the out_dim values used at M_PERSISTENT and M_SLABS
CASES = tuple(itertools.product(SMALL_M, OUT_DIMS)) + tuple(
    itertools.product((M_PERSISTENT, M_SLABS), BIG_OUT_DIMS))


@functools.lru_cache(maxsize=None)
def exact_case(M, out_dim, seed=0):
    """dict of f32 CPU tensors: x [M, 32] (column 2 l + f), xyz [M, 3], w1 .. b3, dsigmas [M], drgbs [M, out_dim - 1],
    sigmas [M] (the values handed to the backward)."""
    g = torch.Generator().manual_seed(1000003 * seed + 131 * M + out_dim)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).float()

    c = dict(M=M, out_dim=out_dim, seed=seed)
    c["x"] = ints(-1, 1, M, MLP_IN)
    c["w1"], c["b1"] = ints(-1, 1, MLP_HID, MLP_IN), ints(-2, 2, MLP_HID)
    c["w2"], c["b2"] = ints(-1, 1, MLP_HID, MLP_HID), ints(-2, 2, MLP_HID)
    w3 = ints(-1, 1, out_dim, MLP_HID)
    w3[0] /= 8.0
    c["w3"], c["b3"] = w3, ints(-2, 2, out_dim)
    c["dsigmas"], c["drgbs"] = ints(-1, 1, M), ints(-1, 1, M, out_dim - 1)
    c["sigmas"] = 8.0 * (1.0 + ints(0, 1, M))
    xyz = torch.zeros(M, 3)
    xyz[1::2, 0] = 100.0
    c["xyz"] = xyz
    return c


def reference(case, e15=math.exp(15.0)):
    """The float64 evaluation: dict(z1, z2 (hidden pre-activations), h1, h2, h [M, out_dim] (output pre-activations,
    blob not added), blob, sigma = exp(h0 + blob), dz3, dz2, dz1, dfeat [M, 32], w1 .. b3 (the six gradients)).
    dZ3[:, 0] = dsigma * min(sigma_given, e15)."""
    d = {k: v.double() for k, v in case.items() if isinstance(v, torch.Tensor)}
    z1 = d["x"] @ d["w1"].t() + d["b1"]
    h1 = z1.clamp(min=0.0)
    z2 = h1 @ d["w2"].t() + d["b2"]
    h2 = z2.clamp(min=0.0)
    h = h2 @ d["w3"].t() + d["b3"]
    blob = BLOB_SCALE * torch.exp(-(d["xyz"] ** 2).sum(-1) / (2.0 * BLOB_STD * BLOB_STD))
    dz3 = torch.cat([(d["dsigmas"] * d["sigmas"].clamp(max=e15))[:, None], d["drgbs"]], 1)
    dz2 = (dz3 @ d["w3"]) * (z2 > 0)
    dz1 = (dz2 @ d["w2"]) * (z1 > 0)
    return dict(z1=z1, z2=z2, h1=h1, h2=h2, h=h, blob=blob, sigma=torch.exp(h[:, 0] + blob), dz3=dz3, dz2=dz2, dz1=dz1,
                dfeat=dz1 @ d["w1"], w1=dz1.t() @ d["x"], b1=dz1.sum(0), w2=dz2.t() @ h1, b2=dz2.sum(0),
                w3=dz3.t() @ h2, b3=dz3.sum(0))


@functools.lru_cache(maxsize=None)
def exact_reference(M, out_dim, seed=0):
    return reference(exact_case(M, out_dim, seed))


def abs_term_sums(case, ref):
    """name -> the largest sum of ABSOLUTE terms of any dot product / sample sum of the forward and the backward: below
    2^24 (times the unit, 1/8 in the sigma row) every partial sum, in any order, is exact in f32."""
    d = {k: v.double().abs() for k, v in case.items() if isinstance(v, torch.Tensor)}
    r = {k: v.abs() for k, v in ref.items()}
    out = {
        "z1": d["x"] @ d["w1"].t() + d["b1"], "z2": r["h1"] @ d["w2"].t() + d["b2"],
        "h": r["h2"] @ d["w3"].t() + d["b3"], "dA2": r["dz3"] @ d["w3"], "dA1": r["dz2"] @ d["w2"],
        "dfeat": r["dz1"] @ d["w1"], "dw1": r["dz1"].t() @ d["x"], "db1": r["dz1"].sum(0),
        "dw2": r["dz2"].t() @ r["h1"], "db2": r["dz2"].sum(0), "dw3": r["dz3"].t() @ r["h2"], "db3": r["dz3"].sum(0),
    }
    return {k: float(v.max()) for k, v in out.items()}


# ---- the trunc-exp clamp
E15_F32 = float(torch.tensor(math.exp(15.0), dtype=torch.float32))           # 3269017.25: what both kernels clamp at
E15_BF16 = float(torch.tensor(E15_F32).to(torch.bfloat16))                   # 3276800: the bf16 path's dZ3 operand
CLAMP_ROWS = (5, 70, 128)            # a row of the first and of the second f32 tile, and the lone row of the third tile
CLAMP_SIGMAS = (2.0 ** 22, math.inf, 2.0 ** 21)
CLAMP_DSIGMAS = (1.0, 1.0, -1.0)


@functools.lru_cache(maxsize=None)
def clamp_case():
    """129 rows, out_dim 5; only CLAMP_ROWS have an upstream gradient: dsigma = +1, +1, -1, drgbs = 0, given sigmas 2^22
    (above e15 = 3269017.25: clamped), +inf (clamped), 2^21 (below: kept).  dW3[0, j] = sum over the rows of
    dsigma * min(sigma, e15) * h2[row, j], and db3[0] (h2 -> 1), must be exact in f32 IN ANY ORDER although
    e15 = 13076069 / 4 needs all 24 bits: the hidden layers of this case are selections (one +-1 per row of w1 and w2,
    biases 0), so h2 is 0 or 1, and with the signs above every sum over a subset of the three rows' factors
    (e15, e15, -2^21) is an f32 value (asserted on the CPU)."""
    g = torch.Generator().manual_seed(77)
    M, out_dim = 129, 5
    c = dict(M=M, out_dim=out_dim, seed=-1)
    c["x"] = torch.randint(-1, 2, (M, MLP_IN), generator=g).float()
    for name, n_out, n_in in (("w1", MLP_HID, MLP_IN), ("w2", MLP_HID, MLP_HID)):
        w = torch.zeros(n_out, n_in)
        col = torch.randint(0, n_in, (n_out,), generator=g)
        w[torch.arange(n_out), col] = (torch.randint(0, 2, (n_out,), generator=g) * 2 - 1).float()
        c[name] = w
    c["b1"], c["b2"] = torch.zeros(MLP_HID), torch.zeros(MLP_HID)
    w3 = torch.randint(-1, 2, (out_dim, MLP_HID), generator=g).float()
    w3[0] /= 8.0
    c["w3"], c["b3"] = w3, torch.randint(-2, 3, (out_dim,), generator=g).float()
    c["dsigmas"], c["drgbs"] = torch.zeros(M), torch.zeros(M, out_dim - 1)
    c["sigmas"] = 8.0 * (1.0 + torch.randint(0, 2, (M,), generator=g).float())
    rows = list(CLAMP_ROWS)
    c["dsigmas"][rows] = torch.tensor(CLAMP_DSIGMAS)
    c["sigmas"][rows] = torch.tensor(CLAMP_SIGMAS)
    xyz = torch.zeros(M, 3)
    xyz[1::2, 0] = 100.0
    c["xyz"] = xyz
    return c


def clamp_reference(bf16):
    """(dw3_row0 [64], db3_0) in float64.  The bf16 path rounds the factor min(sigma, e15) to bf16 when it packs dZ3: the
    single rounding restated here."""
    c = clamp_case()
    ref = reference(c)
    rows = list(CLAMP_ROWS)
    factor = torch.tensor(CLAMP_SIGMAS, dtype=torch.float32).clamp(max=E15_F32)
    if bf16:
        factor = factor.to(torch.bfloat16)
    dz = torch.tensor(CLAMP_DSIGMAS, dtype=torch.float64) * factor.double()
    return dz @ ref["h2"][rows], dz.sum()


# ---- layouts and reports
def level_major(x, stride, fill=0.0, dtype=torch.float32):
    """[M, 32] sample-major -> [16, stride, 2] level-major, rows >= M holding `fill`."""
    M = x.shape[0]
    out = torch.full((16, stride, 2), fill, dtype=torch.float32)
    out[:, :M] = x.reshape(M, 16, 2).permute(1, 0, 2)
    return out.to(dtype)


def sample_major(feat, M):
    """[16, stride, 2] -> [M, 32]."""
    return feat[:, :M].permute(1, 0, 2).reshape(M, 32)


def padded(t, stride, fill=0.0):
    """[M, ...] -> [stride, ...], rows >= M holding `fill`."""
    out = torch.full((stride,) + tuple(t.shape[1:]), fill, dtype=t.dtype)
    out[:t.shape[0]] = t
    return out


def slab_sums(slabs):
    """f32 [n, SLAB] -> name -> float64 sum over the slabs, through the restated layout (dW3 / db3: all 16 padded rows)."""
    s = slabs.double().sum(0)
    assert s.numel() == SLAB
    return {"w1": s[SL_W1:SL_B1].reshape(MLP_HID, MLP_IN), "b1": s[SL_B1:SL_W2],
            "w2": s[SL_W2:SL_B2].reshape(MLP_HID, MLP_HID), "b2": s[SL_B2:SL_W3],
            "w3": s[SL_W3:SL_B3].reshape(MLP_OUTP, MLP_HID), "b3": s[SL_B3:SLAB]}


def first_diff(name, got, want):
    """None when `got` equals `want` bit for bit as numbers (float64 `want` included); else a message naming the first
    differing element: tensor, index (row, column), got, want, and how many differ."""
    got, want = got.detach().cpu(), want.detach().cpu()
    if tuple(got.shape) != tuple(want.shape):
        return "%s: shape %s, want %s" % (name, tuple(got.shape), tuple(want.shape))
    g, w = got.double(), want.double()
    bad = ~((g == w) | (torch.isnan(g) & torch.isnan(w)))
    if not bool(bad.any()):
        return None
    idx = torch.nonzero(bad)
    i = tuple(idx[0].tolist())
    return "%s%s: got %r want %r (%d of %d elements differ; rows %s)" % (
        name, list(i), float(g[i]), float(w[i]), idx.shape[0], bad.numel(), sorted(set(idx[:, 0].tolist()))[:8])
