"""Shared inputs of tests/test_gpu_tuning_paths.py and tests/test_tuning_inputs_cpu.py.

TUNING_DEFAULTS   the one table of lnerf_set_tuning defaults (checked against the C sources on the CPU).
exact_case()      EXACT-ARITHMETIC inputs of the hash grid: a hand-set level table, lattice positions, small-integer
                  values.  Every product and every sum of the gather, the scatter (float atomics, 12- and 8-byte records,
                  merged runs, fixed-point tiles, sliced buckets) and the position gradient is exact in f32, so a kernel
                  must equal the float64 oracle BIT FOR BIT: one wrong lane is a nonzero integer multiple of 2^-12, with
                  no tolerance to hide in.  Why it is exact:
                    * scale 32, bound 1, x = J / 128 - 1 with integer J: pos = J / 8 + 0.5, fractions are multiples of
                      1/8, corner weights multiples of 1/512 (<= 1);
                    * table values k / 8 with |k| <= 32 (exact in bf16 too): a feature is a multiple of 2^-12 below 4;
                    * gradients are integers in [-3, 3]: a record w * g is a multiple of 1/512 below 3, the sum over a
                      run of <= 64 lanes stays below 2^17 / 512 (the 18 significant bits of an 8-byte record hold it),
                      a table row's sum below 2^24 / 512 (f32 holds it, in any order of addition).
ordinary_case()   ordinary inputs (random table, samples ordered along rays, random gradients with zero tails) on the
                  standard 16-level table at the small configuration.
The references are computed once per process and must not be modified by a test."""
import ctypes
import functools

import torch

from oracle import nerf_oracle as O

TUNING_DEFAULTS = {
    "scatter_compact_max_res": 512,
    "scatter_bin_per_cu": 3,
    "scatter_bin_wgs": 0,
    "scatter_skip_zero": 1,
    "scatter_reduce_threads": 1024,
    "scatter_level_groups": 1,
    "gather_pair_loads": 2,
    "gather_dedup_max_res": 512,
    "gather_lds_pad": 0,
    "mlp_fwd_blocks": 768,
    "mlp_fwd_wps": 3,
    "mlp_bwd_blocks": 512,
}

# key -> values one step outside its documented range (include/lnerf_hip.h); scatter_skip_zero is a flag: any value
TUNING_REFUSED = {
    "scatter_compact_max_res": (-1,),
    "scatter_bin_per_cu": (0, 5),
    "scatter_bin_wgs": (-1, 65536),
    "scatter_skip_zero": (),
    "scatter_reduce_threads": (511, 513, 1023, 1025),
    "scatter_level_groups": (0, 33),
    "gather_pair_loads": (-1, 3),
    "gather_dedup_max_res": (-1,),
    "gather_lds_pad": (-1, 65537),
    "mlp_fwd_blocks": (0, 65536),
    "mlp_fwd_wps": (1, 4),
    "mlp_bwd_blocks": (0, 513),
}

# the scatter settings every scatter test walks (the other keys at their defaults)
SCATTER_SETTINGS = [
    ("defaults", {}),
    ("compact_max_res=0", {"scatter_compact_max_res": 0}),
    ("skip_zero=0", {"scatter_skip_zero": 0}),
    ("bin_wgs=4", {"scatter_bin_wgs": 4}),
    ("bin_wgs=8", {"scatter_bin_wgs": 8}),
    ("bin_per_cu=1", {"scatter_bin_per_cu": 1}),
    ("reduce_threads=512", {"scatter_reduce_threads": 512}),
    ("level_groups=2", {"scatter_level_groups": 2}),
    ("level_groups=4", {"scatter_level_groups": 4}),
    ("all non-default", {"scatter_compact_max_res": 0, "scatter_skip_zero": 0, "scatter_bin_wgs": 4,
                         "scatter_bin_per_cu": 1, "scatter_reduce_threads": 512, "scatter_level_groups": 2}),
]
GATHER_SETTINGS = [(pl, dd) for pl in (0, 1, 2) for dd in (0, 512)]

# ---- the exact level table: four levels of scale 32 / resolution 33 (a 34^3 vertex lattice)
EXACT_SIZES = (39304,   # 34^3: dense, 10 buckets of 4096 rows
               16384,   # hashed, a power of two
               4096,    # hashed, ONE bucket (sliced at the capacity the tests use)
               12344)   # hashed, not a power of two: the `% hsize` arms; blocked: 771 blocks, not a power of two either
EXACT_OFFSETS = (0, 39304, 55688, 59784, 72128)
EXACT_SCALE, EXACT_RES = 32.0, 33
EXACT_RAYS, EXACT_PER_RAY = 61, 97
EXACT_M = EXACT_RAYS * EXACT_PER_RAY          # 5917: a multiple of neither 64 nor 256
EXACT_CAPACITY = 3 * EXACT_M                  # m_host = level_stride of every call (m_dev = EXACT_M)
LAYOUTS = ("hash", "blocked", "tiled")


def exact_oracle_levels(gridtype):
    return O.GridLevels(4, 2, EXACT_RES, EXACT_RES, 16, list(EXACT_OFFSETS), [EXACT_SCALE] * 4, [EXACT_RES] * 4,
                        gridtype == "blocked", gridtype == "tiled")


def device_levels(gridtype, offsets=EXACT_OFFSETS, scale=EXACT_SCALE, res=EXACT_RES):
    """An encoding.GridLevels whose table does NOT come from its constructor: the C ABI takes any offsets."""
    from src.latent_nerf.models import encoding as E
    L = len(offsets) - 1
    lv = E.GridLevels(num_levels=L, level_dim=2, base_resolution=res, desired_resolution=res, log2_hashmap_size=16,
                      gridtype=gridtype)
    lv.offsets, lv.scales, lv.resolutions = list(offsets), [float(scale)] * L, [int(res)] * L
    lv.n_rows = offsets[-1]
    lv.c_offsets = (ctypes.c_int32 * (L + 1))(*lv.offsets)
    lv.c_scales = (ctypes.c_float * L)(*lv.scales)
    lv.c_res = (ctypes.c_int32 * L)(*lv.resolutions)
    return lv


def exact_lattice():
    """J int64 [EXACT_M, 3] in [0, 256]: x = J / 128 - 1.  61 rays of 97 samples, each a clamped cumulative sum of
    increments in {0..3} applied with probability 0.35 with a per-ray sign; the first 80 samples are one point (a run
    over the 16-lane rows, lane 32 and a wavefront boundary); both corners of the box are there."""
    g = torch.Generator().manual_seed(1234)
    R, S = EXACT_RAYS, EXACT_PER_RAY
    start = torch.randint(0, 257, (R, 1, 3), generator=g)
    inc = torch.randint(0, 4, (R, S, 3), generator=g)
    move = (torch.rand(R, S, 1, generator=g) < 0.35).long()
    sign = torch.randint(0, 2, (R, 1, 3), generator=g) * 2 - 1
    step = inc * move * sign
    step[:, 0] = 0
    J = (start + step.cumsum(1)).clamp(0, 256).reshape(-1, 3)
    J[:80] = J[0].clone()
    J[S + 5] = 0          # x = (-1, -1, -1)
    J[S + 6] = 256        # x = (+1, +1, +1): pos_grid + 1 == resolution
    return J


@functools.lru_cache(maxsize=None)
def exact_inputs():
    """(J, x f32 [M, 3], table f32 [rows, 2], grad f32 [M, 8]) -- shared by the three layouts."""
    J = exact_lattice()
    x = J.float() / 128.0 - 1.0
    g = torch.Generator().manual_seed(4321)
    table = torch.randint(-32, 33, (EXACT_OFFSETS[-1], 2), generator=g).float() / 8.0
    grad = torch.randint(-3, 4, (EXACT_M, 8), generator=g).float()
    grad[(torch.arange(EXACT_M) % EXACT_PER_RAY) > 70] = 0.0     # the tail of every ray: exact zeros
    return J, x, table, grad


def oracle_forward_backward(x, table, grad, lv, dtype):
    """(features [M, 2 L], dtable [rows, 2]) of the oracle evaluated in `dtype`."""
    t = table.to(dtype).clone().requires_grad_()
    feat = O.grid_encode((x.to(dtype) + 1.0) / 2.0, t, lv)
    feat.backward(grad.to(dtype))
    return feat.detach(), t.grad.detach()


@functools.lru_cache(maxsize=None)
def exact_case(gridtype):
    """dict(x, table, grad, lv, feat, dtable, dxyz): the float64 oracle of one layout on the exact inputs.
    feat [M, 8] (column 2 l + f), dtable [rows, 2], dxyz [M, 3] = d <grad, feat> / d x."""
    J, x, table, grad = exact_inputs()
    lv = exact_oracle_levels(gridtype)
    feat, dtable = oracle_forward_backward(x, table, grad, lv, torch.float64)
    xr = x.double().clone().requires_grad_()
    f2 = O.grid_encode((xr + 1.0) / 2.0, table.double(), lv)
    (dxyz,) = torch.autograd.grad(f2, xr, grad.double())
    return dict(J=J, x=x, table=table, grad=grad, lv=lv, feat=feat, dtable=dtable, dxyz=dxyz)


@functools.lru_cache(maxsize=None)
def first_ray_case(gridtype):
    """The exact inputs with m_dev = EXACT_PER_RAY: only the first ray is scattered, so most buckets receive NO record.
    dict(dtable, empty): the float64 oracle with the gradient rows >= EXACT_PER_RAY zeroed, and per level the list of
    (first row, one past the last row) of its buckets of 4096 rows that no non-zero record reaches (sum of |w g|)."""
    _, x, table, grad = exact_inputs()
    g1 = grad.clone()
    g1[EXACT_PER_RAY:] = 0.0
    lv = exact_oracle_levels(gridtype)
    _, dtable = oracle_forward_backward(x, table, g1, lv, torch.float64)
    _, dabs = oracle_forward_backward(x, torch.zeros_like(table), g1.abs(), lv, torch.float64)
    empty = []
    for a, b in zip(EXACT_OFFSETS[:-1], EXACT_OFFSETS[1:]):
        spans = [(r, min(r + 4096, b)) for r in range(a, b, 4096)]
        empty.append([s for s in spans if float(dabs[s[0]:s[1]].sum()) == 0.0])
    return dict(dtable=dtable, empty=empty)


def level_major(g, L, stride):
    """[M, 2 L] sample-major -> [L, stride, 2] level-major (rows >= M zero)."""
    M = g.shape[0]
    out = torch.zeros(L, stride, 2, dtype=g.dtype)
    out[:, :M] = g.reshape(M, L, 2).permute(1, 0, 2)
    return out


def sample_major(feat, M):
    """[L, stride, 2] -> [M, 2 L]."""
    L = feat.shape[0]
    return feat[:, :M].permute(1, 0, 2).reshape(M, 2 * L)


def cell_runs(J, wave=None):
    """Lengths of the runs of consecutive samples in one cell (cell = floor(J / 8 + 0.5) per axis); wave: runs are
    also cut every `wave` samples, as the lanes of a wavefront see them.  -> (lengths, run id per sample)."""
    cell = (J + 4) // 8
    head = torch.ones(J.shape[0], dtype=torch.bool)
    head[1:] = (cell[1:] != cell[:-1]).any(-1)
    if wave:
        head |= (torch.arange(J.shape[0]) % wave) == 0
    rid = head.long().cumsum(0) - 1
    return torch.bincount(rid), rid


# ---- ordinary inputs: the standard table at the small configuration, samples along rays
SMALL = dict(num_levels=16, base_resolution=4, desired_resolution=128, log2_hashmap_size=12)
ORD_RAYS, ORD_PER_RAY = 300, 97
ORD_STEPS = (0.0009, 0.0034, 0.02)


@functools.lru_cache(maxsize=None)
def ordinary_inputs():
    """(x [M, 3], grad [M, 32]), M = 29100: ray r marches with step ORD_STEPS[r % 3]; every 7th ray is axis-parallel;
    the gradient is exactly zero behind a random termination point of each ray."""
    g = torch.Generator().manual_seed(21)
    R, S = ORD_RAYS, ORD_PER_RAY
    o = (torch.rand(R, 1, 3, generator=g) * 2 - 1) * 0.6
    d = torch.nn.functional.normalize(torch.randn(R, 1, 3, generator=g), dim=-1)
    d[::7] = torch.tensor([1.0, 0.0, 0.0])
    step = torch.tensor(ORD_STEPS)[torch.arange(R) % 3].view(R, 1, 1)
    t = torch.arange(S).view(1, S, 1) * step
    x = (o + d * t).clamp(-0.999, 0.999).reshape(-1, 3)
    M = x.shape[0]
    grad = torch.randn(M, 32, generator=g)
    dead = (torch.arange(M) % S) >= torch.randint(20, S + 1, (R,), generator=g).repeat_interleave(S)
    grad[dead] = 0.0
    return x, grad


@functools.lru_cache(maxsize=None)
def ordinary_case(gridtype, table_bf16=False):
    """dict(x, table, grad, lv, feat, dtable): the f32 oracle (the reference of the module's existing tolerances)."""
    x, grad = ordinary_inputs()
    lv = O.make_grid_levels(blocked=gridtype == "blocked", tiled=gridtype == "tiled", **SMALL)
    g = torch.Generator().manual_seed(5)
    table = torch.randn(lv.n_rows, 2, generator=g) * 0.1
    if table_bf16:
        table = table.to(torch.bfloat16).float()
    feat, dtable = oracle_forward_backward(x, table, grad, lv, torch.float32)
    return dict(x=x, table=table, grad=grad, lv=lv, feat=feat, dtable=dtable)
