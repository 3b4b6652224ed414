"""float64 reference of the training march (csrc/rays.hip k_march_train; contract H4 in include/lnerf_hip.h) that
CLASSIFIES the lattice points of every ray instead of predicting f32 rounding, the cases at the march's geometric edges,
and a checker for any march output (the oracle's or the GPU's).

The definition, restated in float64 (not the kernel's op order):
    near, far   slab test of the ray against the box, near = max(near, min_near); a ray with a zero direction component
                is unconstrained on that axis if its origin lies strictly inside the slab and misses otherwise (a ray IN
                a face plane is a miss: the f32 code's 0 * inf = NaN ends there too)
    lattice     t_0 = near + step(near) u,  t_{k+1} = t_k + step(t_k),  step(t) = min(max(t dt_gamma, dt_min), dt_max)
                with the f32 constants dt_min = 2 sqrt(3) / max_steps, dt_max = 2 sqrt(3) 2^(cascade-1) / G of
                make_params (one rule, also at dt_gamma = 0: dt_max where dt_min > dt_max)
    position    x = clamp(o + t d, -bound, bound)
    level       max(e(max_a |x_a|), e(step G / 2)) with e = frexp's exponent clamped to [0, cascade - 1];
                mip_bound = min(2^level, bound)
    cell        floor(clamp((x / mip_bound + 1) G / 2, 0, G - 1)) per axis, bit level G^3 + Morton(cell)
    sample      the points with t_k < far whose bit is set, the first max_steps of them

Error bounds (ULP = 2^-24, one f32 rounding relative to the result).  An f32 march computes
    near, far   (b - o) * (1 / d): three roundings, no cancellation beyond the one subtraction of two inputs, then
                maxima; t_0 adds a product and a sum: |t_0 - fl| <= 6 ULP max(t, 1)
    t_k         dt_gamma = 0: fl(fl(k dt) + t_0), two more roundings (the inference march: k additions, as below);
                dt_gamma > 0: k additions, each half an ULP of t, plus the rounding of the step t dt_gamma, half an
                ULP of dt <= t; the step's dependence on t keeps the RELATIVE error (t grows by the same factor), and
                below t = 1, where the bound is absolute, the step is clamped or its error smaller still: <= 1 ULP t
                per step.  ERR_T(k, t) = (k + 8) ULP max(t, 1)   (half of the (k + 4) 2^-23 this reference began with)
    far         FAR_ERR = 2^-21 max(|far|, 1): the three roundings above, with room
    x_a         |d_a| ERR_T + 4 ULP (|o_a| + t |d_a|): the product and the sum are two roundings; four, as for near
    u_a         err(x_a) / mip_bound * G / 2 + 4 ULP G in grid units: 1 / mip_bound, the product, the + 1 are three
                roundings of values <= 2, scaled by G / 2 (exact); the cell index is decided on u_a -+ that
    level       the position's level is decided on max|x| -+ err(x), the step's on step G / 2 (1 -+ 1e-5)
A lattice point is
    MUST        surely before far, level and cell the same anywhere inside the bounds, and the bit set
    MUST_NOT    surely at or past far (PAST_FAR), or the same certainty of an EMPTY cell
    FREE        far, a cell boundary or a level boundary lies within the bounds, or the ray's hit / miss is not
                certain (|far - near| within FAR_ERR of both): either outcome is right
build_case asserts, per case, FREE <= 3 % of the lattice points (those not surely past far) and MUST >= 90 % of the
points that are valid and occupied in float64: a case cannot pass by declaring everything free.

Measured free share per configuration (bound, cascade, G, max_steps, dt_gamma), the largest over its occupancy
patterns, and the smallest MUST share; printed per case by test_march_reference_cpu.py::test_case_table (pytest -s):
    plain       (1, 1, 32, 128, 0)        free <= 0.75 %   must >= 99.5 %   (both extremes: the non-cubic inner box)
    workload    (1, 1, 128, 1024, 0)      free <= 0.64 %   must >= 98.7 %
    cap100      (2, 2, 32, 100, 0)        free <= 0.96 %   must >= 98.5 %   (both extremes: the non-cubic inner box; its faces are cell planes)
    cascade3    (4, 3, 32, 256, 1/32)     free <= 0.03 %   must >= 99.9 %
    steplevel   (8, 4, 16, 512, 1/16)     free <= 0.03 %   must >= 99.8 %
    bound1p5    (1.5, 2, 32, 128, 1/64)   free <= 0.03 %   must >= 99.9 %
    inverted16  (1, 1, 64, 16, 0)         free <= 0.02 %   must >= 99.9 %
    inverted64  (1, 1, 128, 64, 0)        free <= 0.07 %   must >= 99.9 %
Of the oracle's samples, and of the GPU's (the same, bit for bit), 0 - 0.7 % sit on FREE points (workload-full: 632 of
98697).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import nerf_oracle as O

ULP = 2.0 ** -24
FREE, MUST, EMPTY, PAST_FAR = 0, 1, 2, 3      # classes of a lattice point (EMPTY and PAST_FAR: must not be a sample)
SQRT3 = 1.7320508075688772

# (bound, cascade, G, max_steps, dt_gamma)
CONFIGS = {
    "plain": (1.0, 1, 32, 128, 0.0),
    "workload": (1.0, 1, 128, 1024, 0.0),
    "cap100": (2.0, 2, 32, 100, 0.0),
    "cascade3": (4.0, 3, 32, 256, 1.0 / 32),
    "steplevel": (8.0, 4, 16, 512, 1.0 / 16),
    "bound1p5": (1.5, 2, 32, 128, 1.0 / 64),
    "inverted16": (1.0, 1, 64, 16, 0.0),       # dt_min > dt_max
    "inverted64": (1.0, 1, 128, 64, 0.0),      # dt_min > dt_max
}
PATTERNS = ("random30", "full", "isolated", "checker", "planes", "shell", "ring")
INNER_BOX = (-0.5, -0.25, -0.5, 0.5, 0.75, 0.5)   # the non-cubic box of the `_aabb` form, strictly inside bound 1
MIN_NEAR = 0.1
JITTER = (0.0, 1.0 - 2.0 ** -24, 0.5, 0.25, 2.0 ** -24, 0.73, 0.999, 0.37, 0.125, 0.61)


def case_names():
    """Every occupancy pattern with every configuration it makes sense for (`ring` needs cascades), plus the
    non-cubic box on the two configurations with bound 1 ... 2 it fits strictly inside."""
    names = []
    for c, cfg in CONFIGS.items():
        for p in PATTERNS:
            if p != "ring" or cfg[1] > 1:
                names.append("%s-%s" % (c, p))
    return names + ["plain-random30-innerbox", "cap100-checker-innerbox"]


def capacity_case_names():
    """One case per configuration for the march under capacity M // 3."""
    return ["%s-random30" % c for c in CONFIGS]


# ------------------------------------------------------------------------------------------ occupancy patterns
def _morton(n):
    def expand(v):
        v = v.astype(np.uint64)
        v = (v * np.uint64(0x00010001)) & np.uint64(0xFF0000FF)
        v = (v * np.uint64(0x00000101)) & np.uint64(0x0F00F00F)
        v = (v * np.uint64(0x00000011)) & np.uint64(0xC30C30C3)
        v = (v * np.uint64(0x00000005)) & np.uint64(0x49249249)
        return v
    return (expand(n[..., 0]) | (expand(n[..., 1]) << np.uint64(1)) | (expand(n[..., 2]) << np.uint64(2))).astype(np.int64)


def occupancy(pattern, bound, cascade, G, seed=0):
    """bool [cascade, G, G, G] indexed [level, x, y, z]."""
    rng = np.random.RandomState(seed)
    i = np.arange(G)
    x, y, z = np.meshgrid(i, i, i, indexing="ij")
    occ = np.zeros((cascade, G, G, G), dtype=bool)
    for l in range(cascade):
        if pattern == "random30":
            occ[l] = rng.rand(G, G, G) < 0.3
        elif pattern == "full":
            occ[l] = True
        elif pattern == "isolated":           # one cell per 8^3 block
            nb = G // 8
            p = rng.randint(0, 8, size=(nb, nb, nb, 3))
            b = np.stack(np.meshgrid(*[np.arange(nb)] * 3, indexing="ij"), -1)
            c = (b * 8 + p).reshape(-1, 3)
            occ[l][c[:, 0], c[:, 1], c[:, 2]] = True
        elif pattern == "checker":
            occ[l] = (x + y + z) % 2 == 0
        elif pattern == "planes":             # one cell thick, one normal to each axis
            occ[l] = (x == G // 3) | (y == G // 2 + 1) | (z == (2 * G) // 3)
        elif pattern == "shell":              # the outermost cell layer only
            occ[l] = (x == 0) | (x == G - 1) | (y == 0) | (y == G - 1) | (z == 0) | (z == G - 1)
        elif pattern == "ring":               # level l only where it lies outside level l - 1 (level 0: all of it)
            if l == 0:
                occ[l] = True
            else:
                mb, inner = min(2.0 ** l, bound), min(2.0 ** (l - 1), bound)
                c = ((np.stack([x, y, z], -1) + 0.5) / G * 2.0 - 1.0) * mb
                occ[l] = np.abs(c).max(-1) > inner
        else:
            raise ValueError(pattern)
    return occ


def pack_occupancy(occ):
    """bool [cascade, G, G, G] -> the march's bitfield (uint8 tensor), Morton order per level."""
    cascade, G = occ.shape[0], occ.shape[1]
    i = np.arange(G)
    n = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3)
    flat = np.zeros((cascade, G ** 3), dtype=np.float32)
    flat[:, _morton(n)] = occ.reshape(cascade, -1)
    return O.packbits(torch.from_numpy(flat.reshape(-1)), 0.5)


# ------------------------------------------------------------------------------------------ rays
def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.linalg.norm(v)).astype(np.float32)


def build_rays(bound, box, dt_step):
    """(rays_o, rays_d, jitter, names of the edge rays): a 12 x 12 camera view from radius 1.25 bound, then the edge
    rays, laid out against `box` (lo, hi per axis).  dt_step: the smallest step, which the corner clip stays under."""
    import math
    HW = 12
    f = HW / (2 * math.tan(math.radians(55) / 2))
    c2w = O.pose_from_angles(math.radians(60), math.radians(20), 1.25 * bound)
    ro, rd = O.get_rays(c2w, f, f, HW / 2, HW / 2, HW, HW)
    o, d = [r for r in ro[0].numpy()], [r for r in rd[0].numpy()]
    u = [JITTER[i % len(JITTER)] for i in range(len(o))]
    lo, hi = np.array(box[:3], dtype=np.float64), np.array(box[3:], dtype=np.float64)
    ctr, half = (lo + hi) / 2, (hi - lo) / 2
    names = []

    def add(name, org, direction, jitter):
        names.append((name, len(o)))
        o.append(np.asarray(org, dtype=np.float32))
        d.append(np.asarray(direction, dtype=np.float32))
        u.append(jitter)

    off = (0.137, -0.291)                     # offsets of the axis rays: on no cell plane of any level
    for a in range(3):
        for s in (1.0, -1.0):
            org = ctr.copy()
            org[(a + 1) % 3] += off[0] * half[(a + 1) % 3]
            org[(a + 2) % 3] += off[1] * half[(a + 2) % 3]
            org[a] -= s * (half[a] + 0.5 * bound)
            e = np.zeros(3)
            e[a] = s
            add("axis%+d" % (s * (a + 1)), org, e, JITTER[(2 * a + (s < 0)) % len(JITTER)])
    add("negzero", ctr + [0.21 * half[0], -half[1] - 0.5 * bound, 0.33 * half[2]], [-0.0, 1.0, -0.0], 0.5)
    add("inside", ctr + [0.3 * half[0], -0.2 * half[1], 0.1 * half[2]], _unit([0.5, 0.7, -0.4]), 0.25)
    add("centre", ctr, _unit([0.3, -0.5, 0.8]), 0.73)
    add("diagonal", lo - half * 0.5, _unit(half), 0.37)
    add("nearface", [ctr[0] + 0.999 * half[0], lo[1] - 0.5 * bound, ctr[2] + 0.2 * half[2]], [0.0, 1.0, 0.0], 0.61)
    add("inface", [hi[0], lo[1] - 0.5 * bound, ctr[2] + 0.2 * half[2]], [0.0, 1.0, 0.0], 0.5)
    add("miss", hi + 2.0 * bound, [1.0, 0.0, 0.0], 0.5)
    # corner clip: through a point dt/8 inside the (hi, hi) edge, across it: inside the box for 0.35 dt
    eps = dt_step / 8
    cdir = _unit([1.0, -1.0, 0.0]).astype(np.float64)
    p = np.array([hi[0] - eps, hi[1] - eps, ctr[2] + 0.3 * half[2]])
    add("corner_u0", p - bound * cdir, cdir, 0.0)
    add("corner_u1", p - bound * cdir, cdir, 1.0 - 2.0 ** -24)
    add("near_past_far", [hi[0] - 0.5 * MIN_NEAR, ctr[1], ctr[2]], _unit([1.0, 0.05, 0.02]), 0.0)
    return (torch.from_numpy(np.stack(o).astype(np.float32)), torch.from_numpy(np.stack(d).astype(np.float32)),
            torch.tensor(u, dtype=torch.float64).to(torch.float32), dict(names))


# ------------------------------------------------------------------------------------------ the float64 reference
MarchRef = namedtuple("MarchRef", "cfg box o d u hit near far t dt err_t cls level level_dt max_steps stats")


def step_constants(cascade, G, max_steps):
    """(dt_min, dt_max) of make_params, as the f32 values they are."""
    return (float(np.float32(2.0 * SQRT3 / max_steps)), float(np.float32(2.0 * SQRT3 * (1 << (cascade - 1)) / G)))


def err_t(k, t):
    return (k + 8) * ULP * np.maximum(np.abs(t), 1.0)


def far_err(far):
    return 2.0 ** -21 * np.maximum(np.abs(far), 1.0)


def slab(o, d, box, min_near):
    """float64 slab test -> (hit: 1 sure hit, 0 sure miss, -1 within the margin, near, far)."""
    N = o.shape[0]
    lo, hi = np.asarray(box[:3], dtype=np.float64), np.asarray(box[3:], dtype=np.float64)
    near, far = np.full(N, -np.inf), np.full(N, np.inf)
    miss = np.zeros(N, dtype=bool)
    for a in range(3):
        z = d[:, a] == 0
        with np.errstate(divide="ignore", invalid="ignore"):
            t1, t2 = (lo[a] - o[:, a]) / d[:, a], (hi[a] - o[:, a]) / d[:, a]
        miss |= z & ~((o[:, a] > lo[a]) & (o[:, a] < hi[a]))
        near = np.where(z, near, np.maximum(near, np.minimum(t1, t2)))
        far = np.where(z, far, np.minimum(far, np.maximum(t1, t2)))
    near = np.maximum(near, min_near)
    margin = far_err(far) + far_err(near)
    hit = np.where(miss | (near - far > margin), 0, np.where(far - near > margin, 1, -1))
    return hit, near, far


def _exponent(v):
    """frexp's exponent (0 for 0)."""
    return np.frexp(v)[1].astype(np.int64)


def build_reference(o32, d32, u32, bits, cfg, box, min_near=MIN_NEAR):
    bound, cascade, G, max_steps, dt_gamma = cfg
    o, d, u = o32.numpy().astype(np.float64), d32.numpy().astype(np.float64), u32.numpy().astype(np.float64)
    N = o.shape[0]
    dt_min, dt_max = step_constants(cascade, G, max_steps)
    gam = float(np.float32(dt_gamma))
    step = lambda t: np.minimum(np.maximum(t * gam, dt_min), dt_max)
    hit, near, far = slab(o, d, box, min_near)
    live = hit != 0
    near0 = np.where(live, near, 0.0)
    far0 = np.where(live, far, 0.0)
    # the lattice, up to the first two points surely past far
    ts, dts = [], []
    t = near0 + step(near0) * u
    k = 0
    past = np.zeros(N, dtype=np.int64)
    while True:
        ts.append(t)
        dts.append(step(t))
        past += (t - err_t(k, t) >= far0 + far_err(far0)) | ~live
        if bool((past >= 2).all()):
            break
        t = t + dts[-1]
        k += 1
        assert k < 1 << 16, "lattice did not end"
    t, dt = np.stack(ts, 1), np.stack(dts, 1)                       # [N,K]
    K = t.shape[1]
    et = err_t(np.arange(K)[None, :], t)
    assert float((et / dt).max()) < 0.25, "the drift bound must stay well under a step"
    fe = far_err(far0)[:, None]
    sure_valid = (t + et < far0[:, None] - fe) & (hit == 1)[:, None]
    sure_past = (t - et >= far0[:, None] + fe) | (hit == 0)[:, None]
    nominal_valid = (t < far0[:, None]) & live[:, None]
    # position, level, cell: nominal and at both ends of the bounds
    x = np.clip(o[:, None, :] + t[..., None] * d[:, None, :], -bound, bound)
    ex = np.abs(d)[:, None, :] * et[..., None] + 4 * ULP * (np.abs(o)[:, None, :] + t[..., None] * np.abs(d)[:, None, :])
    mx, emx = np.abs(x).max(-1), ex.max(-1)
    lv = lambda e: np.clip(e, 0, cascade - 1)
    s = dt * (G * 0.5)
    if cascade > 1:
        l_pos, l_dt = lv(_exponent(mx)), lv(_exponent(s))
        level_sure = ((lv(_exponent(np.maximum(mx - emx, 0))) == lv(_exponent(mx + emx)))
                      & (lv(_exponent(s * (1 - 1e-5))) == lv(_exponent(s * (1 + 1e-5)))))
    else:
        l_pos = l_dt = np.zeros_like(mx, dtype=np.int64)
        level_sure = np.ones_like(mx, dtype=bool)
    level = np.maximum(l_pos, l_dt)
    mip = np.minimum(2.0 ** level, bound)[..., None]
    ug = (x / mip + 1.0) * (G * 0.5)
    eu = ex / mip * (G * 0.5) + 4 * ULP * G
    cell = lambda v: np.floor(np.clip(v, 0.0, G - 1.0)).astype(np.int64)
    n = cell(ug)
    cell_sure = (cell(ug - eu) == cell(ug + eu)).all(-1)
    idx = level * G ** 3 + _morton(n)
    bitsn = bits.numpy()
    occ = ((bitsn[idx >> 3] >> (idx & 7)) & 1).astype(bool)
    sure = level_sure & cell_sure
    cls = np.full(t.shape, FREE, dtype=np.int64)
    cls[sure_valid & sure & occ] = MUST
    cls[~sure_past & sure & ~occ] = EMPTY
    cls[sure_past] = PAST_FAR
    cls[(hit == -1), :] = FREE
    lattice = ~sure_past
    n_lat = int(lattice.sum())
    n_free = int((lattice & (cls == FREE)).sum())
    n_occ = int((nominal_valid & occ).sum())
    n_must = int((cls == MUST).sum())
    stats = dict(lattice=n_lat, free=n_free, occupied=n_occ, must=n_must,
                 free_share=n_free / max(n_lat, 1), must_share=n_must / max(n_occ, 1))
    return MarchRef(cfg, tuple(box), o, d, u, hit, near, far, t, dt, et, cls, np.where(level_sure, level, -1),
                    np.where(level_sure, l_dt > l_pos, False), max_steps, stats)


# ------------------------------------------------------------------------------------------ cases
Case = namedtuple("Case", "name cfg box bits ro rd noises edge ref")


@functools.lru_cache(maxsize=None)
def build_case(name):
    """The case `name` = configuration-pattern[-innerbox], built once per process; never modified."""
    parts = name.split("-")
    cfg = CONFIGS[parts[0]]
    bound, cascade, G, max_steps, dt_gamma = cfg
    box = INNER_BOX if parts[-1] == "innerbox" else (-bound,) * 3 + (bound,) * 3
    bits = pack_occupancy(occupancy(parts[1], bound, cascade, G))
    dt_min, dt_max = step_constants(cascade, G, max_steps)
    ro, rd, noises, edge = build_rays(bound, box, min(dt_min, dt_max))
    ref = build_reference(ro, rd, noises, bits, cfg, box)
    st = ref.stats
    assert st["free_share"] <= 0.03, (name, st)
    assert st["occupied"] > 0 and st["must_share"] >= 0.90, (name, st)
    # the edge rays are what they are meant to be
    assert ref.hit[edge["inface"]] == 0 and ref.hit[edge["miss"]] == 0 and ref.hit[edge["near_past_far"]] == 0
    assert ref.near[edge["inside"]] == MIN_NEAR and ref.near[edge["centre"]] == MIN_NEAR
    c = edge["corner_u0"]
    assert ref.hit[c] == 1 and ref.far[c] - ref.near[c] < min(dt_min, dt_max)
    for e in ("axis+1", "axis-2", "negzero", "diagonal", "nearface"):
        assert ref.hit[edge[e]] == 1, (name, e)
    must = ref.cls == MUST
    if parts[1] in ("random30", "full", "checker"):
        if cascade >= 3:          # samples on every level
            assert all(bool((must & (ref.level == l)).any()) for l in range(cascade)), name
        if parts[0] == "steplevel":   # the step size drives the level
            assert int((must & ref.level_dt).sum()) > 100, name
    if parts[0] == "cap100" and parts[1] in ("full", "checker") and parts[-1] != "innerbox":
        # rays that reach the cap of 100, which is no multiple of the 64-point chunk: the 100th sample falls inside a
        # chunk, in the middle of a four-chunk round; `checker` is the partial grid (empty points before the cap)
        capped = np.nonzero(must.sum(1) > 100)[0]
        assert len(capped) >= (3 if parts[1] == "full" else 1), name
        k100 = np.array([np.nonzero(must[n])[0][99] for n in capped])
        assert bool((k100 % 64 != 63).all()), name
        if parts[1] == "checker":
            assert all(bool((ref.cls[n][:k] == EMPTY).sum() > 10) for n, k in zip(capped, k100)), name
    return Case(name, cfg, box, bits, ro, rd, noises, edge, ref)


MarchOut = namedtuple("MarchOut", "rays xyzs dirs deltas counter")


@functools.lru_cache(maxsize=None)
def oracle_march(name):
    """The oracle's march of a case (no capacity): MarchOut of CPU tensors, counter = (M, live rays, dropped rays)."""
    c = build_case(name)
    bound, cascade, G, max_steps, dt_gamma = c.cfg
    nears, fars = O.near_far_from_aabb(c.ro, c.rd, list(c.box), MIN_NEAR)
    xyzs, dirs, deltas, rays, M = O.march_rays_train(c.ro, c.rd, nears, fars, c.bits, bound, cascade, G, max_steps,
                                                     dt_gamma, c.noises)
    counter = torch.tensor([M, int((rays[:, 2] > 0).sum()), 0], dtype=torch.int32)
    return MarchOut(rays, xyzs, dirs, deltas, counter)


# ------------------------------------------------------------------------------------------ the checker
def _fail(rule, msg, *args):
    raise AssertionError("march rule [%s]: %s" % (rule, msg % args))


def assert_march(ref, rays, xyzs, dirs, deltas, counter, capacity, raw_rays=None):
    """Check a march output against the reference `ref`; the failing rule is named in the AssertionError.
    rays int32 [N,3], xyzs / dirs [>= M, 3], deltas [>= M, 2], counter int32 [>= 3] (word 3, the peak, is checked when
    present: fresh buffers), capacity: the size the march was given.  raw_rays: the rays of the same march without a
    capacity, needed when the capacity drops rays (a dropped ray's count is gone from the output).
    Returns dict(samples, on_free, matched): how many samples were checked, how many of them sit on FREE points, and
    per ray the lattice point of each of its samples."""
    rays = torch.as_tensor(rays).cpu().to(torch.int64)
    N = ref.o.shape[0]
    bound, cascade, G, max_steps, dt_gamma = ref.cfg
    gam = float(np.float32(dt_gamma))
    if rays.shape != (N, 3) or not torch.equal(rays[:, 0], torch.arange(N)):
        _fail("rays", "rays must be [N,3] with the ray ids in order")
    raw = rays if raw_rays is None else torch.as_tensor(raw_rays).cpu().to(torch.int64)
    if int(raw[:, 2].max()) > max_steps:
        n = int(raw[:, 2].argmax())
        _fail("cap", "ray %d has %d samples, max_steps is %d", n, int(raw[n, 2]), max_steps)
    # offsets: the exclusive scan of the counts, then the capacity rule
    scan = torch.cumsum(raw[:, 2], 0) - raw[:, 2]
    if not torch.equal(raw[:, 1], scan):
        n = int((raw[:, 1] != scan).nonzero()[0])
        _fail("offsets", "ray %d starts at %d, the exclusive scan of the counts gives %d", n, int(raw[n, 1]), int(scan[n]))
    want, M, live, dropped = O.apply_capacity(raw.to(torch.int32), int(capacity))
    if not torch.equal(rays, want.to(torch.int64)):
        n = int((rays != want).any(1).nonzero()[0])
        _fail("offsets", "ray %d is %s, the capacity rule gives %s", n, rays[n].tolist(), want[n].tolist())
    cnt = torch.as_tensor(counter).cpu().to(torch.int64)[:4].tolist()
    if cnt[:3] != [M, live, dropped]:
        _fail("counter", "counter %s, expected M, live, dropped = %s", cnt[:3], [M, live, dropped])
    if len(cnt) == 4 and cnt[3] != (M | ((1 << 30) if dropped else 0)):
        _fail("counter", "peak word %#x for M = %d, dropped = %d", cnt[3], M, dropped)
    xyzs, dirs, deltas = [torch.as_tensor(a).cpu() for a in (xyzs, dirs, deltas)]
    d32 = ref.d.astype(np.float32)
    samples = on_free = 0
    matched = [np.zeros(0, dtype=np.int64)] * N
    for n in range(N):
        off, c = int(rays[n, 1]), int(rays[n, 2])
        was_dropped = c == 0 and int(raw[n, 2]) > 0
        cls, tk = ref.cls[n], ref.t[n]
        if ref.hit[n] == 0 and (c or int(raw[n, 2])):
            _fail("miss", "ray %d misses the box by more than the margin and has %d samples", n, max(c, int(raw[n, 2])))
        if c == 0:
            if not was_dropped and bool((cls == MUST).any()):
                _fail("must", "ray %d has no samples, lattice point %d must be one", n, int(np.nonzero(cls == MUST)[0][0]))
            continue
        ts = deltas[off:off + c, 1].numpy().astype(np.float64)
        dts = deltas[off:off + c, 0].numpy().astype(np.float64)
        k = np.clip(np.searchsorted(tk, ts), 1, len(tk) - 1)
        k = np.where(np.abs(tk[k - 1] - ts) <= np.abs(tk[k] - ts), k - 1, k)
        bad = np.abs(tk[k] - ts) > ref.err_t[n, k]
        if bool(bad.any()):
            i = int(np.nonzero(bad)[0][0])
            _fail("lattice", "ray %d sample %d: t = %.9g is %.3g from lattice point %d (t = %.9g), the bound is %.3g",
                  n, i, ts[i], abs(tk[k[i]] - ts[i]), int(k[i]), tk[k[i]], ref.err_t[n, k[i]])
        if bool((np.diff(k) <= 0).any()):
            i = int(np.nonzero(np.diff(k) <= 0)[0][0])
            _fail("lattice", "ray %d samples %d and %d match lattice points %d and %d: not distinct and increasing",
                  n, i, i + 1, int(k[i]), int(k[i + 1]))
        kc = cls[k]
        if bool((kc == PAST_FAR).any()):
            i = int(np.nonzero(kc == PAST_FAR)[0][0])
            _fail("must-not", "ray %d sample %d at t = %.9g is surely at or past far = %.9g", n, i, ts[i], ref.far[n])
        if bool((kc == EMPTY).any()):
            i = int(np.nonzero(kc == EMPTY)[0][0])
            _fail("must-not", "ray %d sample %d at lattice point %d sits in an empty cell", n, i, int(k[i]))
        need = cls == MUST
        if c == max_steps:
            need[k[-1]:] = False          # a capped ray: every MUST point before the last matched one
        need[k] = False
        if bool(need.any()):
            _fail("must", "ray %d (%d samples): lattice point %d at t = %.9g must be a sample and is not", n, c,
                  int(np.nonzero(need)[0][0]), tk[np.nonzero(need)[0][0]])
        tol = gam * ref.err_t[n, k] + 2 * ULP * ref.dt[n, k]
        if gam == 0.0:
            tol = np.zeros_like(tol)      # the uniform step is one f32 constant
        bad = np.abs(dts - ref.dt[n, k]) > tol
        if bool(bad.any()):
            i = int(np.nonzero(bad)[0][0])
            _fail("dt", "ray %d sample %d: dt = %.9g, the reference step is %.9g", n, i, dts[i], ref.dt[n, k[i]])
        want_x = np.clip(ref.o[n][None, :] + ts[:, None] * ref.d[n][None, :], -bound, bound)
        tol_x = 4 * ULP * (np.abs(ref.o[n])[None, :] + ts[:, None] * np.abs(ref.d[n])[None, :])
        bad = ~(np.abs(xyzs[off:off + c].numpy().astype(np.float64) - want_x) <= tol_x)
        if bool(bad.any()):
            i = int(np.nonzero(bad.any(1))[0][0])
            _fail("xyz", "ray %d sample %d: %s, clamp(o + t d) is %s", n, i, xyzs[off + i].tolist(), want_x[i].tolist())
        if not np.array_equal(dirs[off:off + c].numpy().view(np.int32),
                              np.broadcast_to(d32[n].view(np.int32), (c, 3))):
            _fail("dirs", "ray %d: a sample's direction is not the ray's, bit for bit", n)
        samples += c
        on_free += int((kc == FREE).sum())
        matched[n] = k
    return dict(samples=samples, on_free=on_free, matched=matched)


def assert_case(name, out, capacity=None, raw_rays=None):
    c = build_case(name)
    cap = capacity if capacity is not None else max(int(out.xyzs.shape[0]), int(torch.as_tensor(out.rays)[:, 2].sum()))
    return assert_march(c.ref, out.rays, out.xyzs, out.dirs, out.deltas, out.counter, cap, raw_rays)
