"""Float64 restatement of the sketch-shape path (csrc/mesh.hip lnerf_mesh_distance / lnerf_mesh_winding_number and
src/latent_nerf/training/shape.py MeshOccupancy / ShapeLoss), written from the definitions and not from the kernel.
Not a test file.  tests/test_shape_reference_cpu.py checks it without a GPU, tests/test_gpu_shape.py uses it.

U = 2^-24 is the unit roundoff of f32 (half an ulp, relative); one ulp is at most 2 U of the value."""
import itertools

import numpy as np

U = 2.0 ** -24
REGIONS = ("A", "B", "C", "AB", "AC", "BC", "interior")
R_A, R_B, R_C, R_AB, R_AC, R_BC, R_IN = range(7)


def _dot(x, y):
    return np.einsum("...i,...i->...", x, y)


def _segment(p, s0, s1, r0, r1, r01):
    """Distance of p to the segment s0-s1 by the clamped projection, and the region of the closest point (r0 / r1 at
    the ends, r01 strictly between).  A zero-length segment is the point s0."""
    e = s1 - s0
    num, den = _dot(p - s0, e), _dot(e, e)
    t = np.where(den > 0, np.clip(num / np.where(den > 0, den, 1.0), 0.0, 1.0), 0.0)
    d = np.linalg.norm(p - (s0 + t[..., None] * e), axis=-1)
    region = np.where((num <= 0) | (den == 0), r0, np.where(num >= den, r1, r01))
    return d, region


def point_triangle(points, tris):
    """points [n,3], tris [F,3,3] -> (d [n,F] float64, region [n,F] int in range(7), names in REGIONS).

    The foot of p on the triangle's plane has the barycentric coordinates (u, v, w) of the normal equations
        [ab.ab ab.ac; ab.ac ac.ac] (v, w) = (ab.ap, ac.ap),  u = 1 - v - w;
    when all three are positive the closest point is the foot (region interior).  Otherwise it lies on the border and is
    the nearest of the three clamped projections onto AB, AC and BC; a projection clamped to an end is that vertex's
    region.  The signs are taken from the numerators, which are exact in float64 for coordinates that are multiples of
    1/8 in [-2, 2].  A triangle whose float64 area is 0 has no interior: the minimum of its three segments."""
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    t = np.asarray(tris, dtype=np.float64)
    a, b, c = t[None, :, 0, :], t[None, :, 1, :], t[None, :, 2, :]
    ab, ac, ap = b - a, c - a, p - a
    g00, g01, g11 = _dot(ab, ab), _dot(ab, ac), _dot(ac, ac)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    det = g00 * g11 - g01 * g01
    nv, nw = g11 * d1 - g01 * d2, g00 * d2 - g01 * d1
    flat = np.linalg.norm(np.cross(ab, ac), axis=-1) == 0.0
    inside = (nv > 0) & (nw > 0) & (det - nv - nw > 0) & ~flat
    safe = np.where(flat | (det == 0), 1.0, det)
    foot = ap - (nv / safe)[..., None] * ab - (nw / safe)[..., None] * ac
    d_in = np.linalg.norm(foot, axis=-1)
    segs = [_segment(p, a, b, R_A, R_B, R_AB), _segment(p, a, c, R_A, R_C, R_AC), _segment(p, b, c, R_B, R_C, R_BC)]
    ds = np.stack([np.broadcast_to(s[0], d_in.shape) for s in segs])
    rs = np.stack([np.broadcast_to(s[1], d_in.shape) for s in segs])
    k = ds.argmin(0)[None]
    d_edge = np.take_along_axis(ds, k, 0)[0]
    r_edge = np.take_along_axis(rs, k, 0)[0]
    return np.where(inside, d_in, d_edge), np.where(inside, R_IN, r_edge)


def on_lattice(x):
    """True when every coordinate is a multiple of 1/8 in [-2, 2] (the exact-arithmetic inputs of the tests)."""
    x = np.asarray(x, dtype=np.float64)
    return bool(np.all(x * 8 == np.round(x * 8)) and np.all(np.abs(x) <= 2))


def solid_angles(points, tris, exact_inputs=False):
    """points [n,3], tris [F,3,3] -> (omega [n,F], bound [n,F], ambiguous [n,F] bool); see solid_angle_parts."""
    return solid_angle_parts(points, tris, exact_inputs)[:3]


def solid_angle_parts(points, tris, exact_inputs=False):
    """points [n,3], tris [F,3,3] -> (omega [n,F], bound [n,F], ambiguous [n,F] bool, strictly_inside [n,F] bool).

    omega = 2 atan2(det, den) in float64 (van Oosterom & Strackee), a, b, c = vertices - p,
        det = a . (b x c),  den = |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|.
    bound: how far an f32 evaluation of the same expression (dot products as three-term fma chains, the rest rounded
    operation by operation) may be from omega.  With T = |a||b||c| every one of the four terms of den is at most T.
      d_den = k U 4T.  Operations: |x| = sqrt(fma chain) is 3 roundings on a sum of squares (3 U), halved by the root,
        plus the root's own: 2.5 U.  |a||b||c|: 3 x 2.5 + 2 products = 9.5 U T.  (x.y)|z|: the chain is 3 U |x||y|, the
        length 2.5 U, the product 1: 6.5 U T, three times.  Three additions, each rounding a partial sum of at most 4T:
        12 U T.  Together (9.5 + 19.5 + 12) U T = 41 U T <= 10.25 U 4T.  Inputs whose differences a, b, c are not exact
        add U |x| per vector, 3 U T per term: k = 10.25 + 3.  exact_inputs (on_lattice(...) holds) takes k = 10.25.
      d_det = 0 for exact_inputs: every product and partial sum of the triple product is a multiple of 1/512 below
        2^15.  Otherwise 8 U P with P = sum_i |a_i| (|b_j c_k| + |b_k c_j|): two products and a difference per cross
        component (2 U of the absolute terms), the chain's 3 U, the inputs' 3 U.
      The angle of the vector (den, det) moves by at most the integral of |grad atan2| over the error box,
        (|det'| d_den + |den'| d_det) / r^2,  det' = |det| + d_det,  den' = |den| + d_den,
        r^2 = max(0, |det| - d_det)^2 + max(0, |den| - d_den)^2,
      which is the first-order 2 |det| d_den / (det^2 + den^2) of omega = 2 angle with its remainder kept; no statement
      (4 pi) where r = 0.
      atan2f: 6 ulp, the OpenCL full-profile bound that ocml follows, taken at the largest result: 6 x 2 U x 2 pi for
      omega.  The factor 2 is exact.
    ambiguous: det == 0 and den <= d_den.  The point lies on the triangle in its plane and omega is +-2 pi by the sign of
    a zero (or 0 when den rounds to the other side on an edge), in float64 as much as in f32.
    strictly_inside: the ambiguous pairs with den < -d_den, for which 0 is not admissible."""
    p = np.asarray(points, dtype=np.float64)[:, None, :]
    t = np.asarray(tris, dtype=np.float64)
    a, b, c = t[None, :, 0, :] - p, t[None, :, 1, :] - p, t[None, :, 2, :] - p
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    det = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    omega = 2.0 * np.arctan2(det, den)
    T = la * lb * lc
    k = 10.25 if exact_inputs else 13.25
    d_den = k * U * 4.0 * T
    if exact_inputs:
        d_det = np.zeros_like(det)
    else:
        aa, bb, cc = np.abs(a), np.abs(b), np.abs(c)
        perm = sum(aa[..., i] * (bb[..., (i + 1) % 3] * cc[..., (i + 2) % 3] + bb[..., (i + 2) % 3] * cc[..., (i + 1) % 3])
                   for i in range(3))
        d_det = 8.0 * U * perm
    r2 = np.maximum(0.0, np.abs(det) - d_det) ** 2 + np.maximum(0.0, np.abs(den) - d_den) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        ang = ((np.abs(det) + d_det) * d_den + (np.abs(den) + d_den) * d_det) / r2
    ang = np.where(r2 > 0, ang, 2.0 * np.pi)
    ang = np.where(T == 0, 0.0, ang)                       # p on a vertex: det = den = 0 exactly on both sides, omega = 0
    bound = np.minimum(2.0 * ang, 4.0 * np.pi) + 6.0 * 2.0 * U * 2.0 * np.pi
    ambiguous = (det == 0) & (den <= d_den) & (T > 0)
    return omega, bound, ambiguous, ambiguous & (den < -d_den)


def admissible_windings(omega, ambiguous, den_negative):
    """For one point: the winding numbers an evaluation may give when its ambiguous pairs take any admissible value:
    +-2 pi, and also 0 unless den is clearly negative (den_negative: strictly inside the triangle)."""
    base = omega[~ambiguous].sum()
    choices = [(-2.0 * np.pi, 2.0 * np.pi) if neg else (-2.0 * np.pi, 0.0, 2.0 * np.pi) for neg in den_negative[ambiguous]]
    return np.array([(base + sum(combo)) / (4.0 * np.pi) for combo in itertools.product(*choices)])


def trilinear_index(x, bound, R):
    """Continuous voxel index of coordinate x on a voxel-centre grid of R cells over [-bound, bound], clamped to the
    outermost centres: grid_sample(align_corners=False, padding_mode="border")."""
    return np.clip(((np.asarray(x, dtype=np.float64) / bound + 1.0) * R - 1.0) / 2.0, 0.0, R - 1.0)


def trilinear(vol, xyz, bound):
    """vol [R,R,R] indexed [z][y][x], xyz [n,3] -> [n] float64."""
    vol = np.asarray(vol, dtype=np.float64)
    R = vol.shape[0]
    u = trilinear_index(xyz, bound, R)
    i0 = np.minimum(np.floor(u).astype(np.int64), R - 2)
    f = u - i0
    out = np.zeros(u.shape[0])
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        wgt = (f[:, 0] if dx else 1 - f[:, 0]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 2] if dz else 1 - f[:, 2])
        out += wgt * vol[i0[:, 2] + dz, i0[:, 1] + dy, i0[:, 0] + dx]
    return out


def trilinear_f32_bound(vol, exact_coords):
    """How far an f32 trilinear read may be from trilinear(): three nested lerps are 8 U max|vol| (per lerp the two
    weights' roundings and the sum's, against values of at most max|vol|, less than 3 U; 3 x 3 rounded up to 8 as the
    last lerp's inputs already carry the rest).  Coordinates that are not exact in f32 add the index error: divide,
    add 1, times R, subtract 1 are 4 roundings of values below 2.5 R, halved: 5 U R per axis, each moving the result
    by at most the largest difference between axis neighbours: 15 U R max|diff|."""
    vol = np.asarray(vol, dtype=np.float64)
    tol = 8.0 * U * np.abs(vol).max()
    if not exact_coords:
        diff = max(np.abs(np.diff(vol, axis=ax)).max() for ax in range(3))
        tol += 15.0 * U * vol.shape[0] * diff
    return tol


def shape_loss(xyz, sigma, n_valid, w_grid, d_grid, bound, proximal_surface, delta, exact_coords=False):
    """ShapeLoss in float64 -> (loss, dloss_dsigma [cap], near_threshold [cap] bool); see shape_loss_terms."""
    terms, grad, near = shape_loss_terms(xyz, sigma, n_valid, w_grid, d_grid, bound, proximal_surface, delta, exact_coords)
    return terms.sum(), grad, near


def shape_loss_terms(xyz, sigma, n_valid, w_grid, d_grid, bound, proximal_surface, delta, exact_coords=False):
    """The per-sample terms of ShapeLoss in float64 -> (terms [cap], dloss_dsigma [cap], near_threshold [cap] bool).
        occ = clamp(1 - exp(-delta sigma), 0, 1.1);  q = 0.99 if winding > 0.5 else 0.01
        term = -(occ log q + (1 - occ) log(1 - q)) (1 - exp(-d^2 / (2 proximal_surface^2)))   [weight 1 if it is 0]
    over the first n_valid samples, winding and d by trilinear().  d term / d sigma = weight (log(1 - q) - log q) delta
    exp(-delta sigma) for sigma >= 0 and 0 below (the clamp).  near_threshold: the interpolated winding number is within
    trilinear_f32_bound of 0.5, so the indicator of an f32 evaluation may differ."""
    xyz, sigma = np.asarray(xyz, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    cap = sigma.shape[0]
    grad, near, terms = np.zeros(cap), np.zeros(cap, dtype=bool), np.zeros(cap)
    x, s = xyz[:n_valid], sigma[:n_valid]
    w = trilinear(w_grid, x, bound)
    near[:n_valid] = np.abs(w - 0.5) <= trilinear_f32_bound(w_grid, exact_coords)
    q = np.where(w > 0.5, 0.99, 0.01)
    e = np.exp(-delta * np.maximum(s, 0.0))
    occ = 1.0 - e
    weight = np.ones(n_valid)
    if proximal_surface > 0:
        d = trilinear(d_grid, x, bound)
        weight = 1.0 - np.exp(-(d * d) / (2.0 * proximal_surface ** 2))
    terms[:n_valid] = -(occ * np.log(q) + e * np.log(1.0 - q)) * weight
    grad[:n_valid] = weight * (np.log(1.0 - q) - np.log(q)) * delta * e * (s >= 0)
    return terms, grad, near


# ---------------------------------------------------------------------------------------------------------------------
# The cases of the tests, built here so that the CPU tests can check what share of each case a GPU test leaves out.
def lattice_points(rng, n):
    return (rng.integers(-16, 17, (n, 3)) / 8.0).astype(np.float32)


def lattice_triangles(rng, F, small=False):
    """F triangles with an area, vertices multiples of 1/8 in [-2, 2]; small: each within 3/8 of a base point."""
    def draw(k):
        if small:
            return (rng.integers(-13, 14, (k, 1, 3)) + rng.integers(-3, 4, (k, 3, 3))) / 8.0
        return rng.integers(-16, 17, (k, 3, 3)) / 8.0

    t = draw(F)
    while True:
        flat = np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=-1) == 0
        if not flat.any():
            return t.astype(np.float32)
        t[flat] = draw(int(flat.sum()))


DEGENERATE_FORMS = ("a==b", "a==c", "b==c", "a==b==c", "c before a-b", "c between a-b", "c beyond a-b", "b beyond a-c")


def degenerate_triangles(rng, per_form):
    """-> (tris [8 per_form, 3, 3] f32 on the lattice, form index [8 per_form], ends [8 per_form, 2, 3]): the eight
    zero-area forms, and the two ends of the segment (or point) each one is."""
    tris, form, ends = [], [], []
    for k in range(len(DEGENERATE_FORMS)):
        for _ in range(per_form):
            a = rng.integers(-4, 5, 3) / 8.0
            s = rng.integers(-3, 4, 3) / 8.0
            while not s.any():
                s = rng.integers(-3, 4, 3) / 8.0
            o = a + 2 * s
            t, e = {0: ((a, a, o), (a, o)), 1: ((a, o, a), (a, o)), 2: ((a, o, o), (a, o)), 3: ((a, a, a), (a, a)),
                    4: ((a, o, a - 2 * s), (a - 2 * s, o)), 5: ((a, o, a + s), (a, o)),
                    6: ((a, o, a + 4 * s), (a, a + 4 * s)), 7: ((a, a + 4 * s, o), (a, a + 4 * s))}[k]
            tris.append(t), form.append(k), ends.append(e)
    return np.array(tris, dtype=np.float32), np.array(form), np.array(ends, dtype=np.float64)


ICO_SCALE, ICO_SHIFT = np.array([0.5, 0.3, 0.2]), np.array([0.1, -0.15, 0.2])


def asymmetric_icosphere(subdiv):
    """The closed icosphere scaled (0.5, 0.3, 0.2) and shifted (0.1, -0.15, 0.2): no symmetry, so that a swapped axis
    shows.  -> triangles f32 [20 * 4^subdiv, 3, 3]."""
    from src.latent_nerf.training import shape as S
    verts, faces = S.make_icosphere(subdiv, 1.0)
    v = verts.numpy().astype(np.float64) * ICO_SCALE + ICO_SHIFT
    return v.astype(np.float32)[faces.numpy()]


def icosphere_radius(points):
    """|p| in the coordinates in which asymmetric_icosphere is the unit icosphere: its vertices are at 1."""
    return np.linalg.norm((np.asarray(points, dtype=np.float64) - ICO_SHIFT) / ICO_SCALE, axis=-1)


def loss_case(seed, R=16, cap=4096, n_valid=3000):
    """Inputs of the shape-loss test on which the f32 trilinear reads are exact, so that the operations of the loss
    formula are all that separates f32 from float64: bound 1, R = 16, grid values multiples of 1/16 (winding in
    [-0.25, 1.25], distance in [0, 2]) and coordinates multiples of 1/64 in [-1.25, 1.25] (index 8 x + 7.5: weights
    are multiples of 1/8, every product and partial sum a multiple of 2^-13 below 4).  The tail of xyz and sigma is NaN.
    Valid sigmas: exact 0, negative values, uniform (0, 10), and 600 / 1e4, whose exp(-0.2 sigma) underflows to 0."""
    rng = np.random.default_rng(seed)
    w_grid = (rng.integers(-4, 21, (R, R, R)) / 16.0).astype(np.float32)
    d_grid = (rng.integers(0, 33, (R, R, R)) / 16.0).astype(np.float32)
    xyz = np.full((cap, 3), np.nan, dtype=np.float32)
    xyz[:n_valid] = rng.integers(-80, 81, (n_valid, 3)) / 64.0
    sigma = np.full(cap, np.nan, dtype=np.float32)
    s = rng.uniform(0.0, 10.0, n_valid)
    kind = rng.integers(0, 10, n_valid)
    s[kind == 0] = 0.0
    s[kind == 1] = -rng.uniform(0.0, 50.0, int((kind == 1).sum()))
    s[kind == 2] = rng.choice([600.0, 1.0e4], int((kind == 2).sum()))
    sigma[:n_valid] = s
    return xyz, sigma, w_grid, d_grid
