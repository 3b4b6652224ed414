"""The sketch-shape path (BASELINE config 3) against float64 at its geometric edges: csrc/mesh.hip
(lnerf_mesh_distance, lnerf_mesh_winding_number) and src/latent_nerf/training/shape.py (MeshOccupancy, ShapeLoss).
References: tests/shape_reference.py (checked on its own by tests/test_shape_reference_cpu.py).

Every tolerance is a formula of the inputs, U = 2^-24, with its count of operations beside it.  Each test prints the
largest ratio of error to bound it saw.

Lattice inputs are multiples of 1/8 in [-2, 2]: differences are multiples of 1/8 up to 4, dot products multiples of
1/64 up to 48, their pairwise products multiples of 2^-12 up to 2304 < 2^24 2^-12: every dot product of tri_dist2, every
product in va, vb, vc and so every region decision is exact in f32, and a wrong branch cannot hide behind rounding."""
import os

import numpy as np
import pytest
import torch

from tests import shape_reference as SR
from tests.shape_reference import U

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shape_tiles_distance.npz")
PAD, SENTINEL = 64, -12345.0
TILE_F = (1, 255, 256, 257, 513)
TILE_N = (1, 255, 256, 257, 600)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _raw(name, dev, pts, tris):
    """The C entry point on its own output buffer of n + PAD sentinels -> (head [n], tail [PAD]) as numpy."""
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    p = torch.as_tensor(np.ascontiguousarray(pts, dtype=np.float32)).reshape(-1, 3).to(dev)
    t = torch.as_tensor(np.ascontiguousarray(tris, dtype=np.float32)).reshape(-1, 3, 3).to(dev)
    out = torch.full((p.shape[0] + PAD,), SENTINEL, device=dev)
    _b.call(name, _p(p), p.shape[0], _p(t) if t.shape[0] else None, t.shape[0], _p(out), _stream())
    out = out.cpu().numpy()
    return out[:p.shape[0]], out[p.shape[0]:]


def _distance(dev, pts, tris):
    d, tail = _raw("lnerf_mesh_distance", dev, pts, tris)
    assert (tail == SENTINEL).all()
    return d


def _winding(dev, pts, tris):
    w, tail = _raw("lnerf_mesh_winding_number", dev, pts, tris)
    assert (tail == SENTINEL).all()
    return w


# ---------------------------------------------------------------------------------------------------------------------
# distance
def _lattice_tol(pts, tris, d_ref):
    """[n, F]: 9 U (|ap| + |ab| + |ac|) + 4 U d_ref, for lattice inputs.
    The closest point: on an edge one quotient v of exact operands (U, |v| <= 1) and per component one product and one
    difference (2 U): 2 U (|ap| + |ab| + |ac|) covers it.  In the interior va, vb, vc are one rounded difference each
    (U), their sum two additions on top (3 U), the reciprocal and the product one each: v and w carry 6 U; per component
    two products and two differences: (6 + 1) U (|ab| + |ac|) + 2 U (|ap| + |ab|) <= 9 U (|ap| + |ab| + |ac|).  The
    distance is 1-Lipschitz in the closest point.  Then dot3(q, q) is 3 roundings of a sum of squares (1.5 U of the
    distance) and the root one more: below 4 U d."""
    p, t = pts.astype(np.float64)[:, None, :], tris.astype(np.float64)[None]
    L = np.linalg.norm(p - t[:, :, 0], axis=-1) + np.linalg.norm(t[:, :, 1] - t[:, :, 0], axis=-1) \
        + np.linalg.norm(t[:, :, 2] - t[:, :, 0], axis=-1)
    return 9 * U * L + 4 * U * d_ref


def _free_tol(pts, tris, d_ref):
    """[n, F] for inputs that are not on the lattice: 96 U (|ab| + |ac|) P^2 / (|ab| |ac| sin^2 A) + 8 U L + 4 U d_ref,
    P = max(|ap|, |bp|, |cp|), L = |ap| + |ab| + |ac|, A the angle at a.
    A difference of inputs carries U, a dot product e.x of two of them 2 U + the chain's 3 U = 5 U |e||x|.  vb (and va,
    vc) is a difference of two products of such: 2 (10 + 1) U S + U |vb| <= 23 U S with S = |ab||ac| P^2.  The sum
    D = va + vb + vc = |ab x ac|^2: 69 U S + 2 U D.  v = vb / D: (23 + 71) U S / D + 2 U, and S / D =
    P^2 / (|ab||ac| sin^2 A): a far point and a thin triangle are what the barycentric form is sensitive to.  The closest
    point moves by |ab| dv + |ac| dw plus the 4 U L of its own products and differences: 94 -> 96.  The edge and vertex
    regions are shorter chains of the same operands, and the cascade is continuous where a rounding changes the region."""
    p, t = pts.astype(np.float64)[:, None, :], tris.astype(np.float64)[None]
    a, b, c = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    lab, lac = np.linalg.norm(b - a, axis=-1), np.linalg.norm(c - a, axis=-1)
    P = np.maximum.reduce([np.linalg.norm(p - a, axis=-1), np.linalg.norm(p - b, axis=-1), np.linalg.norm(p - c, axis=-1)])
    sin2 = (np.linalg.norm(np.cross(b - a, c - a), axis=-1) / (lab * lac)) ** 2
    L = np.linalg.norm(p - a, axis=-1) + lab + lac
    return 96 * U * (lab + lac) * P * P / (lab * lac * sin2) + 8 * U * L + 4 * U * d_ref


def _check_min(d_gpu, d_ref, tol):
    """min over f of values each within tol[f] of d_ref[f]: at most d_ref[f*] + tol[f*] at the reference's argmin, at
    least the smallest d_ref[f] - tol[f].  -> largest ratio of the excess to the tolerance at the argmin."""
    k = d_ref.argmin(-1)
    rows = np.arange(d_ref.shape[0])
    hi, lo = d_ref[rows, k] + tol[rows, k], (d_ref - tol).min(-1)
    assert np.isfinite(d_gpu).all()
    assert (d_gpu <= hi).all() and (d_gpu >= lo).all(), float(np.abs(d_gpu - d_ref[rows, k]).max())
    return float((np.abs(d_gpu - d_ref[rows, k]) / tol[rows, k]).max())


@pytest.fixture(scope="module")
def lattice():
    rng = np.random.default_rng(0)
    tris, pts = SR.lattice_triangles(rng, 60), SR.lattice_points(rng, 500)
    assert SR.on_lattice(tris) and SR.on_lattice(pts)
    d, region = SR.point_triangle(pts, tris)
    return tris, pts, d, region


def test_distance_per_pair_in_every_region_on_the_lattice(dev, lattice):
    tris, pts, d_ref, region = lattice
    assert min((region == k).mean() for k in range(7)) >= 0.03
    d = np.stack([_distance(dev, pts, tris[f:f + 1]) for f in range(tris.shape[0])], axis=1)
    assert np.isfinite(d).all()
    tol = _lattice_tol(pts, tris, d_ref)
    ratio = np.abs(d - d_ref) / tol
    print("distance, lattice pairs: max |err| / bound per region",
          {SR.REGIONS[k]: float(ratio[region == k].max()) for k in range(7)}, "bound up to %.2e" % tol.max())
    for k in range(7):
        assert (ratio[region == k] <= 1).all(), SR.REGIONS[k]
    # a vertex region: d^2 = |p - vertex|^2 is a multiple of 1/64 below 2^10, exact; only the root rounds
    vertex = region <= SR.R_C
    corner = tris.astype(np.float64)[np.arange(tris.shape[0])[None, :], np.where(vertex, region, 0)]      # [n, F, 3]
    d2 = ((pts.astype(np.float64)[:, None, :] - corner) ** 2).sum(-1)
    want = np.sqrt(d2).astype(np.float32)
    assert (np.abs(d - want)[vertex] <= np.spacing(want)[vertex]).all()


def test_distance_is_zero_on_vertices_edge_midpoints_and_centroids(dev, lattice):
    tris = lattice[0]
    t = tris.astype(np.float64)
    feats = np.concatenate([t, (t + np.roll(t, 1, axis=1)) / 2, t.mean(1, keepdims=True)], axis=1).astype(np.float32)  # [F,7,3]
    worst = 0.0
    for f in range(tris.shape[0]):
        d = _distance(dev, feats[f], tris[f:f + 1])
        d_ref, _ = SR.point_triangle(feats[f], tris[f:f + 1])          # 0, but for the centroid's own f32 rounding
        tol = _lattice_tol(feats[f], tris[f:f + 1], d_ref)[:, 0]
        assert np.isfinite(d).all() and d_ref.max() < 4 * U * 4
        assert (np.abs(d - d_ref[:, 0]) <= tol).all(), (f, d)
        assert (d[:6] == 0).all()                                      # vertices and midpoints are exact in f32
        worst = max(worst, float((np.abs(d - d_ref[:, 0]) / tol).max()))
    print("distance, on features: max |err| / bound %.3f" % worst)


def test_distance_to_zero_area_triangles_is_the_segment_distance(dev):
    """The eight zero-area forms, each alone (F == 1) and mixed into a 257-triangle soup.  a == b used to give 0 / 0 in
    the edge-AB quotient: a NaN that fminf drops, so the triangle vanished (sqrt(3e38) when it was alone)."""
    rng = np.random.default_rng(11)
    flat, form, _ = SR.degenerate_triangles(rng, 4)
    pts = SR.lattice_points(rng, 200)
    d_ref, _ = SR.point_triangle(pts, flat)
    tol = _lattice_tol(pts, flat, d_ref)
    worst = {}
    for f in range(flat.shape[0]):
        d = _distance(dev, pts, flat[f:f + 1])
        name = SR.DEGENERATE_FORMS[form[f]]
        assert np.isfinite(d).all() and (d < 1e3).all(), name
        assert (np.abs(d - d_ref[:, f]) <= tol[:, f]).all(), (name, float(np.abs(d - d_ref[:, f]).max()))
        worst[name] = max(worst.get(name, 0.0), float((np.abs(d - d_ref[:, f]) / tol[:, f]).max()))
    print("distance, zero-area forms alone: max |err| / bound", worst)
    soup = np.concatenate([SR.lattice_triangles(rng, 257 - flat.shape[0], small=True), flat])
    soup = soup[rng.permutation(257)]
    pts = (rng.integers(-8, 9, (200, 3)) / 8.0).astype(np.float32)        # where the zero-area ones are
    d_ref, _ = SR.point_triangle(pts, soup)
    is_flat = np.linalg.norm(np.cross(soup[:, 1] - soup[:, 0], soup[:, 2] - soup[:, 0]), axis=-1) == 0
    assert is_flat.sum() == flat.shape[0] and is_flat[d_ref.argmin(-1)].sum() >= 10        # they decide some of the minima
    print("distance, zero-area forms in a soup of 257: max |err| / bound %.3f"
          % _check_min(_distance(dev, pts, soup), d_ref, _lattice_tol(pts, soup, d_ref)))


# ---------------------------------------------------------------------------------------------------------------------
# tiles and tails
def _tile_case(F):
    rng = np.random.default_rng(100 + F)
    tris = rng.uniform(-1, 1, (F, 3, 3)).astype(np.float32)
    pts = rng.uniform(-1.2, 1.2, (max(TILE_N), 3)).astype(np.float32)
    return tris, pts


@pytest.mark.parametrize("F", TILE_F)
def test_tiles_and_tails_of_both_kernels(dev, F):
    """LDS tiles of 256 triangles and blocks of 256 points, one below, at and one above; the output's tail stays
    untouched (_distance / _winding assert it).  The distances of triangles with an area are bit for bit those of the
    build before tri_dist2 learnt about zero-area triangles (tests/golden/shape_tiles_distance.npz, written by that build
    on an MI355X from _tile_case; tri_dist2 is f32 + - * / fma sqrt only, so the bits do not depend on a math library)."""
    tris, pts = _tile_case(F)
    d_ref, _ = SR.point_triangle(pts, tris)
    tol_d = _free_tol(pts, tris, d_ref)
    omega, bound, amb = SR.solid_angles(pts, tris)
    assert not amb.any()
    w_ref = omega.sum(-1) / (4 * np.pi)
    tol_w = _winding_tol(omega, bound, F)
    golden = np.load(GOLDEN)
    worst_d = worst_w = 0.0
    for n in TILE_N:
        d = _distance(dev, pts[:n], tris)
        worst_d = max(worst_d, _check_min(d, d_ref[:n], tol_d[:n]))
        assert np.array_equal(d.view(np.uint32), golden["F%d_n%d" % (F, n)].view(np.uint32)), (F, n)
        w = _winding(dev, pts[:n], tris)
        assert np.isfinite(w).all() and (np.abs(w - w_ref[:n]) <= tol_w[:n]).all(), (F, n)
        worst_w = max(worst_w, float((np.abs(w - w_ref[:n]) / tol_w[:n]).max()))
    print("tiles F=%d: distance max |err| / bound %.4f, winding %.4f" % (F, worst_d, worst_w))


def test_empty_inputs(dev):
    from src.latent_nerf.raymarching.backend import LnerfError
    tris, pts = _tile_case(257)
    for name in ("lnerf_mesh_distance", "lnerf_mesh_winding_number"):
        head, tail = _raw(name, dev, pts[:0], tris)                    # n == 0 writes nothing
        assert head.size == 0 and (tail == SENTINEL).all()
    w, tail = _raw("lnerf_mesh_winding_number", dev, pts[:300], tris[:0])
    assert (w == 0).all() and not np.signbit(w).any() and (tail == SENTINEL).all()
    with pytest.raises(LnerfError, match=r"lnerf_mesh_distance failed \(-1\): mesh_distance: need at least one triangle"):
        _raw("lnerf_mesh_distance", dev, pts[:300], tris[:0])


# ---------------------------------------------------------------------------------------------------------------------
# winding number
def _winding_tol(omega, bound, F):
    """[n]: (sum_f bound + F U max|partial sum|) / 4 pi.  The kernel adds F solid angles in order, F - 1 additions each
    rounding the partial sum it produces, and multiplies by 1 / (4 pi) once; the partial sums are the reference's, at most
    sum_f bound away."""
    return (bound.sum(-1) + F * U * (np.abs(np.cumsum(omega, -1)).max(-1) + bound.sum(-1))) / (4 * np.pi)


def test_winding_number_on_the_lattice(dev):
    """257 triangles, 600 points.  |w - w_ref| <= (sum_f bound + F U max|partial sum|) / 4 pi.  A point that lies on a
    triangle in its plane is left out of that (at most 10 % are), but must still get one of the values the sign of a zero
    can give: the pair at +2 pi or -2 pi, or 0 when the point is on the triangle's border."""
    rng = np.random.default_rng(5)
    tris, pts = SR.lattice_triangles(rng, 257), SR.lattice_points(rng, 600)
    assert SR.on_lattice(tris) and SR.on_lattice(pts)
    omega, bound, amb, strict = SR.solid_angle_parts(pts, tris, exact_inputs=True)
    touched = amb.any(-1)
    assert touched.sum() <= 0.10 * 600
    w = _winding(dev, pts, tris)
    assert np.isfinite(w).all()
    clean = np.where(amb, 0.0, omega)
    tol = _winding_tol(clean, np.where(amb, 0.0, bound), 257) + 2 * U * amb.sum(-1)     # the pair's own 2 pi, rounded
    w_ref = clean.sum(-1) / (4 * np.pi)
    ok = ~touched
    assert (np.abs(w - w_ref)[ok] <= tol[ok]).all(), float(np.abs(w - w_ref)[ok].max())
    for i in np.nonzero(touched)[0]:
        cand = SR.admissible_windings(omega[i], amb[i], strict[i])
        assert np.abs(cand - w[i]).min() <= tol[i], (i, float(w[i]), cand)
    print("winding, lattice: max |err| / bound %.4f (bound up to %.2e), %d of 600 points on a triangle"
          % (float((np.abs(w - w_ref) / tol)[ok].max()), tol[ok].max(), int(touched.sum())))


def test_winding_number_of_zero_area_triangles_is_zero(dev):
    """On the lattice the triple product of a zero-area triangle is an exact 0, so its solid angle is 2 atan2(0, den) = 0
    wherever den > 0: everywhere but on the segment itself (the ambiguous pairs)."""
    rng = np.random.default_rng(11)
    flat, _, _ = SR.degenerate_triangles(rng, 4)
    pts = SR.lattice_points(rng, 200)
    omega, _, amb = SR.solid_angles(pts, flat, exact_inputs=True)
    assert not omega[~amb].any() and amb.any(-1).sum() <= 0.10 * 200
    w = _winding(dev, pts, flat)
    assert (w[~amb.any(-1)] == 0).all()
    for f in range(flat.shape[0]):
        assert (_winding(dev, pts, flat[f:f + 1])[~amb[:, f]] == 0).all()


@pytest.mark.parametrize("subdiv", [1, 3])
def test_winding_number_of_a_closed_surface(dev, subdiv):
    """The icosphere of 80 and of 1280 faces, scaled (0.5, 0.3, 0.2) and shifted: 1 inside, 0 outside, at random points,
    1e-3 either side of every 8th face's centroid, and far away (|p| = 50)."""
    rng = np.random.default_rng(20 + subdiv)
    tris = SR.asymmetric_icosphere(subdiv)
    F = tris.shape[0]
    assert F in (80, 1280)
    t = tris.astype(np.float64)
    nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    assert ((t.mean(1) - SR.ICO_SHIFT) * nrm).sum(-1).min() > 0         # outward
    near_out, near_in = (t.mean(1) + 1e-3 * nrm)[::8], (t.mean(1) - 1e-3 * nrm)[::8]
    far = rng.normal(size=(40, 3))
    far = 50.0 * far / np.linalg.norm(far, axis=-1, keepdims=True)
    free = rng.uniform(-1.5, 1.5, (300, 3)) * SR.ICO_SCALE + SR.ICO_SHIFT
    r = SR.icosphere_radius(free)
    free = free[(r < 0.85) | (r > 1.001)]
    pts = np.concatenate([near_out, near_in, far, free]).astype(np.float32)
    want = np.concatenate([np.zeros(len(near_out)), np.ones(len(near_in)), np.zeros(40), SR.icosphere_radius(free) < 0.85])
    omega, bound, amb = SR.solid_angles(pts, tris)
    assert not amb.any() and np.abs(omega.sum(-1) / (4 * np.pi) - want).max() < 1e-9 and 10 < want.sum() < len(want) - 10
    tol = _winding_tol(omega, bound, F)
    w = _winding(dev, pts, tris)
    assert (np.abs(w - want) <= tol).all(), float(np.abs(w - want).max())
    print("winding, closed surface F=%d: max |err| / bound %.4f (bound up to %.2e)"
          % (F, float((np.abs(w - want) / tol).max()), tol.max()))


# ---------------------------------------------------------------------------------------------------------------------
# grids and look-ups
def _ico80(dev, bound, R=16):
    from src.latent_nerf.training import shape as S
    tris = SR.asymmetric_icosphere(1)
    verts = torch.from_numpy(tris.reshape(-1, 3))
    faces = torch.arange(verts.shape[0]).reshape(-1, 3)
    return tris, S.MeshOccupancy(verts, faces, dev, bound=bound, resolution=R)


@pytest.mark.parametrize("bound", [1.0, 2.0])
def test_mesh_occupancy_grids_and_trilinear_look_ups(dev, bound):
    R = 16
    tris, occ = _ico80(dev, bound, R)
    assert occ.winding.shape == (1, 1, R, R, R) and occ.dist.shape == (1, 1, R, R, R)
    wg, dg = occ.winding[0, 0].cpu().numpy(), occ.dist[0, 0].cpu().numpy()
    lin = ((np.arange(R) + 0.5) / R * 2 - 1) * bound                       # exact in f32 and in float64
    zz, yy, xx = np.meshgrid(lin, lin, lin, indexing="ij")
    centres = np.stack([xx, yy, zz], -1).reshape(-1, 3)                    # voxel [z][y][x] holds the value at (x, y, z)
    omega, sa_bound, amb = SR.solid_angles(centres, tris)
    assert not amb.any()
    w_ref, tol_w = omega.sum(-1) / (4 * np.pi), _winding_tol(omega, sa_bound, 80)
    assert (np.abs(wg.reshape(-1) - w_ref) <= tol_w).all()
    d_ref, _ = SR.point_triangle(centres, tris)
    ratio_d = _check_min(dg.reshape(-1), d_ref, _free_tol(centres, tris, d_ref))
    print("grids bound=%g: winding max |err| / bound %.4f, distance %.4f"
          % (bound, float((np.abs(wg.reshape(-1) - w_ref) / tol_w).max()), ratio_d))
    assert 4 < (w_ref > 0.5).sum() < R ** 3 // 2

    # look-ups.  2000 points whose coordinates are multiples of bound / 64: the index 8 x / bound + 7.5 and the weights are
    # exact in f32, so 8 U max|vol| (three nested lerps) is the whole error.  Among them the corners of the box, points on
    # its faces (+-bound), points outside it and 200 voxel centres.  Then 1000 free f32 points, whose index carries its own
    # roundings (trilinear_f32_bound counts them).
    rng = np.random.default_rng(31)
    n_exact = 2000
    exact = rng.integers(-80, 81, (n_exact, 3)) * (bound / 64.0)
    exact[:64] = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)] * 8) * bound
    exact[8:64, 1] = rng.integers(-80, 81, 56) * (bound / 64.0)
    pick = rng.choice(R ** 3, 200, replace=False)
    exact[64:264] = centres[pick]
    assert (np.abs(exact) > bound).any(-1).sum() > 100
    free = rng.uniform(-1.25, 1.25, (1000, 3)).astype(np.float32).astype(np.float64) * bound
    xyz = np.concatenate([exact, free]).astype(np.float32)
    assert np.array_equal(xyz[:n_exact].astype(np.float64), exact)
    xyz_dev = torch.from_numpy(xyz).to(dev)
    for name, vol, got in (("winding", wg, occ.winding_at(xyz_dev)), ("distance", dg, occ.distance_at(xyz_dev))):
        got = got.cpu().numpy()
        ref = SR.trilinear(vol, xyz, bound)
        tol = np.concatenate([np.full(n_exact, SR.trilinear_f32_bound(vol, True)),
                              np.full(1000, SR.trilinear_f32_bound(vol, False))])
        assert (np.abs(got - ref) <= tol).all(), (name, float(np.abs(got - ref).max()))
        assert np.array_equal(got[64:264], vol.reshape(-1)[pick]), name                 # a centre reads its voxel
        swapped = SR.trilinear(vol, xyz[:, ::-1], bound)
        assert np.abs(swapped - got).max() > 1000 * tol.max(), name                     # a transposed axis would show
        ratio = np.abs(got - ref) / tol
        print("look-ups bound=%g %s: max |err| / bound exact %.3f free %.3f; x <-> z moves it by %.2e, bound %.2e"
              % (bound, name, float(ratio[:n_exact].max()), float(ratio[n_exact:].max()), np.abs(swapped - got).max(),
                 tol.max()))


def test_occupancy_seed_on_two_cascades(dev):
    from oracle import nerf_oracle as O
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    G = 32
    tris, occ = _ico80(dev, 2.0)
    net = NeRFNetwork(RenderConfig(grid_size=G, bound=2.0, train_h=16, train_w=16), log2_hashmap_size=12).to(dev)
    assert net.cascade == 2 and net.density_grid.shape == (2, G ** 3)
    bits = occ.init_density_grid(net).cpu()
    grid = net.density_grid.cpu()
    val = np.float32(2.0 * net.density_thresh)
    assert set(grid.unique().tolist()) == {0.0, float(val)}
    idx = torch.arange(G ** 3)
    skipped = 0
    for cas in range(2):
        xyz = O.occupancy_cell_points(idx, cas, G, 2.0, None).numpy()
        omega, bound, amb = SR.solid_angles(xyz, tris)
        w, tol = omega.sum(-1) / (4 * np.pi), _winding_tol(omega, bound, 80)
        clear = (np.abs(w - 0.5) > tol) & ~amb.any(-1)
        skipped += int((~clear).sum())
        assert np.array_equal((grid[cas].numpy() > 0)[clear], (w > 0.5)[clear]), cas
        assert (w > 0.5).sum() > 50
    assert skipped <= 0.02 * 2 * G ** 3
    mean = float(net.mean_density_dev.cpu()[0])
    want = grid.double().mean().item()
    assert abs(mean - want) <= 1e-6 * want and want > 0
    assert torch.equal(bits, O.packbits(grid.reshape(-1), min(net.density_thresh, mean)))
    print("occupancy seed: %d of %d cells within the reference's bound of 0.5" % (skipped, 2 * G ** 3))


# ---------------------------------------------------------------------------------------------------------------------
# shape loss
@pytest.mark.parametrize("proximal_surface", [0.3, 0.0])
@pytest.mark.parametrize("with_counter", [True, False])
def test_shape_loss_and_its_gradient(dev, proximal_surface, with_counter):
    """Capacity 4096, 3000 valid, NaN behind them (with counter=None: the 3000 alone).  The inputs are
    shape_reference.loss_case: the f32 trilinear reads are exact on them, so what is compared is the loss formula.
    d loss / d sigma per sample: 16 U |value| -- delta sigma (one product, delta itself rounded to f32: 1.5 U delta sigma
    <= 3 U of the exponential for sigma <= 10), exp (2 U), the weight's d^2, quotient by the rounded 2 p^2, expm1 (2 U)
    with its condition <= 1: 6 U, the two logarithms' difference 2 U, three products 3 U -- plus 2^-126, below which f32
    has no relative precision (exp(-0.2 sigma) underflows for the largest sigmas).
    The loss: a sum of n f32 terms in any order, n U sum|term|, which also covers the terms' own roundings (16 U each)."""
    from src.latent_nerf.training import shape as S
    delta, n_valid = 0.2, 3000
    xyz, sigma, w_grid, d_grid = SR.loss_case(7)
    if not with_counter:
        xyz, sigma = xyz[:n_valid], sigma[:n_valid]
    terms, g_ref, near = SR.shape_loss_terms(xyz, sigma, n_valid, w_grid, d_grid, 1.0, proximal_surface, delta, exact_coords=True)
    assert near.sum() <= 0.02 * n_valid
    _, occ = _ico80(dev, 1.0)
    occ.winding, occ.dist = (torch.from_numpy(v).to(dev).reshape(1, 1, 16, 16, 16) for v in (w_grid, d_grid))
    x = torch.from_numpy(xyz).to(dev)
    s = torch.from_numpy(sigma).to(dev).requires_grad_()
    counter = torch.tensor([n_valid, 7, 0, 0], dtype=torch.int32, device=dev) if with_counter else None
    loss = S.ShapeLoss(occ, proximal_surface=proximal_surface, delta=delta)(x, s, counter)
    loss.backward()
    g = s.grad.cpu().numpy().astype(np.float64)
    assert np.isfinite(float(loss.detach())) and np.isfinite(g).all()
    assert not g[n_valid:].any() and not np.signbit(g[n_valid:]).any()
    tol_sum = n_valid * U * np.abs(terms).sum()
    assert abs(float(loss.detach()) - terms.sum()) <= tol_sum
    tol_g = 16 * U * np.abs(g_ref) + 2.0 ** -126
    keep = ~near
    assert (np.abs(g - g_ref)[keep] <= tol_g[keep]).all(), float((np.abs(g - g_ref) / tol_g)[keep].max())
    dead = (sigma[:n_valid] < 0) | (sigma[:n_valid] >= 600)
    assert (g[:n_valid][dead] == 0).all() and (g[:n_valid][sigma[:n_valid] == 0] != 0).mean() > 0.9
    print("shape loss p=%g counter=%s: loss |err| / bound %.2e, gradient max |err| / bound %.3f, %d samples on the threshold"
          % (proximal_surface, with_counter, abs(float(loss.detach()) - terms.sum()) / tol_sum,
             float((np.abs(g - g_ref) / tol_g)[keep].max()), int(near.sum())))
