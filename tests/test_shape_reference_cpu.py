"""The float64 references of the sketch-shape tests (tests/shape_reference.py) checked without a GPU: against brute
force, against independent formulations, against torch in float64, and the share of each case that the GPU tests
(tests/test_gpu_shape.py) leave out because the reference itself cannot decide it."""
import numpy as np
import pytest
import torch

from oracle import mesh_oracle as MO
from oracle import nerf_oracle as O
from tests import shape_reference as SR


def _segment_distance(p, e0, e1):
    """|p - segment| written without a clamp: the end when the projection falls outside, else Pythagoras."""
    out = np.zeros((p.shape[0], e0.shape[0]))
    for j in range(e0.shape[0]):
        v, e = p - e0[j], e1[j] - e0[j]
        L2 = e @ e
        s = v @ e
        perp2 = np.maximum((v * v).sum(-1) - (s * s) / L2, 0.0) if L2 > 0 else (v * v).sum(-1)
        out[:, j] = np.sqrt(np.where(s <= 0, (v * v).sum(-1), np.where(s >= L2, ((p - e1[j]) ** 2).sum(-1), perp2)))
    return out


@pytest.fixture(scope="module")
def degenerate():
    rng = np.random.default_rng(11)
    tris, form, ends = SR.degenerate_triangles(rng, 4)
    return tris, form, ends, SR.lattice_points(rng, 200)


def test_point_triangle_equals_brute_force_over_a_dense_sampling(degenerate):
    """200^2 barycentric samples of each triangle: the smallest sample distance is never below the reference and exceeds
    it by at most the sampling pitch (the longest edge / 199: every point of the triangle is that close to a sample)."""
    rng = np.random.default_rng(1)
    tris = np.concatenate([SR.lattice_triangles(rng, 6), rng.uniform(-1, 1, (4, 3, 3)).astype(np.float32),
                           degenerate[0][::4]]).astype(np.float64)
    pts = np.concatenate([SR.lattice_points(rng, 30), rng.uniform(-2, 2, (10, 3))]).astype(np.float64)
    d, _ = SR.point_triangle(pts, tris)
    s = np.arange(200) / 199.0
    v, w = np.meshgrid(s, s, indexing="ij")
    keep = v + w <= 1 + 1e-12
    v, w = v[keep], w[keep]
    for f, (a, b, c) in enumerate(tris):
        q = a + v[:, None] * (b - a) + w[:, None] * (c - a)
        brute = np.sqrt(((pts[:, None, :] - q[None]) ** 2).sum(-1)).min(1)
        pitch = max(np.linalg.norm(b - a), np.linalg.norm(c - a), np.linalg.norm(c - b)) / 199.0
        assert (brute - d[:, f] >= -1e-12).all() and (brute - d[:, f] <= pitch + 1e-12).all(), f


def test_point_triangle_equals_the_oracle_distance(degenerate):
    """oracle.mesh_oracle.distance (plane projection and same-side tests) is a different formulation: both agree to
    float64 rounding, on triangles with an area and, since the oracle treats zero-area ones as segments, on those too."""
    rng = np.random.default_rng(2)
    pts = np.concatenate([SR.lattice_points(rng, 300), rng.uniform(-2, 2, (100, 3)).astype(np.float32)])
    for tris in (SR.lattice_triangles(rng, 60), rng.uniform(-1, 1, (60, 3, 3)).astype(np.float32), degenerate[0]):
        d, _ = SR.point_triangle(pts, tris)
        for f in range(0, tris.shape[0], 7):
            assert np.abs(d[:, f] - MO.distance(pts, tris[f:f + 1])).max() < 1e-12
        assert np.abs(d.min(-1) - MO.distance(pts, tris)).max() < 1e-12


def test_every_region_holds_its_share_of_the_lattice_case():
    rng = np.random.default_rng(0)
    tris, pts = SR.lattice_triangles(rng, 60), SR.lattice_points(rng, 500)
    assert SR.on_lattice(tris) and SR.on_lattice(pts)
    _, region = SR.point_triangle(pts, tris)
    share = [float((region == k).mean()) for k in range(7)]
    assert min(share) >= 0.03, dict(zip(SR.REGIONS, share))


def test_zero_area_triangles_are_their_segments(degenerate):
    tris, form, ends, pts = degenerate
    assert sorted(set(form.tolist())) == list(range(8))
    assert (np.linalg.norm(np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]), axis=-1) == 0).all()
    d, region = SR.point_triangle(pts, tris)
    ref = _segment_distance(pts.astype(np.float64), ends[:, 0], ends[:, 1])
    assert np.isfinite(d).all() and np.abs(d - ref).max() < 1e-12
    assert (region != SR.R_IN).all()
    point = form == 3
    to_a = np.linalg.norm(pts.astype(np.float64)[:, None, :] - tris.astype(np.float64)[None, point, 0, :], axis=-1)
    assert np.abs(d[:, point] - to_a).max() < 1e-15 and to_a.max() > 1      # a == b == c is the point a, not distance 0


def _box():
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float64)
    v = v * np.array([0.9, 0.5, 0.7]) - np.array([0.3, 0.2, 0.4])
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # outward
    f = [(q[0], q[k], q[k + 1]) for q in quads for k in (1, 2)]
    return v[np.array(f)]


def test_solid_angles_of_closed_surfaces_sum_to_one_inside_and_zero_outside():
    rng = np.random.default_rng(3)
    box = _box()
    pts = rng.uniform(-1, 1, (400, 3))
    lo, hi = box.reshape(-1, 3).min(0), box.reshape(-1, 3).max(0)
    clear = (np.abs(pts - lo).min(-1) > 1e-3) & (np.abs(pts - hi).min(-1) > 1e-3)
    inside = ((pts > lo) & (pts < hi)).all(-1)
    w = SR.solid_angles(pts, box)[0].sum(-1) / (4 * np.pi)
    assert inside[clear].sum() > 5 and np.abs(w[clear] - inside[clear]).max() < 1e-12
    for subdiv in (1, 2):
        tris = SR.asymmetric_icosphere(subdiv).astype(np.float64)
        # in the sphere's own coordinates the polyhedron lies between the radii 0.85 (inside every face of the 80-face
        # one) and 1 (its vertices; f32 rounding of them stays below the margin)
        ico = rng.uniform(-1.5, 1.5, (400, 3)) * SR.ICO_SCALE + SR.ICO_SHIFT
        r = SR.icosphere_radius(ico)
        w = SR.solid_angles(ico, tris)[0].sum(-1) / (4 * np.pi)
        assert (r < 0.85).sum() > 20 and (r > 1.001).sum() > 20
        assert np.abs(w[r < 0.85] - 1).max() < 1e-12 and np.abs(w[r > 1.001]).max() < 1e-12


def test_solid_angle_bound_covers_an_f32_evaluation():
    """The bound against the expression evaluated in numpy f32 (dot products as plain sums, so not the kernel's
    roundings, but the same count of them), lattice and free inputs."""
    rng = np.random.default_rng(4)
    for exact in (True, False):
        if exact:
            tris, pts = SR.lattice_triangles(rng, 100), SR.lattice_points(rng, 300)
        else:
            tris, pts = rng.uniform(-1, 1, (100, 3, 3)).astype(np.float32), rng.uniform(-1, 1, (300, 3)).astype(np.float32)
        omega, bound, amb = SR.solid_angles(pts, tris, exact_inputs=exact)
        a, b, c = (tris[None, :, k] - pts[:, None] for k in range(3))
        assert a.dtype == np.float32
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        om32 = np.float32(2) * np.arctan2(det, den)
        assert om32.dtype == np.float32
        ok = ~amb
        assert (np.abs(om32 - omega)[ok] <= bound[ok]).all()
        assert np.median(bound[ok]) < 1e-5            # and it is a statement: far below the values it bounds


def test_ambiguous_pairs_are_rare_on_the_lattice_case():
    rng = np.random.default_rng(5)
    tris, pts = SR.lattice_triangles(rng, 257), SR.lattice_points(rng, 600)
    _, _, amb, strict = SR.solid_angle_parts(pts, tris, exact_inputs=True)
    touched = amb.any(-1)
    assert 0 < touched.sum() <= 0.10 * 600, int(touched.sum())
    assert amb.sum(-1).max() <= 4 and not (strict & ~amb).any()


def test_trilinear_equals_grid_sample_in_float64():
    rng = np.random.default_rng(6)
    vol = rng.normal(size=(5, 5, 5))
    for bound in (1.0, 2.0):
        pts = rng.uniform(-1.3, 1.3, (500, 3)) * bound
        edge = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 0.3, 1) for sz in (-1, 1)]) * bound
        lin = ((np.arange(5) + 0.5) / 5 * 2 - 1) * bound
        centres = np.stack(np.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)[:, ::-1]   # (x, y, z), z slowest
        xyz = np.concatenate([pts, edge, centres])
        got = SR.trilinear(vol, xyz, bound)
        g = torch.from_numpy(xyz / bound).reshape(1, 1, 1, -1, 3)
        ref = torch.nn.functional.grid_sample(torch.from_numpy(vol)[None, None], g, mode="bilinear", padding_mode="border",
                                              align_corners=False).reshape(-1).numpy()
        assert np.abs(got - ref).max() < 1e-14
        assert np.array_equal(got[-125:], vol.reshape(-1))       # a voxel centre reads its voxel, [z][y][x]


@pytest.mark.parametrize("proximal_surface", [0.3, 0.0])
def test_shape_loss_derivative_equals_float64_autograd(proximal_surface):
    xyz, sigma, w_grid, d_grid = SR.loss_case(7)
    n_valid, delta = 3000, 0.2
    loss, grad, near = SR.shape_loss(xyz, sigma, n_valid, w_grid, d_grid, 1.0, proximal_surface, delta, exact_coords=True)
    x = torch.from_numpy(xyz[:n_valid].astype(np.float64))
    s = torch.from_numpy(sigma[:n_valid].astype(np.float64)).requires_grad_()

    def sample(vol):
        return torch.nn.functional.grid_sample(torch.from_numpy(vol.astype(np.float64))[None, None], x.reshape(1, 1, 1, -1, 3),
                                               mode="bilinear", padding_mode="border", align_corners=False).reshape(-1)

    inside = (sample(w_grid) > 0.5).double()
    occ = (1.0 - torch.exp(-delta * s)).clamp(0.0, 1.1)
    ce = -(occ * torch.log(inside.clamp(0.01, 0.99)) + (1.0 - occ) * torch.log((1.0 - inside).clamp(0.01, 0.99)))
    if proximal_surface > 0:
        ce = ce * (1.0 - torch.exp(-sample(d_grid) ** 2 / (2.0 * proximal_surface ** 2)))
    ce.sum().backward()
    assert abs(loss - float(ce.detach().sum())) <= 1e-12 * float(ce.detach().abs().sum())
    assert np.abs(grad[:n_valid] - s.grad.numpy()).max() < 1e-14 and not grad[n_valid:].any()
    assert (sigma[:n_valid] == 0).sum() > 100 and (sigma[:n_valid] < 0).sum() > 100 and (sigma[:n_valid] >= 600).sum() > 100
    assert near.sum() <= 0.02 * n_valid and not near[n_valid:].any()          # the share the GPU test leaves out


def test_occupancy_seed_reference_decides_nearly_every_cell():
    """The cells of both cascades (G = 32, bound 2) whose reference winding number is within its own bound of 0.5 are what
    the GPU test of init_density_grid cannot judge: at most 2 %."""
    tris = SR.asymmetric_icosphere(1)
    G = 32
    idx = torch.arange(G ** 3)
    for cas in range(2):
        xyz = O.occupancy_cell_points(idx, cas, G, 2.0, None).numpy()
        omega, bound, amb = SR.solid_angles(xyz, tris)
        w, tol = omega.sum(-1) / (4 * np.pi), (bound.sum(-1) + 80 * SR.U * np.abs(np.cumsum(omega, -1)).max(-1)) / (4 * np.pi)
        undecided = (np.abs(w - 0.5) <= tol) | amb.any(-1)
        assert undecided.mean() <= 0.02, (cas, float(undecided.mean()))
        assert (w > 0.5).sum() > 50
