"""Mesh export without a GPU: the generated marching-cubes tables (tools/gen_mc_tables.py -> csrc/mc_tables.h) are
current and crack-free by construction, the numpy restatement of lnerf_marching_cubes (tests/mc_reference.py) gives
closed, consistently oriented 2-manifolds, and the OBJ writer round-trips through the Latent-Paint reader."""
import collections
import os

import numpy as np
import pytest

from tests import mc_reference as R

GEN = R.load_generator()
TABS = GEN.tables()


def _on_face(e0, e1):
    return bool(GEN.edge_faces(e0) & GEN.edge_faces(e1))


def test_generator_reproduces_committed_header():
    with open(GEN.HEADER) as f:
        committed = f.read()
    assert GEN.render_header() == committed
    assert GEN.main(["--check"]) == 0


def test_triangles_use_only_crossed_edges():
    for case, tris in enumerate(TABS):
        crossed = {e for e, (c0, c1) in enumerate(GEN.EDGES) if ((case >> c0) & 1) != ((case >> c1) & 1)}
        used = {e for t in tris for e in t}
        assert used == crossed, case
        assert all(len(set(t)) == 3 for t in tris), case
    assert TABS[0] == [] and TABS[255] == []


def test_face_segments_depend_only_on_the_face_corners():
    seen = {}
    for case, tris in enumerate(TABS):
        for a in range(3):
            for s in range(2):
                cyc, _ = GEN.face_cycle(a, s)
                signs = tuple((case >> c) & 1 for c in cyc)
                face = (a, s)
                segs = set()
                for t in tris:
                    for j in range(3):
                        e0, e1 = t[j], t[(j + 1) % 3]
                        if face in GEN.edge_faces(e0) and face in GEN.edge_faces(e1):
                            segs.add((e0, e1))
                key = (face, signs)
                assert seen.setdefault(key, segs) == segs, (case, face)
    # the two faces that share a cube edge see the same crossing there, and an ambiguous face keeps its inside corners
    # apart: two segments, each cutting off one inside corner
    for (face, signs), segs in seen.items():
        if signs in ((1, 0, 1, 0), (0, 1, 0, 1)):
            assert len(segs) == 2


def test_interior_edges_shared_twice_opposite_and_face_edges_once():
    for case, tris in enumerate(TABS):
        directed = collections.Counter()
        for t in tris:
            for j in range(3):
                directed[(t[j], t[(j + 1) % 3])] += 1
        assert all(n == 1 for n in directed.values()), case
        for (e0, e1), n in directed.items():
            if _on_face(e0, e1):
                assert (e1, e0) not in directed, (case, e0, e1)   # on the cube's surface: exactly one triangle
            else:
                assert (e1, e0) in directed, (case, e0, e1)       # inside the cube: the reverse in one other triangle


def test_single_corner_orientation_points_outward():
    for c in range(8):
        q = np.array(GEN.corner_pos(c), float)
        (t,) = TABS[1 << c]
        p = np.array([GEN.mid(e) for e in t])
        n = np.cross(p[1] - p[0], p[2] - p[0])
        assert n @ (p[0] - q) > 0


def _lattice(n, lo=-1.0, hi=1.0):
    x = np.linspace(lo, hi, n, dtype=np.float32)
    return np.meshgrid(x, x, x, indexing="ij")


def test_sphere_is_closed_genus_zero_and_outward():
    X, Y, Z = _lattice(40)
    vol = (0.6 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, f, n = R.marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    assert R.is_closed_oriented_manifold(f)
    assert R.euler_characteristic(v, f) == 2
    vol_ref = 4.0 / 3.0 * np.pi * 0.6 ** 3
    assert abs(R.signed_volume(v, f) - vol_ref) < 0.02 * vol_ref
    # vertex normals point away from the centre
    assert (np.einsum("ij,ij->i", n, v) > 0).all()


def test_torus_has_euler_characteristic_zero():
    X, Y, Z = _lattice(48)
    vol = (0.2 - np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)).astype(np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    assert R.is_closed_oriented_manifold(f)
    assert R.euler_characteristic(v, f) == 0
    assert R.signed_volume(v, f) > 0


def test_random_noise_closed_boundary_is_a_closed_oriented_manifold():
    rng = np.random.default_rng(0)
    vol = rng.standard_normal((24, 24, 24)).astype(np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1), close_boundary=True)
    assert len(f) > 1000 and R.is_closed_oriented_manifold(f)
    # values exactly at iso are outside: a lattice of exact zeros and ones
    vol2 = (rng.random((9, 10, 11)) > 0.5).astype(np.float32)
    v2, f2, _ = R.marching_cubes(vol2, 1.0, (0, 0, 0), (1, 1, 1))
    assert len(f2) == 0
    v3, f3, _ = R.marching_cubes(vol2, 0.0, (0, 0, 0), (1, 1, 1))
    assert len(f3) > 0 and R.is_closed_oriented_manifold(f3)
    # without the cap the mesh is open at the box
    _, f4, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1), close_boundary=False)
    assert not R.is_closed_oriented_manifold(f4)


def test_all_inside_closed_boundary_is_the_box():
    vol = np.ones((5, 6, 7), np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, (-1, -2, -3), (1, 2, 3))
    assert R.is_closed_oriented_manifold(f)
    assert np.array_equal(v.min(0), np.float32([-1, -2, -3])) and np.array_equal(v.max(0), np.float32([1, 2, 3]))
    assert abs(R.signed_volume(v, f) - 2 * 4 * 6) < 1e-4


def test_obj_writer_round_trips_through_read_obj(tmp_path):
    from src.latent_nerf.models.mesh_io import write_obj
    from src.latent_paint.models.mesh import read_obj
    X, Y, Z = _lattice(16)
    vol = (0.5 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, f, n = R.marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    col = np.clip(np.abs(n), 0, 1)
    path = write_obj(os.path.join(str(tmp_path), "mesh", "mesh.obj"), v, f, n, col)
    rv, rf, vt, ft = read_obj(path)
    assert np.array_equal(rv.numpy(), v) and np.array_equal(rf.numpy(), f.astype(np.int64))
    assert vt is None and ft is None
    lines = open(path).read().splitlines()
    vlines = [l for l in lines if l.startswith("v ")]
    assert len(vlines) == len(v) and len(vlines[0].split()) == 7
    assert sum(l.startswith("vn ") for l in lines) == len(v)
    assert [l for l in lines if l.startswith("f ")][0].count("//") == 3
    cols = np.array([[float(x) for x in l.split()[4:]] for l in vlines])
    assert np.abs(cols - col).max() < 1e-4
