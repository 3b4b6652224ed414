"""Mesh decimation without a GPU: the numpy restatement of lnerf_decimate (tests/decimate_reference.py) on marching-cubes
meshes (tests/mc_reference.py) keeps closed meshes closed with their topology and on their surface, holds open borders
and the box's corners in place, lands on the target, and refuses a collapse the link condition forbids."""
import numpy as np
import pytest

from tests import decimate_reference as D
from tests import mc_reference as R
from tests.decimate_cases import component_euler as _component_euler


def _lattice(n):
    x = np.linspace(-1, 1, n, dtype=np.float32)
    return np.meshgrid(x, x, x, indexing="ij")


def _sphere(X, Y, Z):
    return 0.6 - np.sqrt(X * X + Y * Y + Z * Z)


def _torus(X, Y, Z):
    return 0.2 - np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)


SHAPES = {"sphere": (_sphere, 40, 2), "torus": (_torus, 48, 0)}


def _mc(sdf, n, close=True):
    X, Y, Z = _lattice(n)
    return R.marching_cubes(sdf(X, Y, Z).astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1), close_boundary=close)


def _clean(v, f):
    """No face repeats an index and every vertex is used."""
    f = np.asarray(f)
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any()
    assert np.array_equal(np.unique(f), np.arange(len(v)))


def _boundary_vertices(f):
    d = R.directed_edges(f)
    key = d[:, 0] * (1 << 32) + d[:, 1]
    rkey = d[:, 1] * (1 << 32) + d[:, 0]
    return np.unique(d[~np.isin(rkey, key)])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_closed_surface_reaches_the_target_on_the_surface(name):
    sdf, n, chi = SHAPES[name]
    v, f, _ = _mc(sdf, n)
    assert 3000 < len(f) < 10000
    target = 1000
    ov, of, on, info = D.decimate(v, f, target)
    assert len(of) in (target, target - 1)
    assert info["collapses"] == (len(f) - len(of)) // 2 and info["rounds"] > 1
    assert R.is_closed_oriented_manifold(of)
    assert R.euler_characteristic(ov, of) == R.euler_characteristic(v, f) == chi
    _clean(ov, of)
    h = 2.0 / (n - 1)
    p = ov.astype(np.float64)
    assert np.abs(sdf(p[:, 0], p[:, 1], p[:, 2])).max() <= 0.5 * h
    assert abs(R.signed_volume(ov, of) / R.signed_volume(v, f) - 1) < 0.02
    assert np.allclose(np.linalg.norm(on, axis=1), 1, atol=1e-5)


def test_box_keeps_its_corners_and_planes():
    vol = np.ones((5, 6, 7), np.float32)
    lo, hi = np.float32([-1, -2, -3]), np.float32([1, 2, 3])
    v, f, _ = R.marching_cubes(vol, 0.0, lo, hi)
    ov, of, _, info = D.decimate(v, f, 12, max_error=1e-12)
    assert len(of) <= 32 and info["collapses"] > 0
    assert R.is_closed_oriented_manifold(of)
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], np.float32)
    for c in corners:
        assert (ov == c).all(1).any(), c
    assert (ov >= lo - 1e-6).all() and (ov <= hi + 1e-6).all()
    assert (np.minimum(np.abs(ov - lo), np.abs(ov - hi)).min(1) <= 1e-6).all()
    assert abs(R.signed_volume(ov, of) - 2 * 4 * 6) < 1e-4


def test_noise_components_keep_their_topology():
    rng = np.random.default_rng(0)
    vol = rng.standard_normal((12, 12, 12)).astype(np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1), close_boundary=True)
    ov, of, _, info = D.decimate(v, f, len(f) // 4)
    assert info["collapses"] > len(f) // 4
    assert R.is_closed_oriented_manifold(of)
    _clean(ov, of)
    assert _component_euler(ov, of) == _component_euler(v, f)


def test_open_border_is_held_bitwise():
    X, Y, Z = _lattice(32)
    vol = (0.8 - np.sqrt(X * X + Y * Y + (Z + 0.6) ** 2)).astype(np.float32)
    v, f, _ = R.marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1), close_boundary=False)
    bv = _boundary_vertices(f)
    assert len(bv) > 50
    ov, of, _, info = D.decimate(v, f, 300)
    assert len(of) < len(f) // 2
    obv = _boundary_vertices(of)
    def bits(a):
        return sorted(map(tuple, np.ascontiguousarray(a).view(np.uint32).tolist()))
    assert bits(ov[obv]) == bits(v[bv])


def test_target_at_or_above_the_face_count_changes_nothing():
    v, f, _ = _mc(_sphere, 24)
    for target in (len(f), len(f) + 7):
        ov, of, _, info = D.decimate(v, f, target)
        assert np.array_equal(ov.view(np.uint32), v.view(np.uint32)) and np.array_equal(of, f)
        assert info == {"rounds": 0, "collapses": 0}


def _bipyramid():
    """Apexes 0 (top) and 1 (bottom) over the ring 2, 3, 4 (outward faces)."""
    t = 2 * np.pi * np.arange(3) / 3
    v = np.concatenate([[[0, 0, 1], [0, 0, -1]], np.stack([np.cos(t), np.sin(t), 0 * t], -1)]).astype(np.float32)
    f = np.array([[0, 2, 3], [0, 3, 4], [0, 4, 2], [1, 3, 2], [1, 4, 3], [1, 2, 4]], np.int32)
    return v, f


def test_link_condition_blocks_a_ring_edge():
    v, f = _bipyramid()
    assert R.is_closed_oriented_manifold(f)
    f64 = f.astype(np.int64)
    fan, deg = D._fan(f64, len(v))
    locked, nxt = D.vertex_status(f64, fan, deg)
    assert not locked.any()
    keys, _ = D.evaluate(v, f64, D.vertex_quadrics(v, f64), fan, deg, locked, nxt, np.inf)
    u, w = f64.reshape(-1), np.roll(f64, -1, axis=1).reshape(-1)
    ring = (u >= 2) & (w >= 2)
    assert ring.any() and (keys[ring] == D.KEY_NONE).all()      # three common neighbours: the two apexes and the third
    assert (keys[~ring & (u < w)] != D.KEY_NONE).any()          # an apex edge may go
    ov, of, _, info = D.decimate(v, f, 0)
    assert len(of) == 4 and R.is_closed_oriented_manifold(of)    # a tetrahedron is where it stops
    assert info["collapses"] == 1


def test_out_of_range_index_is_refused():
    v, f = _bipyramid()
    with pytest.raises(ValueError, match="outside"):
        D.decimate(v, np.where(f == 4, 5, f), 0)


# ---------------------------------------------------------------- the op's surface (library + host side, no GPU needed)
def test_library_exports_the_op_and_checks_its_arguments(built_lib):
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    assert {"lnerf_decimate", "lnerf_decimate_scratch_bytes"} <= set(B.header_symbols())
    assert lib.lnerf_decimate_scratch_bytes(100, 196) > 0
    assert lib.lnerf_decimate_scratch_bytes(-1, 10) == 0 and lib.lnerf_decimate_scratch_bytes(10, 2 ** 30) == 0
    inf = float("inf")
    for args, msg in (((None, 4, None, 4, -1, inf, 8), "target_faces"), ((None, 4, None, 4, 0, -1.0, 8), "max_error"),
                      ((None, 4, None, 4, 0, inf, 8), "null pointer")):
        with pytest.raises(B.LnerfError, match=msg):     # refused on the host, before any device work
            B.call("lnerf_decimate", *args, None, 0, None, None, None, None, None)


def test_host_side_refuses_cpu_tensors_and_bad_arguments(built_lib):
    import torch
    from src.latent_nerf.raymarching import decimate_mesh
    v, f = _bipyramid()
    with pytest.raises(ValueError, match="no CPU path"):
        decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), 0)
    with pytest.raises(ValueError, match="target_faces"):
        decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), -2)
    with pytest.raises(ValueError, match="max_error"):
        decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), 0, max_error=float("nan"))
    with pytest.raises(TypeError):
        decimate_mesh(torch.from_numpy(v), torch.from_numpy(f).float(), 0)


def test_export_and_trainer_take_target_faces():
    import inspect

    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.models.renderer import NeRFRenderer
    assert inspect.signature(NeRFRenderer.export_mesh).parameters["target_faces"].default == 0
    assert TrainConfig().log.mesh_target_faces == 0
    assert apply_overrides(TrainConfig(), {"log.mesh_target_faces": "20000"}).log.mesh_target_faces == 20000
