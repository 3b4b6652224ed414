"""Mesh cleaning on the MI355X: raymarching.mesh_components, clean_mesh / mesh_filter and smooth_mesh against the numpy
restatement (tests/meshclean_reference.py) bit for bit, at block edges, on non-manifold and open meshes and on a long
strip whose vertex ids are shuffled; the refusal of out-of-range indices and arguments; repeatability; and
NeRFRenderer.export_mesh with the cleaning and smoothing stages end to end."""
import functools

import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import meshclean_reference as M

pytestmark = pytest.mark.gpu

BOX = (-1, -1, -1), (1, 1, 1)
KEEP_ARGS = [(0, 0.0, 0), (100, 0.1, 0), (0, 0.0, 1), (8, 0.05, 2)]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _groups(V, F, seed):
    """V random vertices, F random faces that each stay inside one group of 37 consecutive vertices (and now and then
    repeat an index): many components, some vertices in no face."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((V, 3)).astype(np.float32)
    g0 = rng.integers(0, max(V - 37, 1), F) // 37 * 37
    f = (g0[:, None] + rng.integers(0, min(37, V), (F, 3))).astype(np.int32)
    f[::11, 2] = f[::11, 0]
    return v, np.minimum(f, V - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "floaters":
        v, f, _ = R.marching_cubes(M.floaters_volume(), 0.0, *BOX)
    elif name == "noise":                       # the 12^3 noise volume of tests/test_gpu_decimate.py: non-manifold
        vol = np.random.default_rng(0).standard_normal((12, 12, 12)).astype(np.float32)
        v, f, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1))
    elif name == "open":                        # ... and its open cap
        x = np.linspace(-1, 1, 32, dtype=np.float32)
        X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
        v, f, _ = R.marching_cubes((0.8 - np.sqrt(X * X + Y * Y + (Z + 0.6) ** 2)).astype(np.float32), 0.0, *BOX,
                                   close_boundary=False)
    elif name == "staircase":
        v, f, _ = R.marching_cubes(M.staircase_volume(), 0.5, *BOX)
    elif name == "empty":
        v, f = np.random.default_rng(2).standard_normal((5, 3)).astype(np.float32), np.zeros((0, 3), np.int32)
    elif name == "odd":                         # unreferenced vertices, faces that repeat an index, -0 and +0
        v = np.random.default_rng(3).standard_normal((12, 3)).astype(np.float32)
        v[1, 0], v[4, 0], v[6, 1], v[9, 1] = -0.0, 0.0, 0.0, -0.0
        f = np.int32([[4, 4, 1], [1, 3, 3], [6, 9, 10], [10, 9, 6], [6, 6, 6], [11, 8, 7], [7, 8, 10]])
    elif name == "strip":                       # one component, found through ids in a fixed random order
        n = 65536
        perm = np.random.default_rng(1).permutation(n).astype(np.int32)
        i = np.arange(n - 2)
        f = perm[np.stack([i, i + 1, i + 2], 1)]
        v = np.random.default_rng(4).standard_normal((n, 3)).astype(np.float32)
    elif name == "wide":                        # over 1024 blocks of vertices: a thread of the top-level scan owns two
        V = 1024 * 256 + 300
        rng = np.random.default_rng(5)
        v = rng.standard_normal((V, 3)).astype(np.float32)
        f = rng.integers(0, V, (3000, 3)).astype(np.int32)
        f[:500] = (V - 600 + rng.integers(0, 600, (500, 3))).astype(np.int32)
    else:                                       # "V x F"
        V, F = (int(s) for s in name.split("x"))
        v, f = _groups(V, F, V * 7 + F)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


@functools.lru_cache(maxsize=None)
def _ref_components(name):
    return M.components(*_mesh(name))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _t(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _components(dev, v, f):
    from src.latent_nerf.raymarching import mesh_components
    st = {}
    out = mesh_components(*_t(dev, v, f), stats=st)
    torch.cuda.synchronize()
    return {k: (x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for k, x in out.items()}, st


EDGES = ["%dx%d" % (n, n) for n in (255, 256, 257, 1023, 1024, 1025)] + ["255x1025", "1025x255", "257x256"]
COMPONENT_CASES = ["floaters", "noise", "empty", "odd", "strip", "wide"] + EDGES


@pytest.mark.parametrize("case", COMPONENT_CASES)
def test_components_match_restatement_bit_for_bit(dev, case):
    v, f = _mesh(case)
    got, st = _components(dev, v, f)
    ref = _ref_components(case)
    assert got["components"] == ref["components"] == st["components"] and got["referenced"] == ref["referenced"]
    assert np.array_equal(got["vert_comp"], ref["vert_comp"]) and got["vert_comp"].dtype == np.int32
    assert np.array_equal(got["face_comp"], ref["face_comp"])
    assert np.array_equal(got["comp_faces"], ref["comp_faces"])
    assert got["comp_box"].shape == ref["comp_box"].shape and np.array_equal(_bits(got["comp_box"]), _bits(ref["comp_box"]))
    assert 1 <= st["rounds"] <= 256
    if case == "floaters":
        assert ref["comp_faces"].tolist() == [8, 68, 3596, 108, 544, 224]
    if case == "noise":
        assert ref["components"] == 26
    if case == "strip":
        assert ref["components"] == 1 and ref["comp_faces"].tolist() == [65534]
        print("strip: %d rounds" % st["rounds"])
    if case == "wide":
        assert len(v) > 1024 * 256 and ref["components"] > 100
    if case == "odd":
        assert ref["vert_comp"].tolist() == [-1, 0, -1, 0, 0, -1, 1, 1, 1, 1, 1, 1]
    if case == "empty":
        assert ref["components"] == 0 and got["comp_box"].shape == (0, 6)


def test_out_of_range_indices_and_bad_coordinates_are_refused_without_a_fault(dev):
    from src.latent_nerf.raymarching import clean_mesh, mesh_components, mesh_filter, smooth_mesh
    v, f = _mesh("odd")
    tv, = _t(dev, v)
    for bad in (len(v), -1, 2 ** 31 - 1):
        fb = f.copy()
        fb[2, 1] = bad
        tf, = _t(dev, fb)
        for op in (mesh_components, clean_mesh, lambda a, b: smooth_mesh(a, b, 1)):
            with pytest.raises(ValueError, match="outside"):
                op(tv, tf)
        # the filter treats such a face as dropped and reads nothing through it
        ov, of, src = mesh_filter(tv, tf, torch.ones(len(fb), dtype=torch.bool, device=dev))
        keep = np.ones(len(f), bool)
        keep[2] = False
        rv, rf, rsrc = M.mesh_filter(v, f, keep)
        assert np.array_equal(of.cpu().numpy(), rf) and np.array_equal(src.cpu().numpy(), rsrc)
    for bad in (np.nan, np.inf):
        vb = v.copy()
        vb[5, 1] = bad
        with pytest.raises(ValueError, match="non-finite"):
            mesh_components(*_t(dev, vb, f))
    got, _ = _components(dev, v, f)                                  # the device is fine afterwards
    assert np.array_equal(got["vert_comp"], _ref_components("odd")["vert_comp"])


def _clean(dev, v, f, *args):
    from src.latent_nerf.raymarching import clean_mesh
    st = {}
    ov, of, src = clean_mesh(*_t(dev, v, f), *args, stats=st)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), of.cpu().numpy(), src.cpu().numpy(), st


@pytest.mark.parametrize("args", KEEP_ARGS)
@pytest.mark.parametrize("case", ["floaters", "noise"])
def test_clean_mesh_matches_restatement(dev, case, args):
    v, f = _mesh(case)
    gv, gf, gsrc, st = _clean(dev, v, f, *args)
    rv, rf, rsrc, info = M.clean(v, f, *args)
    assert gf.dtype == np.int32 and np.array_equal(gf, rf)
    assert np.array_equal(_bits(gv), _bits(rv)) and np.array_equal(gsrc, rsrc)
    rounds = st.pop("rounds")
    assert st == info and 1 <= rounds <= 256
    if case == "floaters" and args == (100, 0.1, 0):
        assert sorted(M.components(gv, gf)["comp_faces"].tolist()) == [224, 544, 3596]
    if case == "floaters" and args == (0, 0.0, 1):
        assert len(gf) == 3596


# V x F around the 4096-entry block of the flat scan (scan.h) that the incidence lists of lnerf_mesh_smooth go through
FLAT_SCAN_EDGES = ["4095x4097", "4096x4096", "4097x4095"]


@pytest.mark.parametrize("case", ["floaters", "odd", "empty", "257x256", "1025x255", "255x1025", "1024x1024"] + FLAT_SCAN_EDGES)
def test_filter_matches_restatement_on_any_flag(dev, case):
    from src.latent_nerf.raymarching import mesh_filter
    v, f = _mesh(case)
    F = len(f)
    rng = np.random.default_rng(8)
    flags = [np.zeros(F, bool), np.ones(F, bool), rng.random(F) < 0.5, rng.random(F) < 0.02]
    for keep in flags:
        gv, gf, gsrc = mesh_filter(*_t(dev, v, f, keep))
        rv, rf, rsrc = M.mesh_filter(v, f, keep)
        assert np.array_equal(gf.cpu().numpy(), rf) and np.array_equal(gsrc.cpu().numpy(), rsrc)
        assert np.array_equal(_bits(gv.cpu().numpy()), _bits(rv))
    # nothing kept: an empty mesh; everything kept on a mesh without unreferenced vertices: the mesh itself
    gv, gf, gsrc = mesh_filter(*_t(dev, v, f, flags[0]))
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and gsrc.shape == (0,)
    if case == "floaters":
        gv, gf, gsrc = mesh_filter(*_t(dev, v, f, flags[1].astype(np.uint8)))
        assert np.array_equal(gf.cpu().numpy(), f) and np.array_equal(_bits(gv.cpu().numpy()), _bits(v))
        assert np.array_equal(gsrc.cpu().numpy(), np.arange(len(v)))


def _smooth(dev, v, f, *args):
    from src.latent_nerf.raymarching import smooth_mesh
    ov, on = smooth_mesh(*_t(dev, v, f), *args)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), on.cpu().numpy()


SMOOTH_CASES = [("staircase", 1), ("staircase", 3), ("staircase", 0), ("staircase", 3, 0.5, 0.0), ("staircase", 2, 1.0, -1.5),
                ("open", 2), ("noise", 2), ("odd", 3), ("empty", 2), ("257x256", 2), ("1025x255", 1)]
SMOOTH_CASES += [(name, 2) for name in FLAT_SCAN_EDGES]


@pytest.mark.parametrize("case", SMOOTH_CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_smooth_mesh_matches_restatement_bit_for_bit(dev, case):
    v, f = _mesh(case[0])
    gv, gn = _smooth(dev, v, f, *case[1:])
    rv, rn = M.smooth(v, f, *case[1:])
    assert np.array_equal(_bits(gv), _bits(rv))
    assert np.array_equal(_bits(gn), _bits(rn))
    if case[1] == 0:
        assert np.array_equal(_bits(gv), _bits(v))
    elif case[0] != "empty":
        assert not np.array_equal(_bits(gv), _bits(v))


def test_smooth_and_decimate_share_their_normals(dev):
    """smooth_mesh documents its normals "as decimate_mesh's": with nothing to smooth and nothing to collapse the two
    entry points return the same bits, the restatement's."""
    from src.latent_nerf.raymarching import decimate_mesh
    v, f = _mesh("floaters")
    # every vertex referenced and no face repeating an index: decimate_mesh then returns the mesh as it is
    assert np.array_equal(np.unique(f), np.arange(len(v)))
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any()
    sv, sn = _smooth(dev, v, f, 0)
    st = {}
    dv, df, dn = decimate_mesh(*_t(dev, v, f), target_faces=len(f), stats=st)
    torch.cuda.synchronize()
    assert st["rounds"] == 0 and np.array_equal(df.cpu().numpy(), f)
    assert np.array_equal(_bits(dv.cpu().numpy()), _bits(v)) and np.array_equal(_bits(sv), _bits(v))
    rn = M.smooth(v, f, 0)[1]
    assert np.array_equal(_bits(sn), _bits(rn)) and np.array_equal(_bits(dn.cpu().numpy()), _bits(rn))
    assert np.array_equal(_bits(sn), _bits(dn.cpu().numpy()))


def test_taubin_smooths_the_staircase_without_shrinking_it(dev):
    def radii(p):
        r = np.linalg.norm(np.asarray(p, np.float64), axis=1)
        return r.mean(), np.sqrt(((r - r.mean()) ** 2).mean())
    v, f = _mesh("staircase")
    assert len(v) == 2592
    m0, s0 = radii(v)
    p, n = _smooth(dev, v, f, 10)
    q, _ = _smooth(dev, v, f, 10, 0.5, 0.0)
    (m1, s1), (m2, _) = radii(p), radii(q)
    print("rms %.5f -> %.5f, mean radius %+.5f (Taubin) %+.5f (Laplacian)" % (s0, s1, m1 - m0, m2 - m0))
    assert s1 <= 0.6 * s0
    assert abs(m1 - m0) < 0.002
    assert abs(m2 - m0) >= 5 * abs(m1 - m0)
    rp, rn = M.smooth(v, f, 10)
    assert np.array_equal(_bits(p), _bits(rp)) and np.array_equal(_bits(n), _bits(rn))


def test_smoothing_arguments_out_of_range_are_refused(dev):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import smooth_mesh
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    v, f = _mesh("odd")
    tv, tf = _t(dev, v, f)
    for args in ((-1,), (1001,), (1, 0.0), (1, 1.01), (1, float("nan")), (1, 0.5, 0.01), (1, 0.5, -1.51)):
        with pytest.raises(ValueError, match="smooth_mesh"):
            smooth_mesh(tv, tf, *args)
    lib = B.get_lib()
    nb = lib.lnerf_mesh_smooth_scratch_bytes(len(v), len(f))
    scratch = torch.empty(nb, dtype=torch.uint8, device=dev)
    out = torch.full((len(v), 3), -7.0, device=dev)
    for it, lam, mu in ((1001, 0.5, -0.53), (1, 0.0, -0.53), (1, 0.5, 0.25), (1, 0.5, -2.0)):
        rc = lib.lnerf_mesh_smooth(_p(tv), len(v), _p(tf), len(f), it, lam, mu, _p(scratch), nb, _p(out), None, _stream())
        assert rc == -1
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    # an index out of range fails the call before anything is written
    fb = f.copy()
    fb[0, 0] = len(v)
    tb, = _t(dev, fb)
    rc = lib.lnerf_mesh_smooth(_p(tv), len(v), _p(tb), len(f), 1, 0.5, -0.53, _p(scratch), nb, _p(out), None, _stream())
    torch.cuda.synchronize()
    assert rc == -1 and b"1 faces index outside" in lib.lnerf_last_error() and bool((out == -7.0).all())


def test_two_runs_are_identical(dev):
    for case in ("floaters", "noise", "strip"):
        v, f = _mesh(case)
        a, b = _components(dev, v, f)[0], _components(dev, v, f)[0]
        for k in ("vert_comp", "face_comp", "comp_faces", "comp_box"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (case, k)
    for case in ("floaters", "noise"):
        v, f = _mesh(case)
        a, b = _clean(dev, v, f, 8, 0.05, 2), _clean(dev, v, f, 8, 0.05, 2)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a[:3], b[:3]))
        a, b = _smooth(dev, v, f, 3), _smooth(dev, v, f, 3)
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _nerf(dev, latent=False):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    kw = dict(grid_size=32, train_h=16, train_w=16)
    if latent:
        kw["nerf_type"] = NeRFType("latent")
    net = NeRFNetwork(RenderConfig(**kw), log2_hashmap_size=14).to(dev)
    vol = torch.from_numpy(M.floaters_volume()).to(dev)
    net.density_lattice = lambda resolution=None, S=128: vol.clone()      # the field's density, replaced by the floaters
    return net


def test_export_mesh_cleans_smooths_and_decimates(dev, tmp_path):
    from src.latent_paint.models.mesh import read_obj
    net = _nerf(dev)
    b = float(net.bound)
    mv, mf, _ = R.marching_cubes(M.floaters_volume(), 0.0, (-b, -b, -b), (b, b, b))
    cv, cf, csrc, info = M.clean(mv, mf, 100, 0.1, 0)
    kw = dict(thresh=0.0, min_component_faces=100, min_component_diameter=0.1, smooth_iterations=2, target_faces=1500)
    out = net.export_mesh(str(tmp_path / "a"), **kw)
    v, f = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    assert M.components(v, f)["components"] == 3 and 0 < len(f) <= 1500
    assert out["faces_before"] == len(mf) == 4548 and out["faces_cleaned"] == info["faces_after"] == 4364
    assert out["components"] == 6 and out["components_kept"] == 3
    assert out["normals"].shape == out["verts"].shape == out["colors"].shape
    rv, rf, vt, _ = read_obj(str(tmp_path / "a" / "mesh.obj"))
    assert vt is None and np.array_equal(rv.numpy(), v) and np.array_equal(rf.numpy(), f.astype(np.int64))
    # the stages one by one: clean alone carries the lattice normals through vert_src; smooth alone gives its own
    full = net.export_mesh(str(tmp_path / "full"), thresh=0.0)
    only = net.export_mesh(str(tmp_path / "clean"), thresh=0.0, min_component_faces=100, min_component_diameter=0.1)
    assert np.array_equal(only["faces"].cpu().numpy(), cf) and np.array_equal(_bits(only["verts"].cpu().numpy()), _bits(cv))
    assert torch.equal(only["normals"], full["normals"][torch.from_numpy(csrc).to(dev)])
    sm = net.export_mesh(str(tmp_path / "smooth"), thresh=0.0, keep_largest=1, smooth_iterations=2)
    kv, kf, _, _ = M.clean(mv, mf, 0, 0.0, 1)
    sv, sn = M.smooth(kv, kf, 2)
    assert np.array_equal(sm["faces"].cpu().numpy(), kf) and len(kf) == 3596 and sm["components_kept"] == 1
    assert np.array_equal(_bits(sm["verts"].cpu().numpy()), _bits(sv))
    assert np.array_equal(_bits(sm["normals"].cpu().numpy()), _bits(sn))
    # everything at its default: the export of before, byte for byte
    net.export_mesh(str(tmp_path / "d0"), thresh=0.0, target_faces=1500)
    d1 = net.export_mesh(str(tmp_path / "d1"), thresh=0.0, target_faces=1500, min_component_faces=0,
                         min_component_diameter=0.0, keep_largest=0, smooth_iterations=0)
    assert (tmp_path / "d0" / "mesh.obj").read_bytes() == (tmp_path / "d1" / "mesh.obj").read_bytes()
    assert d1["components"] is None and d1["faces_cleaned"] == d1["faces_before"] == 4548
    assert np.array_equal(full["faces"].cpu().numpy(), mf) and M.components(mv, mf)["components"] == 6


def test_textured_export_of_the_cleaned_mesh_writes_the_latent_texture(dev, tmp_path):
    from src.latent_paint.models.mesh import read_obj
    net = _nerf(dev, latent=True)
    out = net.export_mesh(str(tmp_path), thresh=0.0, min_component_faces=100, min_component_diameter=0.1,
                          smooth_iterations=2, target_faces=1500, texture_resolution=256, atlas="charts")
    v, f = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    assert M.components(v, f)["components"] == 3 and len(f) <= 1500 and out["faces_cleaned"] == 4364
    assert out["texture"].shape == (4, 256, 256) and int(out["face_chart"].min()) >= 0
    assert (tmp_path / "latent_texture.pt").exists() and (tmp_path / "albedo.png").exists()
    rv, rf, vt, ft = read_obj(str(tmp_path / "mesh.obj"))
    assert np.array_equal(rf.numpy(), f.astype(np.int64)) and vt is not None and ft.shape == rf.shape


def test_trainer_passes_the_cleaning_options(dev, tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    from src.latent_paint.models.mesh import read_obj
    flat = {"log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32, "render.eval_h": 32,
            "render.eval_w": 32, "render.grid_size": 32, "optim.iters": 2, "log.save_interval": 100,
            "log.eval_size": 1, "log.full_eval_size": 1, "optim.fp16": False, "guide.text": "a lego man",
            "log.exp_name": "c", "log.save_mesh": True, "log.mesh_keep_largest": 1, "log.mesh_smooth_iterations": 2}
    tr = Trainer(apply_overrides(TrainConfig(), flat), device=dev)
    tr.train()
    v, f, _, _ = read_obj(str(tr.exp_path / "mesh" / "mesh.obj"))
    assert f.shape[0] > 0 and M.components(v.numpy(), f.numpy())["components"] == 1
    assert "mesh cleaning kept 1 of" in (tr.exp_path / "log.txt").read_text()
