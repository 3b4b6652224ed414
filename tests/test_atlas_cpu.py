"""The chart atlas without a GPU: the properties of the numpy restatement (tests/atlas_reference.py) on every test mesh,
the conditions the GPU tests rely on, the host-side scale search and shelf packing (src/uv_atlas.py), the new config
fields of both trees, Latent-Paint's order of preference for a UV map, and the argument checks of the lnerf_atlas_*
entry points (made-up pointers: a call that got past its checks would need a GPU)."""
import ctypes
import sys
import types

import numpy as np
import pytest
import torch

from src import uv_atlas as UA
from src.latent_nerf.raymarching import backend as B
from tests import atlas_reference as A

MC = [("sphere", 32, 256), ("torus", 32, 256), ("blob", 32, 256)]
MESHES = {"cube": (A.cube, 64), "octahedron": (A.octahedron, 64), "helicoid": (A.helicoid, 128), "zoo": (A.topology_zoo, 128)}


def _mesh(name):
    if name in MESHES:
        return MESHES[name][0]() + (MESHES[name][1],)
    n, res, R = [c for c in MC if c[0] == name][0]
    return A.mc_mesh(n, res) + (R,)


@pytest.mark.parametrize("name", [c[0] for c in MC] + sorted(MESHES))
def test_reference_atlas_has_every_property(name):
    v, f, R = _mesh(name)
    res = A.chart_atlas(v, f, R)
    ratio = A.check_properties(v, f, res, R)
    assert len(res["chart_rect"]) == res["n_base"] + len(res["evicted"]) == len(res["chart_axis"])
    assert ratio.max() <= 1 + 1e-4                        # (check_properties holds every face to its own rounding bound)
    # a chart's faces all lie in the chart's bucket, and the bucket's axis is within 1/sqrt(3) of every normal
    assert np.array_equal(res["chart_axis"][res["face_chart"]], res["bucket"])
    P = v.astype(np.float64)[f]
    m = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nz = np.linalg.norm(m, axis=1) > 1e-12
    cos = (m[nz] * A.AXES[res["bucket"][nz]]).sum(1) / np.linalg.norm(m[nz], axis=1)
    assert cos.min() >= 1 / np.sqrt(3) - 1e-6


@pytest.mark.parametrize("name,n,R", MC)
def test_marching_cubes_inputs_need_no_eviction_and_few_charts(name, n, R):
    v, f = A.mc_mesh(name, n)
    res = A.chart_atlas(v, f, R)
    assert len(res["evicted"]) == 0 and res["n_base"] < 64
    assert A.strict_coverage_count(res["vt"], res["ft"], R).max() <= 1
    for small in ("sphere", "torus"):                    # the 16^3 meshes of the GPU file
        r16 = A.chart_atlas(*A.mc_mesh(small, 16), 128)
        assert len(r16["evicted"]) == 0 and r16["n_base"] < 64


def test_helicoid_folds_and_the_fold_check_unfolds_it():
    v, f = A.helicoid()
    assert len(f) == 384 and (A.buckets(v, f) == 2).all()             # one +y bucket ...
    before = A.chart_atlas(v, f, 128, fold_check=False)
    assert before["n_base"] == 1                                       # ... and one chart
    assert (A.strict_coverage_count(before["vt"], before["ft"], 128) > 1).sum() > 0
    after = A.chart_atlas(v, f, 128)
    assert len(after["evicted"]) > 0
    assert A.strict_coverage_count(after["vt"], after["ft"], 128).max() <= 1
    keep = np.setdiff1d(np.arange(len(f)), after["evicted"])
    assert (after["face_chart"][keep] == 0).all()
    assert np.array_equal(after["face_chart"][after["evicted"]], 1 + np.arange(len(after["evicted"])))
    # the faces that stay keep their vt bits: the same layout at the same k without the fold check
    same_k = A.emit(*A.plane_coords(v, f, after["bucket"]), f, before["face_chart"],
                    A.pack(before["chart_box"], 128, 2, after["k"])[2], before["chart_box"], after["scale"], 128, 2, len(v))
    assert np.array_equal(same_k[0][same_k[1][keep]].view(np.uint32), after["vt"][after["ft"][keep]].view(np.uint32))


def test_expected_charts_of_the_small_solids():
    v, f = A.cube()
    res = A.chart_atlas(v, f, 64)
    assert res["chart_axis"].tolist() == [0, 1, 2, 3, 4, 5] and res["face_chart"].tolist() == [c for c in range(6) for _ in (0, 1)]
    assert len(res["vt"]) == 24
    area = A.uv_area(res["vt"], res["ft"]) * 64 * 64 / res["scale"] ** 2
    assert np.abs(area - 0.5).max() < 1e-4                             # axis-aligned faces keep their area
    v, f = A.octahedron()
    res = A.chart_atlas(v, f, 64)
    # every score ties at |m_x| = |m_y| = |m_z|: the first maximum is +x where m_x > 0, else -x
    assert res["bucket"].tolist() == [0, 1, 1, 0, 0, 1, 1, 0]
    assert res["n_base"] == 2 and res["face_chart"].tolist() == [0, 1, 1, 0, 0, 1, 1, 0]


def test_topology_edge_cases_in_the_reference():
    v, f = A.topology_zoo()
    res = A.chart_atlas(v, f, 128)
    fc = res["face_chart"]
    assert fc[0] == fc[1] and fc[2] == fc[3] and fc[0] != fc[2]        # stacked squares: two charts
    assert len({fc[4], fc[5], fc[6]}) == 3                             # three faces on one edge: no link across it
    assert (A.twins(f)[12:21].reshape(3, 3)[:, 0] == -1).all()
    assert len(set(fc[7:15].tolist())) == 1                            # the open strip is one chart
    assert res["bucket"][15] == 0 and (fc == fc[15]).sum() == 1        # the zero-area face: bucket 0, alone
    assert res["bucket"][16] == 4 and res["bucket"][17] == 5 and fc[16] != fc[17]   # reversed twin: linked, other bucket
    assert (A.twins(f)[48:54] >= 0).all()
    assert len(res["evicted"]) == 0


# ------------------------------------------------------------------------------ host side: scale search and packing
def test_shelf_packing_order_and_shelf_rule():
    w, h = [4, 6, 3, 5, 6], [3, 5, 5, 3, 2]
    # order (h desc, w desc, index asc): 1 (6x5), 2 (3x5), 3 (5x3), 0 (4x3), 4 (6x2)
    for pack in (UA.shelf_pack, A.shelf_pack):
        ox, oy, state = pack(np.array(w), np.array(h), 10)
        assert ox.tolist() == [5, 0, 6, 0, 0] and oy.tolist() == [5, 0, 0, 5, 8] and state == (6, 8, 2)
        # x + w == R still fits; one more texel opens a shelf; y + h > R fails
        assert pack(np.array([5, 5]), np.array([2, 2]), 10)[0].tolist() == [0, 5]
        assert pack(np.array([5, 6]), np.array([2, 2]), 10)[1].tolist() == [2, 0]
        assert pack(np.array([6, 6]), np.array([5, 6]), 10) is None
        assert pack(np.array([11]), np.array([1]), 10) is None
    # continuing from a state: a taller rectangle raises the open shelf; one that passes the bottom fails
    assert UA.shelf_pack(np.array([2]), np.array([4]), 10, state=(6, 8, 2)) is None
    a = UA.shelf_pack(np.array([2, 2]), np.array([4, 1]), 12, state=(6, 8, 2))
    b = A.shelf_pack(np.array([2, 2]), np.array([4, 1]), 12, state=(6, 8, 2))
    assert a[0].tolist() == b[0].tolist() == [6, 8] and a[1].tolist() == b[1].tolist() == [8, 8] and a[2] == b[2] == (10, 8, 4)


def test_scale_search_matches_the_restatement_and_spans_the_side():
    rng = np.random.default_rng(3)
    lo = rng.uniform(-1, 1, (40, 2)).astype(np.float32)
    ext = rng.uniform(0, 0.7, (40, 2)).astype(np.float32)
    box = np.stack([lo[:, 0], lo[:, 0] + ext[:, 0], lo[:, 1], lo[:, 1] + ext[:, 1]], 1).astype(np.float32)
    for R, pad in ((64, 2), (200, 0), (512, 3)):
        k, s, rect, state = UA.pack_charts(box, R, pad)
        k2, s2, rect2, state2 = A.pack(box, R, pad)
        assert (k, s, state) == (k2, s2, state2) and np.array_equal(rect, rect2)
        assert s == float(np.float32(s))
    one = np.array([[0.0, 2.0, 0.0, 1.0]], np.float32)
    k, s, rect, _ = UA.pack_charts(one, 64, 2)
    assert k == 0 and s == 29.0 and rect.tolist() == [[0, 0, 64, 35]]   # the largest chart spans the side
    k, s, rect, _ = UA.pack_charts(np.zeros((3, 4), np.float32), 64, 2)
    assert (k, s) == (0, 1.0) and rect[:, 2:].tolist() == [[6, 6]] * 3   # every extent 0: s = 1


def test_too_many_charts_raise_with_the_resolution_that_would_do():
    box = np.zeros((1000, 4), np.float32)
    box[:, 1] = box[:, 3] = 0.01
    with pytest.raises(ValueError) as e:
        UA.pack_charts(box, 32, 2)
    msg = str(e.value)
    assert "1000 charts" in msg and "32 x 32" in msg and ">= 192" in msg      # ceil(sqrt(1000)) = 32 rectangles of 6
    with pytest.raises(ValueError):
        A.pack(box, 32, 2)
    assert UA.pack_charts(box[:25], 32, 2)[0] >= 0                             # 5 x 5 of them do fit (6 * 5 <= 32)


# ------------------------------------------------------------------------------ configuration
def test_config_fields_default_to_the_triangle_atlas_and_refuse_other_names():
    from src.latent_nerf.configs.train_config import TrainConfig as NerfConfig
    from src.latent_nerf.configs.train_config import apply_overrides as nerf_over
    from src.latent_paint.configs.train_config import TrainConfig as PaintConfig
    from src.latent_paint.configs.train_config import apply_overrides as paint_over
    assert NerfConfig().log.mesh_atlas == "triangle"
    assert nerf_over(NerfConfig(), {"log.mesh_atlas": "charts"}).log.mesh_atlas == "charts"
    with pytest.raises(ValueError, match="log.mesh_atlas"):
        nerf_over(NerfConfig(), {"log.mesh_atlas": "xatlas"})
    assert PaintConfig().guide.uv_atlas == "triangle"
    base = {"log.exp_name": "e", "guide.shape_path": "m.obj"}
    assert paint_over(PaintConfig(), dict(base, **{"guide.uv_atlas": "charts"})).validate().guide.uv_atlas == "charts"
    with pytest.raises(ValueError, match="guide.uv_atlas"):
        paint_over(PaintConfig(), dict(base, **{"guide.uv_atlas": "boxes"})).validate()
    import inspect
    from src.latent_nerf.models.renderer import NeRFRenderer
    assert inspect.signature(NeRFRenderer.export_mesh).parameters["atlas"].default == "triangle"
    assert inspect.signature(NeRFRenderer._export_textured).parameters["atlas"].default == "triangle"
    with pytest.raises(ValueError, match="atlas"):
        UA.check_atlas_choice("quads", "export_mesh: atlas")


def test_uv_map_preference_is_unchanged_and_only_the_last_branch_reads_the_flag(tmp_path, monkeypatch):
    """mesh UVs, then the cached vt.pth / ft.pth, then xatlas when importable, then the built-in atlas."""
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    v, f = A.octahedron()

    def model(exp, flag=None, vt=None, ft=None):
        guide = types.SimpleNamespace() if flag is None else types.SimpleNamespace(uv_atlas=flag)
        mesh = types.SimpleNamespace(vertices=torch.from_numpy(v), faces=torch.from_numpy(f).long(), vt=vt, ft=ft)
        return types.SimpleNamespace(mesh=mesh, device=torch.device("cpu"), texture_resolution=64,
                                     opt=types.SimpleNamespace(log=types.SimpleNamespace(exp_dir=str(exp)), guide=guide))

    monkeypatch.setitem(sys.modules, "xatlas", None)                   # not importable
    tri_vt, tri_ft = UA.per_triangle_atlas(len(f), torch.device("cpu"))
    for flag in (None, "triangle"):                                    # the flag left alone: the per-triangle atlas, cached
        exp = tmp_path / ("plain_%s" % flag)
        vt, ft = TexturedMeshModel.init_texture_map(model(exp, flag))
        assert torch.equal(vt, tri_vt) and torch.equal(ft, tri_ft)
        assert torch.equal(torch.load(exp / "vt.pth", weights_only=True), tri_vt)
    # 1. the mesh's own UVs win, whatever the flag
    own_vt, own_ft = torch.rand(10, 2), torch.randint(0, 10, (8, 3))
    vt, ft = TexturedMeshModel.init_texture_map(model(tmp_path / "own", "charts", own_vt, own_ft))
    assert torch.equal(vt, own_vt) and torch.equal(ft, own_ft) and not (tmp_path / "own").exists()
    # 2. then the cache
    vt, ft = TexturedMeshModel.init_texture_map(model(tmp_path / "plain_None", "charts"))
    assert torch.equal(vt, tri_vt) and torch.equal(ft, tri_ft)
    # 3. then xatlas when importable
    class _Atlas:
        def add_mesh(self, *a): pass
        def generate(self, **k): pass
        def __getitem__(self, i): return None, np.zeros((8, 3), np.uint32), np.full((5, 2), 0.25, np.float32)
    fake = types.SimpleNamespace(Atlas=_Atlas, ChartOptions=lambda: types.SimpleNamespace())
    monkeypatch.setitem(sys.modules, "xatlas", fake)
    vt, ft = TexturedMeshModel.init_texture_map(model(tmp_path / "xa", "charts"))
    assert vt.shape == (5, 2) and float(vt[0, 0]) == 0.25 and ft.dtype == torch.int64
    # 4. the built-in atlas is the only branch that reads the flag: "charts" reaches the GPU op, which refuses the CPU
    monkeypatch.setitem(sys.modules, "xatlas", None)
    with pytest.raises(ValueError, match="no CPU path"):
        TexturedMeshModel.init_texture_map(model(tmp_path / "charts", "charts"))
    with pytest.raises(ValueError, match="guide.uv_atlas"):
        TexturedMeshModel.init_texture_map(model(tmp_path / "bad", "boxes"))


def test_ops_refuse_cpu_tensors_and_bad_arguments(built_lib):
    from src.latent_nerf.raymarching import chart_atlas
    v, f = A.cube()
    with pytest.raises(ValueError, match="no CPU path"):
        chart_atlas(torch.from_numpy(v), torch.from_numpy(f), 64)
    with pytest.raises(ValueError, match="resolution"):
        chart_atlas(torch.from_numpy(v), torch.from_numpy(f), 0)
    with pytest.raises(ValueError, match="resolution"):
        chart_atlas(torch.from_numpy(v), torch.from_numpy(f), B.UV_MAX_RES + 1)
    with pytest.raises(ValueError, match="pad"):
        chart_atlas(torch.from_numpy(v), torch.from_numpy(f), 8, pad=4)
    with pytest.raises(ValueError, match="no CPU path"):
        UA.chart_atlas(torch.from_numpy(v), torch.from_numpy(f), 64)


# ------------------------------------------------------------------------------ C ABI: checks before any launch
def test_atlas_entry_points_refuse_bad_arguments(built_lib):
    lib = B.get_lib()
    P = ctypes.c_void_p
    ok, odd = P(4096), P(4096 + 4)
    header = open(B.HEADER_PATH).read()
    assert "#define LNERF_ATLAS_MAX_ROUNDS %d" % B.ATLAS_MAX_ROUNDS in header
    assert "#define LNERF_ATLAS_MAX_FACES (1 << 28)" in header and B.ATLAS_MAX_FACES == 1 << 28
    assert lib.lnerf_abi_version() == 7

    def err(rc, word):
        assert rc == -1 and word in lib.lnerf_last_error(), (rc, lib.lnerf_last_error())

    # sizing calls: 0 = out of range
    assert lib.lnerf_atlas_compact_scratch_bytes(-1) == 0 and lib.lnerf_atlas_compact_scratch_bytes((1 << 28) + 1) == 0
    assert lib.lnerf_atlas_boxes_scratch_bytes(-1) == 0
    assert lib.lnerf_atlas_fold_scratch_bytes(-1, 64) == 0 and lib.lnerf_atlas_fold_scratch_bytes(10, 0) == 0
    assert lib.lnerf_atlas_fold_scratch_bytes(10, B.UV_MAX_RES + 1) == 0
    nc, nb, nf = (lib.lnerf_atlas_compact_scratch_bytes(1000), lib.lnerf_atlas_boxes_scratch_bytes(10),
                  lib.lnerf_atlas_fold_scratch_bytes(1000, 64))
    assert nc >= 1000 * 4 and nb >= 160 and nf >= 1000 * 8
    assert lib.lnerf_atlas_fold_scratch_bytes(1000, 1) == nf == lib.lnerf_atlas_fold_scratch_bytes(1000, B.UV_MAX_RES)
    # buckets / round
    err(lib.lnerf_atlas_buckets(ok, 8, ok, -1, ok, ok, ok, None), b"faces")
    err(lib.lnerf_atlas_buckets(ok, -1, ok, 12, ok, ok, ok, None), b"vertices")
    err(lib.lnerf_atlas_buckets(ok, 8, ok, 12, ok, ok, None, None), b"null counts")
    err(lib.lnerf_atlas_buckets(ok, 8, ok, 12, None, ok, ok, None), b"null pointer")
    err(lib.lnerf_atlas_round(ok, ok, -1, ok, ok, None), b"faces")
    err(lib.lnerf_atlas_round(ok, ok, 12, ok, None, None), b"null flag")
    err(lib.lnerf_atlas_round(ok, None, 12, ok, ok, None), b"null pointer")
    # compact
    err(lib.lnerf_atlas_compact(ok, ok, -1, ok, nc, ok, ok, ok, None), b"faces")
    err(lib.lnerf_atlas_compact(ok, ok, 1000, ok, nc - 1, ok, ok, ok, None), b"scratch of")
    err(lib.lnerf_atlas_compact(ok, ok, 1000, odd, nc, ok, ok, ok, None), b"16-byte aligned")
    err(lib.lnerf_atlas_compact(ok, ok, 1000, ok, nc, None, ok, ok, None), b"null pointer")
    err(lib.lnerf_atlas_compact(ok, ok, 1000, ok, nc, ok, ok, None, None), b"null pointer")
    # boxes
    err(lib.lnerf_atlas_boxes(ok, 8, ok, ok, ok, -1, 10, ok, nb, ok, None), b"out of range")
    err(lib.lnerf_atlas_boxes(ok, 8, ok, ok, ok, 12, -1, ok, nb, ok, None), b"out of range")
    err(lib.lnerf_atlas_boxes(ok, 8, ok, ok, ok, 12, 10, ok, nb - 1, ok, None), b"scratch of")
    err(lib.lnerf_atlas_boxes(ok, 8, ok, ok, ok, 12, 10, odd, nb, ok, None), b"16-byte aligned")
    err(lib.lnerf_atlas_boxes(ok, 8, ok, ok, ok, 12, 10, ok, nb, None, None), b"null pointer")
    # uv
    uv = lambda **k: lib.lnerf_atlas_uv(ok, 8, ok, ok, k.get("F", 12), ok, ok, ok, ok, 6, k.get("pad", 2), k.get("s", 10.0),
                                        k.get("R", 64), k.get("vt", ok), 24, None)
    err(uv(F=-1), b"out of range")
    err(uv(R=0), b"resolution")
    err(uv(R=B.UV_MAX_RES + 1), b"resolution")
    err(uv(pad=-1), b"pad")
    err(uv(s=float("nan")), b"scale")
    err(uv(s=float("inf")), b"scale")
    err(uv(vt=None), b"null pointer")
    # fold
    fold = lambda **k: lib.lnerf_atlas_fold(ok, 24, ok, k.get("F", 1000), k.get("R", 64), k.get("stages", B.UV_COVER),
                                            k.get("items", 5), k.get("scratch", ok), k.get("bytes", nf), k.get("owner", ok),
                                            k.get("ev", ok), k.get("counts", ok), None)
    err(fold(F=-1), b"faces")
    err(fold(R=0), b"resolution")
    err(fold(R=B.UV_MAX_RES + 1), b"resolution")
    err(fold(stages=0), b"stage bits")
    err(fold(stages=B.UV_EMIT), b"stage bits")
    err(fold(bytes=nf - 1), b"scratch of")
    err(fold(scratch=odd), b"16-byte aligned")
    err(fold(scratch=None), b"null pointer")
    err(fold(counts=None), b"null pointer")
    err(fold(owner=None), b"null output")
    err(fold(ev=None), b"null output")
    err(fold(items=-1), b"negative item count")
