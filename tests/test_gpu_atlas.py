"""The chart atlas on the MI355X: raymarching.chart_atlas against the numpy restatement (tests/atlas_reference.py) bit for
bit -- vt, ft, face_chart, chart_rect, chart_axis, scale, k and the evicted set -- on the smallest meshes at which each
stage can go wrong, its properties, a position round trip through the bake and Latent-Paint's bilinear lookup, and
the export / Latent-Paint paths end to end."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import atlas_reference as A
from tests import uv_reference as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _op(dev, v, f, R, pad=2):
    from src.latent_nerf.raymarching import chart_atlas
    st = {}
    vt, ft, info = chart_atlas(torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev), R, pad, stats=st)
    torch.cuda.synchronize()
    assert vt.dtype == torch.float32 and ft.dtype == torch.int64 and info["face_chart"].dtype == torch.int32
    assert info["chart_rect"].dtype == torch.int32 and info["chart_rect"].shape[1] == 4
    assert st["rounds"] == info["rounds"] and st["k"] == info["k"] and st["charts"] == info["chart_rect"].shape[0]
    return dict(vt=vt.cpu().numpy(), ft=ft.cpu().numpy(), face_chart=info["face_chart"].cpu().numpy(),
                chart_rect=info["chart_rect"].cpu().numpy(), chart_axis=info["chart_axis"].cpu().numpy(),
                scale=info["scale"], k=info["k"], evicted=info["evicted_faces"].cpu().numpy(), rounds=info["rounds"],
                n_evicted=info["evicted"])


@functools.lru_cache(maxsize=None)
def _ref(name):
    v, f, R = _mesh(name)
    return A.chart_atlas(v, f, R)


def _mesh(name):
    fixed = {"cube": (A.cube, 64), "octahedron": (A.octahedron, 64), "helicoid": (A.helicoid, 128), "zoo": (A.topology_zoo, 128)}
    if name in fixed:
        return fixed[name][0]() + (fixed[name][1],)
    if name == "icosphere":
        from src.latent_nerf.training.shape import make_icosphere
        v, f = make_icosphere(2)
        return v.numpy(), f.numpy().astype(np.int32), 128
    kind, n, R = {"sphere16": ("sphere", 16, 128), "torus16": ("torus", 16, 128), "blob32": ("blob", 32, 256),
                  "sphere32": ("sphere", 32, 256)}[name]
    return A.mc_mesh(kind, n) + (R,)


def _same(got, ref):
    assert np.array_equal(got["face_chart"], ref["face_chart"])
    assert np.array_equal(got["chart_axis"], ref["chart_axis"])
    assert (got["k"], got["scale"]) == (ref["k"], ref["scale"])
    assert np.array_equal(got["chart_rect"], ref["chart_rect"])
    assert np.array_equal(got["evicted"], ref["evicted"]) and got["n_evicted"] == len(ref["evicted"])
    assert np.array_equal(got["ft"], ref["ft"])
    assert got["vt"].shape == ref["vt"].shape and np.array_equal(got["vt"].view(np.uint32), ref["vt"].view(np.uint32))


def _checked(dev, name):
    from src.latent_nerf.raymarching import backend as B
    v, f, R = _mesh(name)
    got = _op(dev, v, f, R)
    _same(got, _ref(name))
    A.check_properties(v, f, got, R)
    assert 1 <= got["rounds"] <= B.ATLAS_MAX_ROUNDS
    return v, f, R, got


def test_cube_six_charts_in_axis_order(dev):
    v, f, R, got = _checked(dev, "cube")
    assert got["chart_axis"].tolist() == [0, 1, 2, 3, 4, 5]
    assert got["face_chart"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5] and len(got["vt"]) == 24
    # axis-aligned faces keep their area: UV area = 3D area * s^2 / R^2 up to the rounding of the corners
    area = A.uv_area(got["vt"], got["ft"]) * R * R / got["scale"] ** 2
    # corners move by <= 8 R 2^-24 texels (atlas_reference.check_properties), the perimeter is (2 + sqrt 2) s texels
    assert np.abs(area - 0.5).max() <= 8 * R * 2.0 ** -24 * 3.5 / got["scale"]


def test_octahedron_ties_take_the_first_maximum(dev):
    v, f, R, got = _checked(dev, "octahedron")
    assert got["chart_axis"].tolist() == [0, 1] and got["face_chart"].tolist() == [0, 1, 1, 0, 0, 1, 1, 0]


def test_icosphere_matches_and_has_every_property(dev):
    v, f, R, got = _checked(dev, "icosphere")
    assert len(f) == 320 and got["n_evicted"] == 0 and 6 <= len(got["chart_axis"]) < 64


@pytest.mark.parametrize("name", ["sphere16", "torus16", "blob32"])
def test_gpu_marching_cubes_meshes(dev, name):
    """The mesh comes from the GPU's marching cubes (bit-equal to the restatement's, which the reference atlas uses)."""
    from src.latent_nerf.raymarching import chart_atlas, marching_cubes
    kind, n = {"sphere16": ("sphere", 16), "torus16": ("torus", 16), "blob32": ("blob", 32)}[name]
    v, f, R = _mesh(name)
    gv, gf, _ = marching_cubes(torch.from_numpy(A.field(kind, n)).to(dev), 0.0, (-1, -1, -1), (1, 1, 1))
    assert np.array_equal(gv.cpu().numpy().view(np.uint32), v.view(np.uint32)) and np.array_equal(gf.cpu().numpy(), f)
    vt, ft, info = chart_atlas(gv, gf, R)
    ref = _ref(name)
    assert np.array_equal(vt.cpu().numpy().view(np.uint32), ref["vt"].view(np.uint32))
    assert np.array_equal(ft.cpu().numpy(), ref["ft"]) and info["evicted"] == 0
    v, f, R, got = _checked(dev, name)
    if name == "blob32":                                 # more than one workgroup per pass and per scan
        assert len(f) > 3000 and len(got["chart_axis"]) < 64


def test_helicoid_evicts_what_the_reference_evicts(dev):
    v, f, R, got = _checked(dev, "helicoid")
    assert len(f) == 384 and got["n_evicted"] == len(_ref("helicoid")["evicted"]) > 0
    assert A.strict_coverage_count(got["vt"], got["ft"], R).max() <= 1
    assert len(got["chart_axis"]) == 1 + got["n_evicted"] and (got["chart_axis"] == 2).all()


def test_topology_edge_cases(dev):
    v, f, R, got = _checked(dev, "zoo")
    fc = got["face_chart"]
    assert fc[0] == fc[1] and fc[2] == fc[3] and fc[0] != fc[2]        # stacked squares: two charts ...
    rect = got["chart_rect"]
    a, b = rect[fc[0]], rect[fc[2]]
    assert a[0] + a[2] <= b[0] or b[0] + b[2] <= a[0] or a[1] + a[3] <= b[1] or b[1] + b[3] <= a[1]   # ... no shared texel
    assert len({fc[4], fc[5], fc[6]}) == 3                             # three faces on one edge
    assert len(set(fc[7:15].tolist())) == 1                            # the open strip
    assert (fc == fc[15]).sum() == 1 and got["chart_axis"][fc[15]] == 0   # the zero-area face
    assert fc[16] != fc[17]                                            # the reversed copy


def test_out_of_range_index_is_refused_and_counted(dev):
    from src.latent_nerf.raymarching import chart_atlas
    v, f = A.cube()
    bad = f.copy()
    bad[3, 1], bad[7, 0], bad[7, 2] = 8, -1, 1 << 30
    with pytest.raises(ValueError, match="2 faces index outside verts"):
        chart_atlas(torch.from_numpy(v).to(dev), torch.from_numpy(bad).to(dev), 64)
    torch.cuda.synchronize()
    # and an empty mesh is an empty atlas
    vt, ft, info = chart_atlas(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev, dtype=torch.int32), 64)
    assert vt.shape == (0, 2) and ft.shape == (0, 3) and info["chart_rect"].shape == (0, 4)


def test_two_calls_give_identical_bits(dev):
    for name in ("blob32", "helicoid"):
        v, f, R = _mesh(name)
        a, b = _op(dev, v, f, R), _op(dev, v, f, R)
        _same(a, b)


def _round_trip_reference(v, f, vt, ft, R, gutter):
    """max over faces and the two barycentric points of |bilinear(baked positions)(uv) - point|, all in numpy."""
    _, idx, pos, _, _ = U.uv_raster(v, f, vt, ft, R)
    tex = np.zeros((3, R * R), np.float32)
    tex[:, idx] = pos.T
    mask = np.zeros(R * R, np.uint8)
    mask[idx] = 2
    tex, _ = U.uv_dilate(tex.reshape(3, R, R), mask.reshape(R, R), gutter)
    worst = 0.0
    for b in BARY:
        uv = (vt.astype(np.float64)[ft] * np.array(b)[None, :, None]).sum(1)
        pt = (v.astype(np.float64)[f] * np.array(b)[None, :, None]).sum(1)
        worst = max(worst, float(np.linalg.norm(A.bilinear(tex, uv) - pt, axis=1).max()))
    return worst


BARY = ((1 / 3, 1 / 3, 1 / 3), (0.6, 0.2, 0.2))


def test_position_round_trip_through_the_bake(dev):
    """Bake fn(x) = x over the chart atlas of the 32^3 sphere (R = 256, gutter 4), look two barycentric points per face
    up through Latent-Paint's bilinear texture_map, compare with the true point.

    The issue's bound was 3 / s (in-plane error <= sqrt(2) / s where a tap is a gutter texel, dropped coordinate <= 2 / s).
    The numpy restatement of the same measurement (uv_reference.uv_raster + uv_dilate + a numpy bilinear) gives
    0.04455 = 4.30 / s at s = 96.526, so that derivation is short: a gutter tap is itself the MEAN of covered texels up
    to a texel diagonal further out, which doubles the reach (<= 2 sqrt(2) / s in the plane, times the slope sqrt(2) in
    the dropped coordinate: 4 / s and more for slivers whose own texel centre is not covered).  As the issue rules for
    that case, the GPU result is held to the restatement's own maximum with 0.1 % slack.  For information, the
    per-triangle atlas at the same R measures 0.00004 (every sample sits well inside its own face's cell)."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    from src.latent_paint.models.render import _TextureMap
    from src.uv_atlas import per_triangle_atlas
    v, f, R = _mesh("sphere32")
    tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
    net = NeRFNetwork(RenderConfig(grid_size=32, train_h=16, train_w=16), log2_hashmap_size=12).to(dev)
    got = _op(dev, v, f, R)
    _same(got, _ref("sphere32"))
    s = got["scale"]

    def measure(vt, ft):
        tex = net.bake_texture(tv, tf, vt, ft, resolution=R, gutter=4, S=32, fn=lambda pts: pts)["texture"]
        worst = 0.0
        for b in BARY:
            w = torch.tensor(b, device=dev, dtype=torch.float32)
            uv = (vt[ft] * w[None, :, None]).sum(1).contiguous()
            pt = (tv[tf.long()].double() * w.double()[None, :, None]).sum(1)
            look = _TextureMap.apply(tex[None], uv, torch.zeros(uv.shape[0], device=dev, dtype=torch.int32), 1)
            worst = max(worst, float((look.double() - pt).norm(dim=1).max()))
        return worst

    charts = measure(torch.from_numpy(got["vt"]).to(dev), torch.from_numpy(got["ft"]).to(dev))
    ref = _round_trip_reference(v, f, got["vt"], got["ft"], R, 4)
    tri = measure(*per_triangle_atlas(len(f), dev))
    print("round trip: charts %.5f (%.2f / s, s = %.3f), restatement %.5f, 3 / s = %.5f; per-triangle %.5f"
          % (charts, charts * s, s, ref, 3 / s, tri))
    assert ref > 3 / s                                   # the documented finding; should it ever hold, assert 3 / s again
    assert charts <= ref * 1.001


def _nerf(dev):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    cfg = RenderConfig(grid_size=32, train_h=16, train_w=16)
    return NeRFNetwork(cfg, log2_hashmap_size=14).to(dev), cfg


def _paint_cfg(tmp_path, name, shape, R, **over):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": name, "log.exp_root": str(tmp_path), "guide.text": "a goldfish", "guide.shape_path": str(shape),
            "guide.texture_resolution": R, "guide.texture_interpolation_mode": "bilinear", "optim.iters": 1,
            "log.save_interval": 100, "log.eval_size": 1, "log.full_eval_size": 1, "render.eval_grid_size": 64,
            "log.save_mesh": False}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def test_export_mesh_with_charts_end_to_end(dev, tmp_path):
    import warnings

    from src.latent_paint.models.mesh import Mesh, read_obj
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    net, cfg = _nerf(dev)
    R = 256
    with warnings.catch_warnings():
        warnings.simplefilter("error")                   # no per-triangle resolution warning for the chart atlas
        out = net.export_mesh(str(tmp_path), resolution=32, S=32, thresh=cfg.density_thresh, texture_resolution=R,
                              atlas="charts")
    F = out["faces"].shape[0]
    assert F > 100 and out["vt"].shape[0] < 3 * F and out["ft"].shape == (F, 3)
    assert out["face_chart"].shape == (F,) and out["chart_rect"].shape[1] == 4 and out["atlas_scale"] > 0
    assert {"mesh.obj", "mesh.mtl", "albedo.png", "latent_texture.pt"} <= {p.name for p in tmp_path.iterdir()}
    ref = A.chart_atlas(out["verts"].cpu().numpy(), out["faces"].cpu().numpy(), R)
    assert np.array_equal(out["vt"].cpu().numpy().view(np.uint32), ref["vt"].view(np.uint32))
    assert np.array_equal(out["ft"].cpu().numpy(), ref["ft"])
    v, f, vt, ft = read_obj(str(tmp_path / "mesh.obj"))
    assert torch.equal(vt, out["vt"].cpu()) and torch.equal(ft, out["ft"].cpu())
    mesh = Mesh(str(tmp_path / "mesh.obj"), dev)
    assert torch.equal(mesh.vt.cpu(), out["vt"].cpu()) and torch.equal(mesh.ft.cpu(), out["ft"].cpu())
    pcfg = _paint_cfg(tmp_path, "paint", tmp_path / "mesh.obj", R, **{"guide.init_texture": str(tmp_path / "latent_texture.pt")})
    model = TexturedMeshModel(pcfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=R)
    assert torch.equal(model.vt.cpu(), out["vt"].cpu())
    img = model.render(math.radians(60.0), math.radians(30.0), 1.25)["image"]
    torch.cuda.synchronize()
    assert img.shape[-2:] == (64, 64) and bool(torch.isfinite(img).all())
    with pytest.raises(ValueError, match="atlas"):
        net.export_mesh(str(tmp_path / "bad"), resolution=32, S=32, thresh=cfg.density_thresh, texture_resolution=R, atlas="x")


def test_latent_paint_builds_caches_and_reloads_the_chart_atlas(dev, tmp_path):
    from src.latent_nerf.training.shape import make_icosphere
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    v, f = make_icosphere(2)
    v, f = v.numpy(), f.numpy()
    shape = tmp_path / "ico.obj"
    shape.write_text("".join("v %r %r %r\n" % tuple(float(x) for x in p) for p in v) +
                     "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))
    pcfg = _paint_cfg(tmp_path, "ico", shape, 128, **{"guide.uv_atlas": "charts"})
    m = TexturedMeshModel(pcfg, device=dev, render_grid_size=64, texture_resolution=128)
    ref = A.chart_atlas(m.mesh.vertices.cpu().numpy(), m.mesh.faces.cpu().numpy(), 128)
    assert np.array_equal(m.vt.cpu().numpy().view(np.uint32), ref["vt"].view(np.uint32))
    assert np.array_equal(m.ft.cpu().numpy(), ref["ft"]) and m.vt.shape[0] < 3 * len(f)
    cache = tmp_path / "ico"
    assert torch.equal(torch.load(cache / "vt.pth", weights_only=True), m.vt.cpu())
    pcfg2 = _paint_cfg(tmp_path, "ico", shape, 128)                   # the flag left alone: the cache wins
    m2 = TexturedMeshModel(pcfg2, device=dev, render_grid_size=64, texture_resolution=128)
    assert torch.equal(m2.vt, m.vt) and torch.equal(m2.ft, m.ft)
    img = m.render(math.radians(60.0), math.radians(30.0), 1.25)["image"]
    assert bool(torch.isfinite(img).all())
