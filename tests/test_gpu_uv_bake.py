"""Texture baking on the MI355X: lnerf_uv_raster / lnerf_uv_dilate against the numpy restatement (tests/uv_reference.py,
bit for bit), argument errors, the texel convention through Latent-Paint's own texture lookup, the field bake,
NeRFRenderer.export_mesh(texture_resolution=...) end to end, Latent-Paint starting from the export and the NeRF
trainer's log.mesh_texture_resolution."""
import math
import os

import numpy as np
import pytest
import torch

from tests import uv_reference as U

pytestmark = pytest.mark.gpu

SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")
BLUB = os.path.join(SHAPES, "blub.obj")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _blub():
    from src.latent_paint.models.mesh import read_obj
    v, f, vt, ft = read_obj(BLUB)
    return v.numpy(), f.numpy(), vt.numpy(), ft.numpy()


def _sphere_mesh(dev, n=32):
    from src.latent_nerf.raymarching import marching_cubes
    a = torch.linspace(-1, 1, n)
    X, Y, Z = torch.meshgrid(a, a, a, indexing="ij")
    vol = (0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).float().to(dev)
    v, f, _ = marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    return v.cpu().numpy(), f.cpu().numpy()


def _cases(dev):
    from src.uv_atlas import atlas_min_resolution, per_triangle_atlas
    rng = np.random.default_rng(7)
    bv, bf, bvt, bft = _blub()
    sv, sf = _sphere_mesh(dev)
    svt, sft = per_triangle_atlas(len(sf), "cpu")
    # random overlapping triangles: many texels covered by several faces (the max-index rule)
    F = 300
    rv = rng.standard_normal((3 * F, 3)).astype(np.float32)
    rvt = rng.uniform(0.1, 0.9, (3 * F, 2)).astype(np.float32)
    rf = np.arange(3 * F).reshape(F, 3)
    # degenerate (zero area, collinear, coincident corners) and NaN / inf UVs mixed with ordinary faces
    dvt = rng.uniform(0, 1, (3 * F, 2)).astype(np.float32)
    dvt[0:3] = 0.25
    dvt[3:6] = [[0.1, 0.1], [0.5, 0.5], [0.9, 0.9]]
    dvt[6, 0] = np.nan
    dvt[10, 1] = np.inf
    dvt[14] = [-np.inf, np.nan]
    dvt[18:21] = [[0.3, 0.3], [0.3, 0.3], [0.7, 0.2]]
    # triangles partly (or wholly) outside [0,1]^2
    ovt = (rng.uniform(-0.4, 1.4, (F, 1, 2)) + rng.uniform(-0.15, 0.15, (F, 3, 2))).reshape(-1, 2).astype(np.float32)
    ovt[0:3] = [[-5.0, -5.0], [6.0, -5.0], [0.5, 7.0]]          # one triangle much larger than the texture
    ovt[3:6] = [[2.0, 2.0], [3.0, 2.0], [2.0, 3.0]]             # nowhere near it
    # two triangles over most of a 1024 x 1024 texture: 4096 blocks of texels, so a thread of the top-level scan owns four
    qv = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    qvt = np.float32([[0.05, 0.05], [0.95, 0.05], [0.95, 0.95], [0.05, 0.95]])
    qf = np.array([[0, 1, 2], [0, 2, 3]])
    return [("blub256", bv, bf, bvt, bft, 256), ("blub300", bv, bf, bvt, bft, 300),
            ("sphere_atlas", sv, sf, svt.numpy(), sft.numpy(), atlas_min_resolution(len(sf))),
            ("overlap", rv, rf, rvt, rf, 97), ("degenerate", rv, rf, dvt, rf, 64), ("outside", rv, rf, ovt, rf, 50),
            ("quad1024", qv, qf, qvt, qf, 1024)]


CASE_NAMES = ["blub256", "blub300", "sphere_atlas", "overlap", "degenerate", "outside", "quad1024"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASE_NAMES)
def test_op_matches_restatement_bit_for_bit(dev, case):
    from src.latent_nerf.raymarching import uv_dilate, uv_raster
    name, v, f, vt, ft, R = [c for c in _cases(dev) if c[0] == case][0]
    tf, idx, pos = uv_raster(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.from_numpy(vt).to(dev),
                             torch.from_numpy(ft).to(dev), R)
    torch.cuda.synchronize()
    rtf, ridx, rpos, _, _ = U.uv_raster(v, f, vt, ft, R)
    assert np.array_equal(tf.cpu().numpy(), rtf)
    assert np.array_equal(idx.cpu().numpy(), ridx)
    assert np.array_equal(_bits(pos.cpu().numpy()), _bits(rpos))
    if case == "overlap":
        count, _ = U.coverage_count(v, f, vt, ft, R)
        assert (count >= 2).sum() > 100                              # the rule was exercised
    if case == "degenerate":
        assert not np.isin([0, 1, 2, 3, 4, 6], rtf).any()             # zero-area / non-finite faces cover nothing
    if case == "outside":
        assert rtf.reshape(-1)[ridx].tolist().count(0) > 0 and 1 not in rtf
    if case == "quad1024":
        per_block = (rtf >= 0).reshape(-1, 256).sum(1)                # empty, partly covered and full blocks of texels
        assert [(per_block == 0).sum(), ((per_block > 0) & (per_block < 256)).sum(), (per_block == 256).sum()] \
            == [408, 1844, 1844] and len(ridx) == 850084
    # a gutter over a random texture (C = 4 and C = 3) against the restatement
    rng = np.random.default_rng(R)
    for C, passes in ((4, 4), (3, 3)):
        tex = rng.standard_normal((C, R, R)).astype(np.float32) * (rtf >= 0)[None]
        mask = ((rtf >= 0) * 2).astype(np.uint8)
        gt, gm = uv_dilate(torch.from_numpy(tex).to(dev), torch.from_numpy(mask).to(dev), passes)
        torch.cuda.synchronize()
        wt, wm = U.uv_dilate(tex, mask, passes)
        assert np.array_equal(gm.cpu().numpy(), wm)
        assert np.array_equal(_bits(gt.cpu().numpy()), _bits(wt))


def test_arguments_are_refused_without_a_fault(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching import uv_dilate, uv_raster
    v, f, vt, ft = (torch.from_numpy(x).to(dev) for x in _blub())
    for R in (0, -3, 8193):
        with pytest.raises(ValueError, match="resolution"):
            uv_raster(v, f, vt, ft, R)
    with pytest.raises(_b.LnerfError, match="resolution"):     # the C entry point checks on its own as well
        _b.call("lnerf_uv_raster", None, 0, None, None, 0, None, 0, 9000, _b.UV_ITEMS, 0, None, 0, None, None, None, 0,
                None, None)
    bad_f = f.clone()
    bad_f[5, 1] = v.shape[0]
    with pytest.raises(ValueError, match="1 faces index outside"):
        uv_raster(v, bad_f, vt, ft, 64)
    bad_ft = ft.clone()
    bad_ft[7, 2] = -1
    bad_ft[9, 0] = vt.shape[0] + 100
    with pytest.raises(ValueError, match="2 faces index outside"):
        uv_raster(v, f, vt, bad_ft, 64)
    with pytest.raises(ValueError):
        uv_dilate(torch.zeros(4, 8, 8, device=dev), torch.zeros(8, 9, dtype=torch.uint8, device=dev), 1)
    tf, idx, _ = uv_raster(v, f, vt, ft, 64)                       # the device is fine afterwards
    torch.cuda.synchronize()
    assert idx.shape[0] == int((tf >= 0).sum()) > 0


def _probe(p):
    return torch.stack([p[:, 0], p[:, 1], p[:, 2], p[:, 0] * p[:, 1]], -1)


def test_bake_lines_up_with_latent_paint_texture_lookup(dev):
    """Bake fn(x) = (x, y, z, x*y) onto blub with its own UVs, render it through Latent-Paint's raster path (bilinear
    texture_map on the interpolated UVs, 256 x 256, two views) and compare with fn at the rasterised surface point
    (positions interpolated as face attributes).  Compared: pixels whose 3 x 3 texels around the sample all belong to
    the pixel's own face.  There fn is linear in (u, v) in its first three channels and x*y bends by far less than one
    texel's change, so a lookup in the right convention reproduces fn: |error| <= 0.01 d + 1e-6 at every pixel, with
    d the largest change of the baked texture from the sample's texel to its 8 neighbours (one texel, h = 1/R in uv).
    A lookup half a texel off in u or in v errs by up to d / 2, a flipped v by far more: both are checked to fail."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    from src.latent_paint.models.mesh import Mesh
    from src.latent_paint.models.render import Renderer, _InterpAttr, _TextureMap
    mesh = Mesh(BLUB, dev)
    mesh.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    net = NeRFNetwork(RenderConfig(grid_size=32, train_h=16, train_w=16), log2_hashmap_size=12).to(dev)
    R = 1024
    baked = net.bake_texture(mesh.vertices, mesh.faces, mesh.vt, mesh.ft, resolution=R, gutter=4, S=32, fn=_probe)
    tex, tmask = baked["texture"], baked["mask"]
    assert tex.shape == (4, R, R) and baked["rgb"].shape == (3, R, R)
    from src.latent_nerf.raymarching import uv_raster
    texel_face = uv_raster(mesh.vertices, mesh.faces, mesh.vt, mesh.ft, R)[0].long()
    pad_face = torch.nn.functional.pad(texel_face, (1, 1, 1, 1), value=-1)
    pad_tex = torch.nn.functional.pad(tex[None], (1, 1, 1, 1), mode="replicate")[0]
    renderer = Renderer(device=dev, dim=(256, 256), interpolation_mode="bilinear")
    uv_attr = mesh.vt[mesh.ft].contiguous()
    pos_attr = mesh.vertices[mesh.faces].contiguous()
    checked = 0
    for theta, phi in ((60.0, 30.0), (100.0, 200.0)):
        face_idx, bary, H, W = renderer._rasterize(mesh.vertices, mesh.faces, math.radians(theta), math.radians(phi),
                                                   1.25, 0.25, renderer.dim)
        with torch.no_grad():
            uv = _InterpAttr.apply(uv_attr, face_idx, bary).contiguous()
            pts = _InterpAttr.apply(pos_attr, face_idx, bary)
        hit = face_idx >= 0
        i = torch.clamp(((1 - uv[:, 1]) * R).floor().long(), 0, R - 1)
        j = torch.clamp((uv[:, 0] * R).floor().long(), 0, R - 1)
        inside = hit.clone()
        d = torch.zeros(uv.shape[0], 4, device=dev)
        centre = tex[:, i, j].T
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                inside &= pad_face[i + 1 + di, j + 1 + dj] == face_idx.long()
                d = torch.maximum(d, (pad_tex[:, i + 1 + di, j + 1 + dj].T - centre).abs())
        ok = inside
        assert int(ok.sum()) > 200, int(ok.sum())
        assert bool((tmask.reshape(-1)[(i * R + j)[ok]] == 2).all())
        want = _probe(pts)[ok]
        dk = d[ok]

        def err(uv_in):
            with torch.no_grad():
                return (_TextureMap.apply(tex[None], uv_in.contiguous(), face_idx, 1)[ok] - want).abs()

        def within(e):
            return bool((e <= 0.01 * dk + 1e-6).all())

        e = err(uv)
        assert within(e), float((e - 0.01 * dk).max())
        assert float(e.mean()) <= 1e-3 * float(dk.mean())
        for shift in ((0.5 / R, 0.0), (0.0, 0.5 / R)):
            assert not within(err(uv + torch.tensor(shift, device=dev)))
        assert not within(err(torch.stack([uv[:, 0], 1 - uv[:, 1]], -1)))
        checked += int(ok.sum())
    assert checked > 1000


def _nerf(dev, precision, nerf_type="latent"):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    kw = dict(grid_size=32, train_h=16, train_w=16, nerf_type=NeRFType(nerf_type))
    if precision == "bf16":
        kw.update(mlp_precision="bf16", table_dtype="bf16", gridtype="blocked")
    cfg = RenderConfig(**kw)
    return NeRFNetwork(cfg, log2_hashmap_size=14).to(dev), cfg


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_field_bake_is_the_field_at_the_texel_points(dev, precision):
    from src.latent_nerf.raymarching import uv_raster
    net, _ = _nerf(dev, precision)
    v, f, vt, ft = (torch.from_numpy(x).to(dev) for x in _blub())
    v = v - v.mean(0)
    v = 0.9 * v / v.abs().max()
    R = 256
    baked = net.bake_texture(v, f, vt, ft, resolution=R, gutter=2, S=24)     # 13824-point chunks
    _, idx, pos = uv_raster(v, f, vt, ft, R)
    with torch.no_grad():
        _, feats = net.field(pos, pos.shape[0])
    got = baked["texture"].reshape(4, -1)[:, idx.long()].T.contiguous()
    assert torch.equal(got.view(torch.int32), feats.float().contiguous().view(torch.int32))
    assert int((baked["mask"] == 2).sum()) == idx.shape[0] and int((baked["mask"] == 1).sum()) > 0
    from src.latent_nerf.training.guidance import LATENT_TO_RGB
    m = torch.tensor(LATENT_TO_RGB, device=dev)
    want_rgb = ((baked["texture"].reshape(4, -1).T @ m) / 2 + 0.5).clamp(0, 1).T.reshape(3, R, R)
    assert torch.equal(baked["rgb"], want_rgb)


@pytest.mark.parametrize("nerf_type", ["latent", "rgb"])
def test_export_mesh_textured_end_to_end(dev, tmp_path, nerf_type):
    from PIL import Image

    from src.latent_paint.models.mesh import read_obj
    net, cfg = _nerf(dev, "f32", nerf_type)
    out = net.export_mesh(str(tmp_path), resolution=64, S=32, thresh=cfg.density_thresh, texture_resolution=512)
    F = out["faces"].shape[0]
    assert F > 100 and out["texture"].shape == ((4 if nerf_type == "latent" else 3), 512, 512)
    names = {p.name for p in tmp_path.iterdir()}
    assert {"mesh.obj", "mesh.mtl", "albedo.png"} <= names
    assert ("latent_texture.pt" in names) == (nerf_type == "latent")
    v, f, vt, ft = read_obj(str(tmp_path / "mesh.obj"))
    assert np.array_equal(v.numpy(), out["verts"].cpu().numpy()) and np.array_equal(f.numpy(), out["faces"].cpu().numpy())
    assert torch.equal(vt, out["vt"].cpu()) and torch.equal(ft, out["ft"].cpu())
    assert "map_Kd albedo.png" in (tmp_path / "mesh.mtl").read_text()
    img = np.asarray(Image.open(tmp_path / "albedo.png"))
    assert img.shape == (512, 512, 3) and img.dtype == np.uint8
    assert np.array_equal(img, (out["rgb"].permute(1, 2, 0).cpu().numpy() * 255).round().astype(np.uint8))
    if nerf_type == "latent":
        lt = torch.load(tmp_path / "latent_texture.pt", weights_only=True)
        assert lt.shape == (4, 512, 512) and lt.dtype == torch.float32 and torch.equal(lt, out["texture"].cpu())
    # texture_resolution = 0 is today's vertex-colour file, byte for byte
    plain = net.export_mesh(str(tmp_path / "plain"), resolution=64, S=32, thresh=cfg.density_thresh)
    assert "vt" not in plain and read_obj(plain["path"])[2] is None
    # too few texels per chart cell: a warning that names the resolution needed
    with pytest.warns(UserWarning, match="texture_resolution >= "):
        net.export_mesh(str(tmp_path / "small"), resolution=64, S=32, thresh=cfg.density_thresh, texture_resolution=64)


def test_latent_paint_starts_from_the_export(dev, tmp_path):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.training.trainer import Trainer
    net, cfg = _nerf(dev, "f32")
    R = 256
    net.export_mesh(str(tmp_path / "nerf"), resolution=40, S=32, thresh=cfg.density_thresh, texture_resolution=R)
    lt = torch.load(tmp_path / "nerf" / "latent_texture.pt", weights_only=True)
    flat = {"log.exp_name": "paint", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": str(tmp_path / "nerf" / "mesh.obj"), "guide.init_texture": str(tmp_path / "nerf" /
                                                                                               "latent_texture.pt"),
            "guide.texture_resolution": R, "guide.texture_interpolation_mode": "bilinear", "optim.iters": 1,
            "log.save_interval": 100, "log.eval_size": 1, "log.full_eval_size": 1, "render.eval_grid_size": 64,
            "log.save_mesh": False}
    tr = Trainer(apply_overrides(TrainConfig(), flat).validate(), device=dev)
    assert torch.equal(tr.mesh_model.texture_img.detach().cpu(), lt[None])
    # the mesh's own UVs (the atlas of the export) are what the texture is looked up with
    from src.latent_paint.models.mesh import read_obj
    _, _, vt, ft = read_obj(str(tmp_path / "nerf" / "mesh.obj"))
    assert torch.equal(tr.mesh_model.vt.cpu(), vt) and torch.equal(tr.mesh_model.ft.cpu(), ft)
    tr.train()
    assert tr.train_step == 1
    assert float((tr.mesh_model.texture_img.detach().cpu() - lt[None]).abs().max()) > 0
    bad = dict(flat, **{"guide.texture_resolution": 128, "log.exp_name": "bad"})
    with pytest.raises(ValueError, match="texture_resolution"):
        Trainer(apply_overrides(TrainConfig(), bad).validate(), device=dev)


def test_nerf_trainer_writes_the_textured_set(dev, tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    flat = {"log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32, "render.eval_h": 32,
            "render.eval_w": 32, "render.grid_size": 32, "optim.iters": 4, "log.save_interval": 100,
            "log.eval_size": 1, "log.full_eval_size": 2, "optim.fp16": False, "guide.text": "a lego man",
            "log.exp_name": "t", "log.save_mesh": True, "log.mesh_texture_resolution": 512}
    tr = Trainer(apply_overrides(TrainConfig(), flat), device=dev)
    tr.train()
    names = {p.name for p in (tr.exp_path / "mesh").iterdir()}
    assert {"mesh.obj", "mesh.mtl", "albedo.png", "latent_texture.pt"} <= names
    from src.latent_paint.models.mesh import read_obj
    v, f, vt, ft = read_obj(str(tr.exp_path / "mesh" / "mesh.obj"))
    assert v.shape[0] > 0 and vt is not None and ft.shape == f.shape and int(ft.min()) >= 0
