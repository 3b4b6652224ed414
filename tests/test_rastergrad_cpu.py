"""CPU side of the vertex-gradient kernels (csrc/rastergrad.hip): the float64 reference of tests/rastergrad_reference.py is
checked against central differences and against the properties the kernels are held to, the shared scenes are checked to
put no decision on a rounding edge, and the config / model plumbing is checked to be off by default."""
import pytest
import torch

from tests import rastergrad_reference as RG


def _scene(H, W):
    fxy, fz, faces = RG.screen_scene()
    return fxy, fz, faces, RG.oracle_face_idx(fxy, fz, H, W)


def _info(H, W):
    fxy, fz, faces, idx = _scene(H, W)
    info = {}
    b = RG.bary(idx, fxy, fz, H, W)
    RG.antialias(RG.scene_image(2, H, W), idx, b, fxy, fz, faces, info=info)
    return info, idx, b


# ------------------------------------------------------------------------------------------------ preconditions
def _check_pairs(info):
    for pr in (info["h"], info["v"]):
        ev = pr["differ"]
        assert bool((pr["ddepth"][ev] > 1e-4).all())
        t_all = pr["t_all"][pr["cross_all"]]                      # every crossing edge of an evaluated pair
        assert bool(((t_all - 0).abs() > 1e-3).all()) and bool(((t_all - 1).abs() > 1e-3).all())
        t = pr["t"][ev & pr["any_ok"]]
        assert bool(((t - 0.5).abs() > 1e-3).all())


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_no_decision_of_the_screen_scene_sits_on_a_rounding_edge(H, W):
    info, idx, _ = _info(H, W)
    _check_pairs(info)
    fxy, fz, faces = RG.screen_scene()
    assert int((idx == 8).sum()) == 0 and int((idx == 9).sum()) == 0     # behind the camera, degenerate: never win
    assert all(int((idx == f).sum()) > 0 for f in range(8))


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_every_kind_of_pair_occurs_in_the_screen_scene(H, W):
    info, idx, _ = _info(H, W)
    for key in ("h", "v"):
        pr = info[key]
        ok, t = pr["ok"], pr["t"]
        assert bool((ok & (t < 0.5)).any()) and bool((ok & (t >= 0.5)).any()), key
        assert bool((ok & pr["far_face"]).any()) and bool((ok & ~pr["far_face"]).any()), key
        assert bool((pr["differ"] & pr["shared"] & pr["any_ok"]).any()), key      # rule 3 skips interior edges
    # pairs that touch the image border (first / last column of a horizontal pair, first / last row of a vertical one)
    assert bool(info["h"]["ok"][:, :, 0].any() or info["h"]["ok"][:, :, -1].any() or info["v"]["ok"][:, 0].any()
                or info["v"]["ok"][:, -1].any() or info["h"]["ok"][:, 0].any() or info["h"]["ok"][:, -1].any()
                or info["v"]["ok"][:, :, 0].any() or info["v"]["ok"][:, :, -1].any())


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_no_decision_of_the_chain_scene_sits_on_a_rounding_edge(H, W):
    verts, faces, cams, face_uv, tex = RG.chain_scene()
    fxy, fz = RG.prepare(verts, faces, cams)
    idx = RG.oracle_face_idx(fxy, fz, H, W)
    extra = {}
    RG.render_chain(verts, faces, cams, idx, face_uv, tex, H, W, extra=extra)
    _check_pairs(extra)
    assert bool((extra["h"]["ok"].any())) and bool(extra["v"]["ok"].any())
    fg = idx >= 0
    R = tex.shape[-1]
    for c in RG.texel_position(extra["uv"][fg], R):
        assert bool(((c - c.round()).abs() > 1e-3).all())                 # off every texel boundary
        assert bool((c > 1e-3).all()) and bool((c < R - 1 - 1e-3).all())  # no clamp active
    b = extra["bary"][fg]
    assert bool((b > 1e-4).all())                                         # no winner decided on an edge


@pytest.mark.parametrize("R", (4, 8))
def test_no_uv_of_the_lookup_scene_sits_on_a_texel_boundary_or_clamp(R):
    uv, _ = RG.uv_scene(R)
    for c, raw in zip(RG.texel_position(uv.clamp(0, 1), R), (uv[:, 0], uv[:, 1])):
        assert bool(((c - c.round()).abs() > 1e-3).all())
        assert bool(((c - 0).abs() > 1e-3).all()) and bool(((c - (R - 1)).abs() > 1e-3).all())
        assert bool(((raw - 0).abs() > 1e-3).all()) and bool(((raw - 1).abs() > 1e-3).all())
    assert bool(((uv < 0) | (uv > 1)).any(0).all())                       # both axes have clamped points


# ------------------------------------------------------------------------------------------------ gradients
def _central(fn, x, eps=1e-6):
    g = torch.zeros_like(x)
    flat = x.reshape(-1)
    for k in range(flat.numel()):
        hi, lo = flat.clone(), flat.clone()
        hi[k] += eps
        lo[k] -= eps
        g.reshape(-1)[k] = (fn(hi.reshape(x.shape)) - fn(lo.reshape(x.shape))) / (2 * eps)
    return g


def test_reference_gradients_agree_with_central_differences():
    H, W = 13, 11
    fxy, fz, faces, idx = _scene(H, W)
    img, gout = RG.scene_image(2, H, W), RG.randn((2, H, W, RG.C_IMAGE), 21)
    b = RG.bary(idx, fxy, fz, H, W)
    _, gimg, gxy = RG.case_antialias(idx, faces, H, W)(img.clone(), gout, fxy.clone(), fz)
    fd = _central(lambda x: float((RG.antialias(img, idx, b, x, fz, faces) * gout).sum()), fxy)
    assert float((fd - gxy).abs().max()) <= 1e-6 * float(gxy.abs().max()) and float(gxy.abs().max()) > 0
    gb = RG.randn((2 * H * W, 3), 22)
    gxy2, gz2 = RG.case_bary(idx, H, W)(gb, fxy.clone(), fz.clone())
    fd = _central(lambda x: float((RG.bary(idx, x, fz, H, W) * gb).sum()), fxy)
    assert float((fd - gxy2).abs().max()) <= 1e-6 * float(gxy2.abs().max())
    fd = _central(lambda z: float((RG.bary(idx, fxy, z, H, W) * gb).sum()), fz)
    assert float((fd - gz2).abs().max()) <= 1e-6 * float(gz2.abs().max())
    verts, cams = RG.prepare_scene()
    gxy3, gz3 = RG.randn((3, 5, 3, 2), 28), RG.randn((3, 5, 3), 29)
    (gv,) = RG.case_prepare(RG.PREPARE_FACES)(verts.clone(), cams, gxy3, gz3)
    fd = _central(lambda v: float(sum((o * w).sum() for o, w in zip(RG.prepare(v, RG.PREPARE_FACES, cams), (gxy3, gz3)))),
                  verts)
    assert float((fd - gv).abs().max()) <= 1e-6 * float(gv.abs().max())
    assert float(gv[6].abs().max()) == 0.0                                  # the vertex in no face


def test_lookup_gradient_is_zero_where_a_clamp_is_active():
    uv, idx = RG.uv_scene(8)
    (g,) = RG.case_texture(idx)(RG.randn((3, 8, 8), 26), uv.clone(), RG.randn((uv.shape[0], 3), 27))
    out = (uv < 0) | (uv > 1)
    assert bool((g[out] == 0).all()) and float(g[5, 0]) == 0.0 and bool((g[-8:] == 0).all())
    assert bool((g[6:-8] != 0).all())


def test_antialiasing_leaves_a_constant_image_unchanged():
    for H, W in RG.SIZES:
        fxy, fz, faces, idx = _scene(H, W)
        img = torch.full((2, H, W, 3), 0.375, dtype=torch.float64)
        assert torch.equal(RG.antialias(img, idx, RG.bary(idx, fxy, fz, H, W), fxy, fz, faces), img)


def test_umbrella_of_a_constant_is_zero_and_its_transpose_is_autograds():
    for faces, V in ((RG.FAN_FACES, 6), (RG.TETRA_FACES, 4)):
        const = torch.full((V, 3), 1.75, dtype=torch.float64)
        L = RG.umbrella(const, faces)
        used = torch.zeros(V, dtype=torch.bool)
        used[faces.reshape(-1)] = True
        assert float(L[used].abs().max()) <= 1e-15 and torch.equal(L[~used], const[~used])
        x = RG.randn((V, 3), 30).requires_grad_()
        y = RG.randn((V, 3), 31)
        (g,) = torch.autograd.grad((RG.umbrella(x, faces) * y).sum(), x)
        assert float((g - RG.umbrella(y, faces, transpose=True)).abs().max()) <= 1e-14


# ------------------------------------------------------------------------------------------------ config and model
def _cfg(**flat):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    base = {"log.exp_name": "t", "guide.shape_path": "shapes/blub.obj"}
    base.update(flat)
    return apply_overrides(TrainConfig(), base)


def test_validate_rules_of_the_geometry_options():
    good = {"optim.disp_lr": 5e-5, "render.antialias": True, "guide.texture_interpolation_mode": "bilinear"}
    _cfg(**good).validate()
    _cfg(**{"render.antialias": True}).validate()                          # antialiasing alone is allowed
    for bad in ({"optim.disp_lr": -1e-5}, {"optim.lap_weight": -1.0}, {"optim.reg_weight": -0.5},
                {**good, "guide.texture_interpolation_mode": "nearest"},
                {**good, "guide.texture_interpolation_mode": "mipmap"},
                {**good, "render.antialias": False}):
        with pytest.raises(ValueError):
            _cfg(**bad).validate()


def test_the_default_config_has_none_of_the_new_behaviour(tmp_path):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    cfg = _cfg().validate()
    assert cfg.render.antialias is False and cfg.optim.disp_lr == 0.0
    assert (cfg.optim.lap_weight, cfg.optim.reg_weight) == (100.0, 10.0)
    cfg.log.exp_root = tmp_path
    cfg.guide.shape_path = RG.RB.SHAPES + "/blub.obj"
    cfg.guide.texture_resolution = 8
    model = TexturedMeshModel(cfg, render_grid_size=16, texture_resolution=8)
    assert sorted(model.state_dict()) == ["background_sphere_colors", "texture_img", "texture_img_rgb_finetune"]
    assert model.get_geometry_params() == [] and not model.renderer.antialias and not model.learn_geometry
    assert model.surface_vertices() is model.mesh.vertices
    cfg2 = _cfg(**{"optim.disp_lr": 5e-5, "render.antialias": True, "guide.texture_interpolation_mode": "bilinear"})
    cfg2.log.exp_root, cfg2.guide.shape_path, cfg2.guide.texture_resolution = tmp_path, cfg.guide.shape_path, 8
    geo = TexturedMeshModel(cfg2, render_grid_size=16, texture_resolution=8)
    assert "displacement" in geo.state_dict() and geo.get_geometry_params()[0] is geo.displacement
    assert geo.displacement.shape == geo.mesh.vertices.shape and float(geo.displacement.detach().abs().max()) == 0.0
    assert len(geo.get_params()) == 2
