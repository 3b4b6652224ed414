"""CPU side of the shading kernels (csrc/meshshade.hip): the new entry points are exported and refuse bad arguments before
any launch, the float64 reference of tests/meshshade_reference.py agrees with central differences, `corner_table` agrees with
a Python loop, every scene the GPU tests compare on keeps its decisions off a rounding edge, and the config refuses what
the feature cannot do."""
import ctypes

import pytest
import torch

from tests import meshshade_reference as MS
from tests import rastergrad_reference as RG

NEW = ("lnerf_vertex_normals_forward", "lnerf_vertex_normals_scratch_bytes", "lnerf_vertex_normals_backward",
       "lnerf_raster_shade_forward", "lnerf_raster_shade_backward")
ERR_INVALID_ARG = -1


# ------------------------------------------------------------------------------------------------ symbols and arguments
def test_the_new_entry_points_are_exported_and_bound(built_lib):
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7
    declared = B.header_symbols()
    for name in NEW:
        assert name in declared and name in B._SIGNATURES and hasattr(lib, name), name
    assert B._RESTYPES["lnerf_vertex_normals_scratch_bytes"] is ctypes.c_size_t


def test_every_entry_point_refuses_bad_arguments_before_any_launch(built_lib):
    """The pointers are made up: a call that got past its checks would need a GPU."""
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    P = ctypes.c_void_p(4096)
    Z = ctypes.c_size_t

    def refused(name, *args):
        assert getattr(lib, name)(*args) == ERR_INVALID_ARG, name
        msg = lib.lnerf_last_error().decode()
        assert name[len("lnerf_"):] in msg, (name, msg)

    fwd, bwd = "lnerf_raster_shade_forward", "lnerf_raster_shade_backward"
    for B_, H, W in ((0, 4, 4), (65536, 4, 4), (1, 0, 4), (1, 4, 32768)):
        refused(fwd, P, P, P, P, P, P, B_, H, W, 2, 3, P, P, P, None)
        refused(bwd, P, P, P, P, P, P, P, P, P, B_, H, W, 2, 3, P, P, P, None)
    refused(fwd, P, P, P, P, P, P, 32768, 256, 256, 2, 3, P, P, P, None)                 # B*H*W = 2^31
    refused(bwd, P, P, P, P, P, P, P, P, P, 32768, 256, 256, 2, 3, P, P, P, None)
    refused(fwd, P, P, P, P, P, P, 1, 4, 4, 0, 3, P, P, P, None)                         # n_faces
    refused(fwd, P, P, P, P, P, P, 1, 4, 4, 2, 0, P, P, P, None)                         # n_verts
    refused(bwd, P, P, P, P, P, P, P, P, P, 1, 4, 4, 2, 0, P, P, P, None)
    for k in range(6):                                                                    # a NULL required pointer
        args = [P] * 6
        args[k] = None
        refused(fwd, *args, 1, 4, 4, 2, 3, P, P, P, None)
        refused(bwd, P, P, P, *args, 1, 4, 4, 2, 3, P, P, P, None)
    refused(fwd, P, P, P, P, P, P, 1, 4, 4, 2, 3, None, None, None, None)                # all three outputs NULL
    refused(bwd, None, None, None, P, P, P, P, P, P, 1, 4, 4, 2, 3, P, P, P, None)       # all three gradients NULL
    for k in range(3):                                                                    # every gradient output is required
        outs = [P] * 3
        outs[k] = None
        refused(bwd, P, P, P, P, P, P, P, P, P, 1, 4, 4, 2, 3, *outs, None)

    vf, vb = "lnerf_vertex_normals_forward", "lnerf_vertex_normals_backward"
    need = lib.lnerf_vertex_normals_scratch_bytes(5, 2)
    assert need == 64                                                                     # 5 * 3 floats, padded to 16 bytes
    assert lib.lnerf_vertex_normals_scratch_bytes(0, 2) == 0 and lib.lnerf_vertex_normals_scratch_bytes(5, 0) == 0
    assert lib.lnerf_vertex_normals_scratch_bytes(2 ** 31 // 3 + 1, 2) == 0
    assert lib.lnerf_vertex_normals_scratch_bytes(5, (1 << 28) + 1) == 0
    refused(vf, P, 0, P, 2, P, P, P, None)
    refused(vf, P, 5, P, 0, P, P, P, None)
    refused(vb, P, P, 0, P, 2, P, P, P, Z(need), P, None)
    for k in range(5):
        args = [P, 5, P, 2, P, P, P]
        args[(0, 2, 4, 5, 6)[k]] = None
        refused(vf, *args, None)
    for k in range(6):
        args = [P, P, 5, P, 2, P, P, P, Z(need), P]
        args[(0, 1, 3, 5, 6, 9)[k]] = None
        refused(vb, *args, None)
    refused(vb, P, P, 5, P, 2, P, P, None, Z(need), P, None)                              # no scratch
    refused(vb, P, P, 5, P, 2, P, P, P, Z(need - 1), P, None)                             # scratch too small
    refused(vb, P, P, 5, P, 2, P, P, ctypes.c_void_p(4096 + 4), Z(need), P, None)         # scratch misaligned


# ------------------------------------------------------------------------------------------------ the reference
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
    for name in ("tetra", "fan", "ico1"):   # (the edge cases are discontinuities: they are asserted as zeros instead)
        verts, faces = MS.normal_meshes()[name]
        gvn = MS.randn(tuple(verts.shape), 42)
        _, gv = MS.case_vnormals(faces)(verts.clone(), gvn)
        fd = _central(lambda v: float((MS.vertex_normals(v, faces) * gvn).sum()), verts)
        assert float((fd - gv).abs().max()) <= 1e-6 * float(gv.abs().max()) and float(gv.abs().max()) > 0, name
    H, W = 13, 11
    s = MS.pixel_scene(H, W)
    want = MS.case_shade(s["idx"], s["faces"], H, W)(s["vn"].clone(), s["bary"].clone(), s["fz"].clone(), s["lights"],
                                                      s["gn"], s["gl"], s["gd"])[3:]

    def loss(vn, bary, fz):
        outs = MS.shade(s["idx"], bary, fz, s["faces"], vn, s["lights"], H, W)
        return float(sum((o * g).sum() for o, g in zip(outs, (s["gn"], s["gl"], s["gd"]))))

    for k, (x, g) in enumerate(zip((s["bary"], s["vn"], s["fz"]), want)):
        args = [s["vn"], s["bary"], s["fz"]]
        slot = (1, 0, 2)[k]

        def fn(t):
            a = list(args)
            a[slot] = t
            return loss(*a)

        fd = _central(fn, x)
        assert float((fd - g).abs().max()) <= 1e-6 * float(g.abs().max()) and float(g.abs().max()) > 0, k


@pytest.mark.parametrize("name", ("fan", "tetra", "unused", "out_of_range"))
def test_corner_table_agrees_with_a_python_loop(name):
    from src.latent_paint.models.render import corner_table
    faces, V = {"fan": (MS.fan_mesh()[1], 8), "tetra": (RG.TETRA_FACES, 4), "unused": (RG.PREPARE_FACES, 7),
                "out_of_range": (MS.fan_edge_mesh()[1], 15)}[name]
    start, corners = corner_table(faces, V)
    want_start, want_corners = MS.corner_table_loop(faces, V)
    assert start.dtype == torch.int32 and corners.dtype == torch.int32
    assert start.tolist() == want_start and corners.tolist() == want_corners
    assert len(corners) == faces.numel() and len(start) == V + 1
    if name == "unused":
        assert want_start[6] == want_start[7]                                             # vertex 6 is in no face
    if name == "out_of_range":
        assert corners.tolist()[-1] == -1 and want_start[-1] == faces.numel() - 1         # the corner with id == V is in no list


# ------------------------------------------------------------------------------------------------ preconditions
def test_vertex_normal_meshes_keep_every_length_off_zero_except_the_edge_cases():
    for name, (verts, faces) in MS.normal_meshes().items():
        info = {}
        vn = MS.vertex_normals(verts, faces, info)
        assert bool(torch.isfinite(vn).all())
        if name == "fan_edges":
            zero = MS.fan_edge_mesh()[2]
            keep = torch.ones(verts.shape[0], dtype=torch.bool)
            keep[zero] = False
            assert bool((vn[zero] == 0).all()) and bool((info["m_vertex"][zero] == 0).all())
            assert bool((info["m_vertex"][keep] > 1e-3).all())
            assert int((info["l"] == 0).sum()) == 1 and bool((info["l"][info["l"] != 0] > 1e-3).all())
            plain = MS.vertex_normals(*MS.fan_mesh())
            assert torch.equal(vn[:8], plain)                                             # nothing else moves
        else:
            assert bool((info["l"] > 1e-3).all()) and bool((info["m_vertex"] > 1e-3).all()), name
    assert MS.normal_meshes()["ico3"][0].shape[0] == 642 and MS.normal_meshes()["ico1"][0].shape[0] == 42


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_pixel_scene_keeps_every_decision_off_a_rounding_edge_and_exercises_both_clamps(H, W):
    s = MS.pixel_scene(H, W)
    info = {}
    MS.shade(s["idx"], s["bary"], s["fz"], s["faces"], s["vn"], s["lights"], H, W, info)
    fg, acc = info["fg"], info["unclamped"]
    assert torch.equal(fg, s["idx"] >= 0) and int(fg.sum()) > 40
    assert bool((info["m_pixel"][fg] > 1e-3).all())
    assert bool(((acc[fg] - MS.LIGHT_MIN).abs() > 1e-4).all()) and bool(((acc[fg] - MS.LIGHT_MAX).abs() > 1e-4).all())
    view0, view1 = fg.clone(), fg.clone()
    view0[H * W:] = False
    view1[:H * W] = False
    assert int((acc[view0] < MS.LIGHT_MIN).sum()) >= 8                                    # default lights: clamped low ...
    assert int(((acc[view0] > MS.LIGHT_MIN) & (acc[view0] < MS.LIGHT_MAX)).sum()) >= 8    # ... and unclamped
    assert int((acc[view0] > MS.LIGHT_MAX).sum()) == 0                                    # (they peak at 0.973)
    assert int((acc[view1] > MS.LIGHT_MAX).sum()) >= 8                                    # twice the default: clamped high


@pytest.mark.parametrize("constant", (False, True))
def test_sphere_scene_keeps_every_decision_off_a_rounding_edge(constant):
    verts, faces, cams, face_uv, tex, lights = MS.sphere_scene(constant)
    S = MS.SPHERE_SIDE
    idx = MS.sphere_winners(verts, faces, cams)
    extra = {}
    MS.shaded_chain(verts, faces, cams, idx, face_uv, tex, lights, S, S, antialias=not constant, extra=extra)
    fg = extra["fg"]
    assert int(fg.sum()) > 100 and bool((extra["l"] > 1e-3).all()) and bool((extra["m_vertex"] > 1e-3).all())
    assert bool((extra["m_pixel"][fg] > 1e-3).all())
    acc = extra["unclamped"][fg]
    assert bool(((acc - MS.LIGHT_MIN).abs() > 1e-4).all()) and bool(((acc - MS.LIGHT_MAX).abs() > 1e-4).all())
    assert bool((extra["bary"][fg] > 1e-4).all())                                         # no winner decided on an edge
    R = tex.shape[-1]
    for c in RG.texel_position(extra["uv"][fg], R):
        assert bool(((c - c.round()).abs() > 1e-3).all())
        assert bool((c > 1e-3).all()) and bool((c < R - 1 - 1e-3).all())
    if not constant:
        for pr in (extra["h"], extra["v"]):
            ev = pr["differ"]
            assert bool((pr["ddepth"][ev] > 1e-4).all())
            t_all = pr["t_all"][pr["cross_all"]]
            assert bool(((t_all - 0).abs() > 1e-3).all()) and bool(((t_all - 1).abs() > 1e-3).all())
            assert bool(((pr["t"][ev & pr["any_ok"]] - 0.5).abs() > 1e-3).all())
        assert bool(extra["h"]["ok"].any()) and bool(extra["v"]["ok"].any())
    assert len(MS.interior_vertices(idx, faces, verts.shape[0])) >= 3


def test_the_reference_gives_the_reason_for_the_feature():
    """Constant texture, no antialiasing: the image alone gives the vertices no gradient, the shaded image does."""
    verts, faces, cams, face_uv, tex, lights = MS.sphere_scene(constant_texture=True)
    idx = MS.sphere_winners(verts, faces, cams)
    S = MS.SPHERE_SIDE
    w1 = MS.sphere_weights(tex.shape[0] + 1)[0]
    v = verts.clone().requires_grad_()
    plain = RG.render_chain(v, faces, cams, idx, face_uv, tex, S, S)   # (its antialiasing moves only the silhouette)
    fxy, fz = RG.prepare(v, faces, cams)
    b = RG.bary(idx, fxy, fz, S, S)
    col = RG.texture_lookup(tex, RG.interpolate(idx, b, face_uv), idx)
    (g,) = torch.autograd.grad((col.reshape(2, S, S, -1) * w1[..., :-1]).sum(), v)
    assert float(g.abs().max()) == 0.0 and plain.shape[-1] == tex.shape[0] + 1
    gv = MS.case_sphere(idx, faces, False, (1, 0, 0))(verts.clone(), cams, face_uv, tex, lights, *MS.sphere_weights(5))[4]
    extra = {}
    MS.shaded_chain(verts, faces, cams, idx, face_uv, tex, lights, S, S, antialias=False, extra=extra)
    lit = (extra["unclamped"] > MS.LIGHT_MIN) & (extra["unclamped"] < MS.LIGHT_MAX)   # (a clamped lighting passes nothing)
    inner = MS.interior_vertices(idx, faces, verts.shape[0], keep=lit)
    assert len(inner) >= 3 and bool((gv[inner].abs().amax(1) > 0).all())


# ------------------------------------------------------------------------------------------------ config and model
def _cfg(**flat):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    base = {"log.exp_name": "t", "guide.shape_path": "shapes/blub.obj"}
    base.update(flat)
    return apply_overrides(TrainConfig(), base)


def test_validate_rules_of_the_shading_options():
    cfg = _cfg().validate()
    assert cfg.render.shading == "albedo" and cfg.render.shading_ratio == 1.0 and cfg.log.eval_maps is False
    assert tuple(cfg.render.lights) == MS.DEFAULT_LIGHTS
    _cfg(**{"render.shading": "lambertian"}).validate()                                   # needs no optim.disp_lr
    _cfg(**{"render.shading": "lambertian", "render.shading_ratio": 0.0}).validate()
    _cfg(**{"render.shading": "textureless", "render.backbone": "texture-rgb-mesh"}).validate()
    assert _cfg(**{"render.lights": "0.5,0,1,1,0,0,0,0,0.25"}).validate().render.lights == (0.5, 0, 1, 1, 0, 0, 0, 0, 0.25)
    with pytest.raises(ValueError, match="grey latent is not defined"):
        _cfg(**{"render.shading": "textureless"}).validate()
    for bad in ({"render.shading": "phong"}, {"render.shading_ratio": -0.1}, {"render.shading_ratio": 1.5},
                {"render.shading_ratio": float("nan")}, {"render.lights": (1.0, 0.0, 1.0)},
                {"render.lights": (1.0,) * 8 + (float("inf"),)}, {"render.lights": (1.0,) * 10},
                {"render.lights": "1,0,1,1,0,0,0,0,x"}):
        with pytest.raises(ValueError):
            _cfg(**bad).validate()


def test_the_model_draws_the_shading_ratio_from_a_generator_of_its_own(tmp_path):
    import numpy as np
    from src.latent_paint.models.textured_mesh import TexturedMeshModel

    obj = MS.write_sphere_obj(tmp_path / "sphere.obj")

    def model(**flat):
        cfg = _cfg(**flat).validate()
        cfg.log.exp_root, cfg.guide.shape_path, cfg.guide.texture_resolution = tmp_path, obj, 8
        return TexturedMeshModel(cfg, render_grid_size=16, texture_resolution=8)

    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    m = model(**{"render.shading": "lambertian", "render.shading_ratio": 0.5, "optim.seed": 7})
    draws = [m._shaded_step() for _ in range(64)]
    assert (np.random.get_state()[1] == before).all()                                     # the global generator is untouched
    rng = np.random.RandomState(7)
    assert draws == [bool(rng.uniform(0, 1) < 0.5) for _ in range(64)] and 8 < sum(draws) < 56
    assert not any(model(**{"render.shading": "lambertian", "render.shading_ratio": 0.0})._shaded_step() for _ in range(64))
    assert all(model(**{"render.shading": "lambertian"})._shaded_step() for _ in range(64))
    plain = model()
    state = plain._shading_rng.get_state()[1].copy()
    assert not plain._shaded_step() and (plain._shading_rng.get_state()[1] == state).all()  # albedo draws nothing
    assert plain.renderer.lights == MS.DEFAULT_LIGHTS
    with pytest.raises(ValueError, match="grey latent"):
        cfg = _cfg(**{"render.shading": "textureless", "render.backbone": "texture-rgb-mesh"}).validate()
        cfg.log.exp_root, cfg.guide.shape_path = tmp_path, obj
        TexturedMeshModel(cfg, render_grid_size=16, texture_resolution=8, latent_mode=True)
