"""The vertex-gradient kernels of csrc/rastergrad.hip against the float64 reference of tests/rastergrad_reference.py.

The reference takes the GPU's own face_idx, so the discrete winners are shared; tests/test_rastergrad_cpu.py asserts that
no other decision of these scenes sits on a rounding edge.  Tolerances: for every compared tensor the same reference was run
in float32 on the CPU on these very inputs, and 4 x its largest deviation from float64 (relative to the tensor's largest
magnitude) is allowed -- REL below, printed by

    python -m tests.rastergrad_reference

The antialias forward has a derived bound instead, 16 eps max(H, W) max|image| (t is a difference divided by a pixel
pitch)."""
import ctypes

import pytest
import torch

from tests import rastergrad_reference as RG

pytestmark = pytest.mark.gpu

REL = {
    'antialias_16x16': (1.47e-07, 1.66e-07),
    'bary_16x16': (1.76e-07, 9.15e-08),
    'interp_D2_16x16': (7.18e-08,),
    'interp_D5_16x16': (8.64e-08,),
    'chain_16x16': (9.04e-06, 3.68e-06),
    'antialias_13x11': (4.25e-06, 2.39e-06),
    'bary_13x11': (3.16e-07, 1.05e-07),
    'interp_D2_13x11': (5.93e-08,),
    'interp_D5_13x11': (6.38e-08,),
    'chain_13x11': (3.21e-06, 1.57e-06),
    'texture_R4': (8.17e-08,),
    'texture_R8': (1.35e-07,),
    'prepare': (6.95e-08,),
    'umbrella_fan': (3.59e-08, 1.72e-08),
    'umbrella_tetra': (5.94e-08, 5.94e-08),
}
EPS = 2.0 ** -23
ERR_INVALID_ARG = -1          # LNERF_ERR_INVALID_ARG (include/lnerf_hip.h)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _d(t, dev, dtype=torch.float32):
    """A contiguous device copy the caller keeps alive across the launch."""
    return t.to(dtype).contiguous().to(dev)


def _lib():
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    return _b, _p


def _close(name, got, want, rel):
    """|got - want| <= tolerance(rel, max|want|); prints the figure first."""
    mag = float(want.abs().max())
    err = float((got.double().cpu() - want).abs().max())
    tol = RG.tolerance(rel, mag)
    print("%s: max error %.3g, allowed %.3g (magnitude %.3g)" % (name, err, tol, mag))
    assert mag > 0 and err <= tol, (name, err, tol)


def _rasterize(dev, fxy, fz, H, W):
    """The GPU's winners and weights for projected faces given directly (whole-image boxes)."""
    _b, _p = _lib()
    B, F = fz.shape[0], fz.shape[1]
    fxy_d, fz_d = fxy.float().contiguous().to(dev), fz.float().contiguous().to(dev)
    box = torch.tensor([0, W - 1, 0, H - 1], dtype=torch.int16).repeat(B, F, 1).contiguous().to(dev)
    idx = torch.full((B * H * W,), -9, dtype=torch.int32, device=dev)
    bary = torch.full((B * H * W, 3), 7.0, device=dev)
    _b.call("lnerf_rasterize_batch", B, H, W, _p(fz_d), _p(fxy_d), _p(box), F, _p(idx), _p(bary), None)
    return fxy_d, fz_d, idx, bary


@pytest.fixture(scope="module", params=RG.SIZES, ids=lambda s: "%dx%d" % s)
def scene(request, dev):
    """The base scene at one size, rasterised once on the GPU, with the reference's antialias results."""
    H, W = request.param
    fxy, fz, faces = RG.screen_scene()
    fxy_d, fz_d, idx_d, bary_d = _rasterize(dev, fxy, fz, H, W)
    idx = idx_d.cpu().long()
    assert torch.equal(idx, RG.oracle_face_idx(fxy, fz, H, W))          # the winners the CPU preconditions were checked on
    img, gout = RG.scene_image(2, H, W), RG.randn((2, H, W, RG.C_IMAGE), 21)
    ref = RG.case_antialias(idx, faces, H, W)(img.clone(), gout, fxy.clone(), fz)
    return dict(H=H, W=W, fxy=fxy, fz=fz, faces=faces, idx=idx, fxy_d=fxy_d, fz_d=fz_d, idx_d=idx_d, bary_d=bary_d,
                faces_d=faces.to(torch.int32).contiguous().to(dev), img=img, gout=gout, ref=ref,
                key="%dx%d" % (H, W))


def _aa_forward(s, dev, img):
    _b, _p = _lib()
    B, H, W, C = img.shape
    img_d = img.float().contiguous().to(dev)
    out = torch.full_like(img_d, 7.0)
    _b.call("lnerf_raster_antialias_forward", _p(img_d), _p(s["idx_d"]), _p(s["bary_d"]), _p(s["fxy_d"]), _p(s["fz_d"]),
            _p(s["faces_d"]), B, H, W, C, s["faces"].shape[0], _p(out), None)
    return out


def test_antialias_forward_matches_the_reference_bit_identically_on_every_run(scene, dev):
    s = scene
    out = _aa_forward(s, dev, s["img"])
    want = s["ref"][0]
    bound = 16 * EPS * max(s["H"], s["W"]) * float(s["img"].abs().max())
    err = float((out.double().cpu() - want).abs().max())
    print("antialias forward %s: max error %.3g, bound %.3g" % (s["key"], err, bound))
    assert err <= bound
    assert float((want - s["img"]).abs().max()) > 0.1                    # the pass did something
    assert torch.equal(_aa_forward(s, dev, s["img"]), out)
    const = torch.full((2, s["H"], s["W"], 3), 0.375, dtype=torch.float64)
    assert torch.equal(_aa_forward(s, dev, const).cpu(), const.float())


def test_antialias_backward_matches_the_reference(scene, dev):
    _b, _p = _lib()
    s = scene
    B, H, W, C = s["img"].shape
    F = s["faces"].shape[0]
    img_d, gout_d = s["img"].float().contiguous().to(dev), s["gout"].float().contiguous().to(dev)
    gimg = torch.full_like(img_d, 7.0)
    gxy = torch.zeros(B, F, 3, 2, device=dev)
    _b.call("lnerf_raster_antialias_backward", _p(gout_d), _p(img_d), _p(s["idx_d"]), _p(s["bary_d"]), _p(s["fxy_d"]),
            _p(s["fz_d"]), _p(s["faces_d"]), B, H, W, C, F, _p(gimg), _p(gxy), None)
    rel = REL["antialias_" + s["key"]]
    _close("antialias grad_image " + s["key"], gimg, s["ref"][1], rel[0])
    _close("antialias grad_face_xy " + s["key"], gxy, s["ref"][2], rel[1])
    assert float(s["ref"][2][:, 8:].abs().max()) == 0 and float(gxy[:, 8:].abs().max()) == 0   # rejected faces: nothing
    # it ADDS INTO grad_face_xy
    gxy2 = torch.ones(B, F, 3, 2, device=dev)
    _b.call("lnerf_raster_antialias_backward", _p(gout_d), _p(img_d), _p(s["idx_d"]), _p(s["bary_d"]), _p(s["fxy_d"]),
            _p(s["fz_d"]), _p(s["faces_d"]), B, H, W, C, F, _p(gimg), _p(gxy2), None)
    assert bool((gxy2[:, 8:] == 1).all()) and bool(((gxy2 != 1) == (gxy != 0)).all())


def test_bary_backward_matches_the_reference(scene, dev):
    _b, _p = _lib()
    s = scene
    B, H, W, F = 2, s["H"], s["W"], s["faces"].shape[0]
    gb = RG.randn((B * H * W, 3), 22)
    want = RG.case_bary(s["idx"], H, W)(gb, s["fxy"].clone(), s["fz"].clone())
    gxy, gz = torch.zeros(B, F, 3, 2, device=dev), torch.zeros(B, F, 3, device=dev)
    gb_d = _d(gb, dev)
    _b.call("lnerf_raster_bary_backward", _p(gb_d), _p(s["idx_d"]), _p(s["fxy_d"]),
            _p(s["fz_d"]), B, H, W, F, _p(gxy), _p(gz), None)
    rel = REL["bary_" + s["key"]]
    _close("bary grad_face_xy " + s["key"], gxy, want[0], rel[0])
    _close("bary grad_face_z " + s["key"], gz, want[1], rel[1])


@pytest.mark.parametrize("D", (2, 5))
def test_interpolation_bary_gradient_matches_the_reference(scene, dev, D):
    _b, _p = _lib()
    s = scene
    P, F = s["idx"].shape[0], s["faces"].shape[0]
    attr, dfeat = RG.randn((F, 3, D), 23), RG.randn((P, D), 24)
    (want,) = RG.case_interp(s["idx"])(RG.bary(s["idx"], s["fxy"], s["fz"], s["H"], s["W"]), attr, dfeat)
    got = torch.full((P, 3), 7.0, device=dev)
    attr_d, dfeat_d = _d(attr, dev), _d(dfeat, dev)
    _b.call("lnerf_interpolate_attributes_backward_bary", _p(s["idx_d"]), _p(attr_d), _p(dfeat_d), P, D, F, _p(got), None)
    _close("interp grad_bary D=%d %s" % (D, s["key"]), got, want, REL["interp_D%d_%s" % (D, s["key"])][0])
    assert bool((got[s["idx_d"] < 0] == 0).all())


@pytest.mark.parametrize("R", (4, 8))
def test_lookup_uv_gradient_matches_the_reference_and_is_zero_under_a_clamp(dev, R):
    _b, _p = _lib()
    uv, idx = RG.uv_scene(R)
    tex, dout = RG.randn((3, R, R), 26), RG.randn((uv.shape[0], 3), 27)
    (want,) = RG.case_texture(idx)(tex, uv.clone(), dout)
    got = torch.full((uv.shape[0], 2), 7.0, device=dev)
    uv_d, idx_d, tex_d, dout_d = _d(uv, dev), _d(idx, dev, torch.int32), _d(tex, dev), _d(dout, dev)
    _b.call("lnerf_texture_map_backward_uv", _p(uv_d), _p(idx_d), _p(tex_d), _p(dout_d), uv.shape[0], 3, R, _p(got), None)
    _close("texture grad_uv R=%d" % R, got, want, REL["texture_R%d" % R][0])
    got = got.cpu()
    assert bool((got[(uv < 0) | (uv > 1)] == 0).all()) and float(got[5, 0]) == 0.0 and bool((got[-8:] == 0).all())
    assert bool((got[6:-8] != 0).all())


def test_prepare_backward_sums_views_and_corners(dev):
    _b, _p = _lib()
    verts, cams = RG.prepare_scene()
    faces = RG.PREPARE_FACES
    gxy, gz = RG.randn((3, 5, 3, 2), 28), RG.randn((3, 5, 3), 29)
    (want,) = RG.case_prepare(faces)(verts.clone(), cams, gxy, gz)
    got = torch.full((7, 3), 7.0, device=dev)                            # overwritten, the unused vertex included
    gxy_d, gz_d, verts_d, faces_d, cams_d = (_d(gxy, dev), _d(gz, dev), _d(verts, dev), _d(faces, dev, torch.int32),
                                             _d(cams, dev))
    _b.call("lnerf_raster_prepare_batch_backward", _p(gxy_d), _p(gz_d), _p(verts_d), 7, _p(faces_d), 5, _p(cams_d), 3,
            _p(got), None)
    _close("prepare grad_verts", got, want, REL["prepare"][0])
    assert float(got[6].abs().max()) == 0.0


@pytest.mark.parametrize("name,faces,V", (("fan", RG.FAN_FACES, 6), ("tetra", RG.TETRA_FACES, 4)))
def test_umbrella_and_its_transpose(dev, name, faces, V):
    from src.latent_paint.models.render import _umbrella
    x = RG.randn((V, 3), 30 if name == "fan" else 31)
    want = RG.case_umbrella(faces)(x)
    f32 = faces.to(torch.int32).contiguous().to(dev)
    xd = x.float().to(dev)
    _close("umbrella L " + name, _umbrella(xd, f32, False), want[0], REL["umbrella_" + name][0])
    _close("umbrella L^T " + name, _umbrella(xd, f32, True), want[1], REL["umbrella_" + name][1])
    if name == "fan":
        assert torch.equal(_umbrella(xd, f32, False)[5], xd[5]) and torch.equal(_umbrella(xd, f32, True)[5], xd[5])


# ------------------------------------------------------------------------------------------------ the whole chain
def _chain(dev, H, W):
    """vertices -> antialiased [B,H,W,C+1] through the Renderer's autograd nodes -> (image, grad_verts, reference)."""
    from src.latent_paint.models.render import Renderer
    verts, faces, cams, face_uv, tex = RG.chain_scene()
    r = Renderer(dev, dim=(W, H), interpolation_mode="bilinear", antialias=True)
    views = RG.CHAIN_VIEWS
    vd = verts.float().to(dev).requires_grad_()
    elev, azim, rad = zip(*views)
    img, mask, state = r.render_views_texture(vd, faces.to(dev), face_uv.float().to(dev)[None], tex.float().to(dev)[None],
                                              elev, azim, rad, look_at_height=0.0, return_state=True)
    out = r.antialias_views(torch.cat([img, mask], 1), state, faces.to(dev)).permute(0, 2, 3, 1)
    gout = RG.randn((2, H, W, tex.shape[0] + 1), 25)
    (gv,) = torch.autograd.grad((out * gout.float().to(dev)).sum(), vd)
    idx = state[0].cpu().long()
    fxy, fz = RG.prepare(verts, faces, cams)
    assert torch.equal(idx, RG.oracle_face_idx(fxy, fz, H, W))
    want = RG.case_chain(idx, faces, H, W)(verts.clone(), cams, face_uv, tex, gout)
    return out.detach(), gv, want


@pytest.fixture(scope="module", params=RG.SIZES, ids=lambda s: "%dx%d" % s)
def chain(request, dev):
    H, W = request.param
    return ("%dx%d" % (H, W),) + _chain(dev, H, W)


def test_whole_chain_vertices_to_antialiased_image(chain):
    key, out, gv, want = chain
    _close("chain image " + key, out, want[0], REL["chain_" + key][0])
    _close("chain grad_verts " + key, gv, want[1], REL["chain_" + key][1])
    assert bool((want[1].abs().amax(1) > 0).all())                       # every vertex of the scene receives gradient


def test_the_chain_comparison_bites_on_one_vertex(chain):
    """Zeroing the gradient of a single vertex must fail the comparison above."""
    key, out, gv, want = chain
    broken = gv.clone()
    broken[4] = 0
    with pytest.raises(AssertionError):
        _close("chain grad_verts, vertex 4 zeroed " + key, broken, want[1], REL["chain_" + key][1])


def test_geometry_gradients_need_the_bilinear_lookup(dev):
    from src.latent_paint.models.render import Renderer
    verts, faces, cams, face_uv, tex = RG.chain_scene()
    for mode in ("nearest", "bicubic", "mipmap"):
        r = Renderer(dev, dim=(16, 16), interpolation_mode=mode)
        with pytest.raises(ValueError, match="bilinear"):
            r.render_views_texture(verts.float().to(dev).requires_grad_(), faces.to(dev), face_uv.float().to(dev)[None],
                                   tex.float().to(dev)[None], [1.4], [0.2], [2.0])


# ------------------------------------------------------------------------------------------------ argument checks
def test_every_entry_point_refuses_bad_arguments(dev):
    _b, _p = _lib()
    lib = _b.get_lib()
    t = torch.zeros(4096, device=dev)
    i = torch.zeros(4096, device=dev, dtype=torch.int32)
    P, I = _p(t), _p(i)

    def refused(name, *args):
        assert getattr(lib, name)(*args) == ERR_INVALID_ARG, name
        msg = lib.lnerf_last_error().decode()
        assert name[len("lnerf_"):] in msg, (name, msg)

    refused("lnerf_raster_antialias_forward", P, I, P, P, P, I, 0, 4, 4, 3, 2, P, None)
    refused("lnerf_raster_antialias_forward", P, I, P, P, P, I, 1, 4, 4, 0, 2, P, None)
    refused("lnerf_raster_antialias_forward", P, I, P, P, P, I, 1, 4, 4, 3, 0, P, None)
    refused("lnerf_raster_antialias_forward", P, None, P, P, P, I, 1, 4, 4, 3, 2, P, None)
    refused("lnerf_raster_antialias_forward", P, I, P, P, P, I, 1, 4, 4, 3, 2, P, None)          # out is image
    refused("lnerf_raster_antialias_backward", P, P, I, P, P, P, I, 1, 4, 40000, 3, 2, P, P, None)
    refused("lnerf_raster_antialias_backward", P, P, I, P, P, P, I, 1, 4, 4, 3, 2, None, P, None)
    refused("lnerf_raster_antialias_backward", P, P, I, P, P, P, I, 1, 4, 4, 3, 2, P, P, None)   # grad_image is grad_out
    refused("lnerf_raster_bary_backward", P, I, P, P, 1, 0, 4, 2, P, P, None)
    refused("lnerf_raster_bary_backward", P, I, P, P, 1, 4, 4, 2, P, None, None)
    refused("lnerf_interpolate_attributes_backward_bary", I, P, P, 16, 17, 2, P, None)
    refused("lnerf_interpolate_attributes_backward_bary", I, P, P, 0, 2, 2, P, None)
    refused("lnerf_interpolate_attributes_backward_bary", I, None, P, 16, 2, 2, P, None)
    refused("lnerf_texture_map_backward_uv", P, I, P, P, 16, 0, 4, P, None)
    refused("lnerf_texture_map_backward_uv", P, I, P, P, 16, 3, 0, P, None)
    refused("lnerf_texture_map_backward_uv", P, I, None, P, 16, 3, 4, P, None)
    refused("lnerf_raster_prepare_batch_backward", P, P, P, 0, I, 2, P, 1, P, None)
    refused("lnerf_raster_prepare_batch_backward", P, P, P, 4, I, 2, P, 0, P, None)
    refused("lnerf_raster_prepare_batch_backward", P, P, P, 4, I, 2, None, 1, P, None)
    assert lib.lnerf_mesh_umbrella_scratch_bytes(0, 2) == 0 and lib.lnerf_mesh_umbrella_scratch_bytes(5, -1) == 0
    assert lib.lnerf_mesh_umbrella_scratch_bytes(5, 2) == 32 + 64
    o = torch.zeros(64, device=dev)
    refused("lnerf_mesh_umbrella", P, 5, I, 2, 2, P, ctypes.c_size_t(96), _p(o), None)           # transpose flag
    refused("lnerf_mesh_umbrella", P, 5, I, 2, 0, P, ctypes.c_size_t(16), _p(o), None)           # scratch too small
    refused("lnerf_mesh_umbrella", P, 5, I, 2, 0, P, ctypes.c_size_t(96), P, None)               # out is x
    refused("lnerf_mesh_umbrella", P, 0, I, 2, 0, P, ctypes.c_size_t(96), _p(o), None)
    assert float(t.abs().max()) == 0 and float(o.abs().max()) == 0                                # nothing was launched
