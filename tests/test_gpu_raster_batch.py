"""B views per call on the tile-culled rasteriser (lnerf_raster_prepare_batch / lnerf_rasterize_batch, csrc/raster.hip),
from the kernels up to the Latent-Paint trainer's `render.batch_size`.

Everything the rasteriser gives is compared with torch.equal: against oracle/raster_oracle.rasterize on the synthetic
scenes and against the brute-force kernel lnerf_rasterize on the real meshes.  That equality holds where the brute-force
test accepts no (pixel, face) pair outside the face's box; tests/test_raster_batch_cpu.py checks that condition, on the
CPU, for these scenes and meshes.  The boxes are compared with the numpy restatement of the header's rule
(tests/raster_batch_reference.py)."""
import math

import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO
from tests import raster_batch_reference as R
from tests.test_gpu_raster_ops import ULP, _grid_scene, _pixel_centres, _random_scene, _taps

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _cams(views, dy=0.25):
    from src.latent_paint.models.render import Renderer
    return [Renderer.get_camera_from_view(t, p, r, dy) for t, p, r in views]


def _prepare_batch(dev, verts, faces, cams, H, W):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    B, F_ = len(cams), faces.shape[0]
    cams_dev = torch.tensor([list(c) for c in cams], dtype=torch.float32).to(dev)
    verts_d, faces_d = verts.float().contiguous().to(dev), faces.to(torch.int32).contiguous().to(dev)
    fz = torch.full((B, F_, 3), 7.0, device=dev)
    fxy = torch.full((B, F_, 3, 2), 7.0, device=dev)
    box = torch.full((B, F_, 4), -9, dtype=torch.int16, device=dev)
    _b.call("lnerf_raster_prepare_batch", _p(verts_d), verts.shape[0], _p(faces_d), F_, _p(cams_dev), B, H, W, _p(fz),
            _p(fxy), _p(box), None)
    return verts_d, faces_d, fz, fxy, box


def _rasterize_batch(dev, H, W, fz, fxy, box):
    """fz [B,F,3], fxy [B,F,3,2], box [B,F,4] int16 (any device) -> face_idx [B,H*W] long, bary [B,H*W,3] on the CPU.
    The outputs start as sentinels: a pixel the kernel does not write fails the comparison."""
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    B, F_ = fz.shape[0], fz.shape[1]
    fz, fxy, box = fz.contiguous().to(dev), fxy.contiguous().to(dev), box.contiguous().to(dev)
    assert box.dtype == torch.int16 and box.shape == (B, F_, 4)
    idx = torch.full((B, H * W), -9, dtype=torch.int32, device=dev)
    bary = torch.full((B, H * W, 3), 7.0, device=dev)
    _b.call("lnerf_rasterize_batch", B, H, W, _p(fz), _p(fxy), _p(box), F_, _p(idx), _p(bary), None)
    return idx.cpu().long(), bary.cpu()


def _brute(dev, H, W, fz, fxy):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    fz, fxy = fz.contiguous().to(dev), fxy.contiguous().to(dev)
    idx = torch.full((H * W,), -9, dtype=torch.int32, device=dev)
    bary = torch.full((H * W, 3), 7.0, device=dev)
    _b.call("lnerf_rasterize", H, W, _p(fz), _p(fxy), fz.shape[0], _p(idx), _p(bary), None)
    return idx.cpu().long(), bary.cpu()


def _boxes(H, W, fz, fxy):
    return torch.from_numpy(R.face_boxes(H, W, fz.cpu(), fxy.cpu()))


# ------------------------------------------------------------------------------------------------------ 1. prepare
def test_prepare_batch_equals_single_view_calls_and_the_box_rule(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    g = torch.Generator().manual_seed(3)
    V, F_ = 500, 700
    verts = (torch.rand(V, 3, generator=g) - 0.5).float()
    faces = torch.randint(0, V, (F_, 3), generator=g, dtype=torch.int32)
    # two views from outside, one from inside the cloud: faces behind the camera, across z = 0, and huge coordinates
    views = [(math.radians(65.0), math.radians(40.0), 1.4), (math.radians(100.0), math.radians(250.0), 2.5),
             (math.radians(80.0), math.radians(10.0), 0.2)]
    cams = _cams(views, dy=0.1)
    H, W = 45, 29
    verts_d, faces_d, fz, fxy, box = _prepare_batch(dev, verts, faces, cams, H, W)
    kinds = set()
    for b, cam in enumerate(cams):
        sz = torch.empty(F_, 3, device=dev)
        sxy = torch.empty(F_, 3, 2, device=dev)
        _b.call("lnerf_raster_prepare", _p(verts_d), V, _p(faces_d), F_, cam, _p(sz), _p(sxy), None)
        assert torch.equal(fz[b], sz) and torch.equal(fxy[b], sxy), b
        want = R.face_boxes(H, W, sz.cpu(), sxy.cpu())
        assert torch.equal(box[b].cpu(), torch.from_numpy(want)), b
        empty = (want == np.array(R.EMPTY, dtype=np.int16)).all(1)
        clipped = ~empty & ((want[:, 0] == 0) | (want[:, 1] == W - 1) | (want[:, 2] == 0) | (want[:, 3] == H - 1))
        kinds |= {"empty"} if empty.any() else set()
        kinds |= {"clipped"} if clipped.any() else set()
        kinds |= {"inner"} if (~empty & ~clipped).any() else set()
    assert kinds == {"empty", "clipped", "inner"}


def test_batch_entry_points_refuse_bad_arguments(built_lib):
    import ctypes
    from src.latent_nerf.raymarching import backend as _b
    lib, P = _b.get_lib(), ctypes.c_void_p
    ok = P(4096)
    prep = lambda B=1, H=8, W=8, cams=ok, box=ok: lib.lnerf_raster_prepare_batch(ok, 3, ok, 1, cams, B, H, W, ok, ok, box, None)
    rast = lambda B=1, H=8, W=8, box=ok, F=1: lib.lnerf_rasterize_batch(B, H, W, ok, ok, box, F, ok, ok, None)
    for call in (prep, rast):
        assert call(B=0) == -1 and b"B must be" in lib.lnerf_last_error()
        assert call(H=32768) == -1 and b"32767" in lib.lnerf_last_error()
        assert call(W=32768) == -1 and b"32767" in lib.lnerf_last_error()
        assert call(H=0) == -1
        assert call(box=None) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert prep(cams=None) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert rast(F=0) == -1 and b"no faces" in lib.lnerf_last_error()


# ---------------------------------------------------------------------------------- 2. against the oracle, bit for bit
# The entry point picks one of two kernel shapes from B x (8 x 8 tiles per view): csrc/raster.hip,
# RASTER_SMALL_MAX_TILES.  Every property below is checked on both sides of it.
SMALL_MAX_TILES = 2048


@pytest.mark.parametrize("copies", [1, 20])
def test_rasterize_batch_bit_exact_against_oracle_and_brute_force(dev, copies):
    H, W = 37, 53                                   # multiples of neither 8 nor 16; the grid scene is built for them
    assert (3 * copies * 5 * 7 > SMALL_MAX_TILES) == (copies > 1)
    scenes = [_grid_scene(H, W), _random_scene(300, seed=300), _random_scene(129, seed=129)]
    Fmax = max(s[0].shape[0] for s in scenes)
    fz = torch.full((3, Fmax, 3), 1.0)              # padding: faces behind the camera, culled by their empty box
    fxy = torch.zeros(3, Fmax, 3, 2)
    fxy[:, :, 1, 0] = 0.5
    fxy[:, :, 2, 1] = 0.5
    for b, (z, xy) in enumerate(scenes):
        fz[b, :z.shape[0]], fxy[b, :z.shape[0]] = z, xy
    box = torch.stack([_boxes(H, W, fz[b], fxy[b]) for b in range(3)])
    idx, bary = _rasterize_batch(dev, H, W, fz.repeat(copies, 1, 1), fxy.repeat(copies, 1, 1, 1), box.repeat(copies, 1, 1))
    for c in range(1, copies):                      # view 3c + b shows scene b
        assert torch.equal(idx[3 * c:3 * c + 3], idx[:3]) and torch.equal(bary[3 * c:3 * c + 3], bary[:3]), c
    for b, (z, xy) in enumerate(scenes):
        assert bool((box[b, z.shape[0]:] == torch.tensor(R.EMPTY, dtype=torch.int16)).all())
        ridx, rbary = RO.rasterize(H, W, z, xy)
        assert torch.equal(idx[b], ridx), b
        assert torch.equal(bary[b], rbary), b
        bidx, bbary = _brute(dev, H, W, fz[b], fxy[b])
        assert torch.equal(idx[b], bidx) and torch.equal(bary[b], bbary), b
        hit = ridx >= 0
        assert int(hit.sum()) > H * W // 4 and int((~hit).sum()) > 0
        if b > 0:
            assert int(ridx.max()) == z.shape[0] - 1      # the scene's last face wins pixels


# ------------------------------------------------------------------------------------------------ 3. queue overflow
def _overflow_scene(F_):
    """F_ - 1 triangles that cover the whole image at random constant depths, then one closer triangle over a part of
    it.  For F_ >= 4 two of the full-screen faces, F_ // 2 indices apart, are exact duplicates closer than all the
    other full-screen ones: wherever the last face is not, the lower of the two indices must win."""
    g = torch.Generator().manual_seed(F_)
    full = torch.tensor([[-1.5, -1.5], [4.0, -1.5], [-1.5, 4.0]])
    fxy = full[None].repeat(F_, 1, 1)
    depth = -(1.0 + torch.rand(F_, generator=g))
    lo, hi = None, None
    if F_ >= 4:
        lo, hi = F_ // 6, F_ // 6 + F_ // 2
        depth[lo] = depth[hi] = -0.75
    depth[-1] = -0.5
    fxy[-1] = torch.tensor([[-1.5, -1.5], [0.3, -1.5], [-1.5, 1.2]])
    fz = depth[:, None].repeat(1, 3)
    return fz.contiguous(), fxy.contiguous(), lo, hi


@pytest.mark.parametrize("F_,side,B", [(6000, 16, 1), (1, 16, 1), (63, 16, 1), (65, 16, 1), (1500, 64, 33)])
def test_more_faces_than_the_queue_holds(dev, F_, side, B):
    """6000 faces are more than any LDS queue can hold (160 KiB / 36 B = 4551); the last case runs the 16 x 16 kernel
    (33 views x 64 tiles > SMALL_MAX_TILES), whose queue holds 512."""
    H = W = side
    assert (B * (side // 8) ** 2 > SMALL_MAX_TILES) == (B > 1)
    fz, fxy, lo, hi = _overflow_scene(F_)
    box = _boxes(H, W, fz, fxy)
    assert box[:F_ - 1].tolist() == [[0, W - 1, 0, H - 1]] * (F_ - 1)     # every full-screen face reaches every tile
    idx, bary = _rasterize_batch(dev, H, W, fz[None].repeat(B, 1, 1), fxy[None].repeat(B, 1, 1, 1),
                                 box[None].repeat(B, 1, 1))
    ridx, rbary = RO.rasterize(H, W, fz, fxy)
    assert torch.equal(idx, ridx[None].expand(B, -1)) and torch.equal(bary, rbary[None].expand(B, -1, -1))
    bidx, bbary = _brute(dev, H, W, fz, fxy)
    assert torch.equal(idx[0], bidx) and torch.equal(bary[0], bbary)
    last = int((ridx == F_ - 1).sum())
    assert 0 < last < H * W                                    # the last face is the closest on part of the image
    if lo is not None:
        assert int((ridx == lo).sum()) == H * W - last and int((ridx == hi).sum()) == 0
    else:
        assert int((ridx == -1).sum()) == H * W - last


@pytest.mark.parametrize("B", [SMALL_MAX_TILES // 4, SMALL_MAX_TILES // 4 + 1])
def test_both_kernel_shapes_at_the_threshold(dev, B):
    """A 16 x 16 image is four 8 x 8 tiles: B = 512 views are the last launch of the small shape, B = 513 the first of
    the large one.  Every view shows the same scene and must give the oracle's result."""
    H = W = 16
    fz, fxy = _random_scene(129, seed=129)
    box = _boxes(H, W, fz, fxy)
    idx, bary = _rasterize_batch(dev, H, W, fz[None].repeat(B, 1, 1), fxy[None].repeat(B, 1, 1, 1),
                                 box[None].repeat(B, 1, 1))
    ridx, rbary = RO.rasterize(H, W, fz, fxy)
    assert int((ridx >= 0).sum()) > H * W // 4
    assert torch.equal(idx, ridx[None].expand(B, -1)) and torch.equal(bary, rbary[None].expand(B, -1, -1))


# --------------------------------------------------------------------------------------------------- 4. empty tiles
@pytest.mark.parametrize("copies", [1, 70])
def test_culled_views_and_empty_tiles_are_background(dev, copies):
    H, W = 24, 40
    assert (2 * copies * 3 * 5 > SMALL_MAX_TILES) == (copies > 1)
    px, py = _pixel_centres(H, W)
    dx, dy = 2.0 / W, 2.0 / H
    j, i = 20, 10
    small = torch.tensor([[[float(px[j]) - 0.4 * dx, float(py[i]) + 0.4 * dy],
                           [float(px[j + 1]) + 0.9 * dx, float(py[i]) + 0.4 * dy],
                           [float(px[j]) - 0.4 * dx, float(py[i]) - 0.9 * dy]]])
    small_z = torch.tensor([[-1.0, -1.2, -1.4]])
    # view 0: the one face is behind the camera (an empty box); view 1: it covers two pixels
    fz = torch.stack([small_z.abs(), small_z])
    fxy = torch.stack([small, small])
    box = torch.stack([_boxes(H, W, fz[b], fxy[b]) for b in range(2)])
    assert tuple(box[0, 0].tolist()) == R.EMPTY and box[1, 0].tolist() == [j - 2, j + 3, i - 2, i + 2]
    idx, bary = _rasterize_batch(dev, H, W, fz.repeat(copies, 1, 1), fxy.repeat(copies, 1, 1, 1), box.repeat(copies, 1, 1))
    for c in range(1, copies):
        assert torch.equal(idx[2 * c:2 * c + 2], idx[:2]) and torch.equal(bary[2 * c:2 * c + 2], bary[:2]), c
    assert bool((idx[0] == -1).all()) and bool((bary[0] == 0).all())
    ridx, rbary = RO.rasterize(H, W, fz[1], fxy[1])
    assert (ridx >= 0).nonzero().flatten().tolist() == [i * W + j, i * W + j + 1]
    assert torch.equal(idx[1], ridx) and torch.equal(bary[1], rbary)
    assert bool((bary[1][ridx < 0] == 0).all())


# ------------------------------------------------------------------------------- 5. real meshes against brute force
@pytest.mark.parametrize("shape,B,side", [("blub", 4, 64), ("teddy", 4, 64), ("env_sphere", 2, 64), ("blub", 3, 256)])
def test_real_meshes_equal_the_brute_force_kernel(dev, shape, B, side):
    """(blub at 256 x 256 with 3 views is 3072 tiles: the 16 x 16 kernel.)"""
    H = W = side
    # the painted meshes are normalised; the background sphere (radius 20) is not: the camera sits inside it, most of
    # its faces are behind the camera or project to huge coordinates
    verts, faces = R.load_shape(shape, normalise=shape != "env_sphere")
    cams = _cams(R.training_views(B, seed=23))
    _, _, fz, fxy, box = _prepare_batch(dev, verts, faces, cams, H, W)
    idx, bary = _rasterize_batch(dev, H, W, fz, fxy, box)
    covered = 0
    for b in range(B):
        bidx, bbary = _brute(dev, H, W, fz[b], fxy[b])
        assert torch.equal(idx[b], bidx), (shape, b, int((idx[b] != bidx).sum()))
        assert torch.equal(bary[b], bbary), (shape, b)
        covered += int((bidx >= 0).sum())
    if shape == "env_sphere":
        assert covered == B * H * W                            # inside the sphere every pixel is covered
        assert bool((box.cpu()[..., 1] < box.cpu()[..., 0]).any())
    else:
        assert 0.03 * B * H * W < covered < 0.9 * B * H * W


# ------------------------------------------------------------------------------------------------------ 6. renderer
VIEWS3 = [(math.radians(65.0), math.radians(40.0), 1.4), (math.radians(110.0), math.radians(200.0), 1.2),
          (math.radians(30.0), math.radians(300.0), 1.6)]


def _sphere_mesh():
    from src.latent_paint.models.mesh import Mesh
    from tests.test_gpu_raster import _uv_sphere
    v, vt, f = _uv_sphere()
    return Mesh(vertices=v * 0.6, faces=f, vt=vt, ft=f.clone())


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
def test_render_views_texture_slices_and_texture_gradient(dev, mode):
    from src.latent_paint.models.render import Renderer, _InterpAttr
    mesh = _sphere_mesh()
    H, W, C, Rt = 40, 48, 4, 32
    Rn = Renderer(dev, dim=(W, H), interpolation_mode=mode)
    uv_attr = mesh.vt[mesh.ft][None].to(dev)
    g = torch.Generator().manual_seed(9)
    tex = torch.randn(1, C, Rt, Rt, generator=g).to(dev)
    el, az, ra = [v[0] for v in VIEWS3], [v[1] for v in VIEWS3], [v[2] for v in VIEWS3]
    dy = 0.1
    up = torch.randint(-3, 4, (3, C, H, W), generator=g).float().to(dev)      # integer upstream gradients
    tb = tex.clone().requires_grad_()
    img, mask = Rn.render_views_texture(mesh.vertices, mesh.faces, uv_attr, tb, el, az, ra, dy)
    assert img.shape == (3, C, H, W) and mask.shape == (3, 1, H, W)
    img.backward(up)
    single_sum = torch.zeros_like(tex)
    for b in range(3):
        ts = tex.clone().requires_grad_()
        simg, smask = Rn.render_single_view_texture(mesh.vertices, mesh.faces, uv_attr, ts, el[b], az[b], ra[b], dy)
        assert torch.equal(img[b:b + 1], simg) and torch.equal(mask[b:b + 1], smask), b
        assert 0.05 < float(smask.mean()) < 0.95
        simg.backward(up[b:b + 1])
        single_sum += ts.grad
    wimg, _ = Rn.render_views_texture(mesh.vertices, mesh.faces, uv_attr, tex, el, az, ra, dy, white_background=True)
    assert torch.equal(wimg, img.detach() + (1 - mask))
    if mode == "nearest":          # integer addends: their sum is exact in any atomic order
        assert torch.equal(tb.grad, single_sum)
        return
    if mode == "bilinear":         # (n + 4) ulp of each texel's absolute sum, n = its number of addends
        face_idx, bary, _, _, _ = Rn._rasterize_views(mesh.vertices, mesh.faces, el, az, ra, dy, (W, H))
        uv = _InterpAttr.apply(uv_attr[0], face_idx, bary).cpu()
        fg = (face_idx >= 0).cpu()
        idx, w = _taps(uv, Rt, "bilinear")
        dout = up.permute(0, 2, 3, 1).reshape(-1, C).cpu().double()           # [P,C], P = B*H*W
        gw = w[None] * dout.T[:, :, None]                                      # [C,P,4]
        keep = fg[None, :, None].expand_as(gw)
        gw = torch.where(keep, gw, torch.zeros(()).double())
        ix = idx[None].expand(C, -1, -1).reshape(C, -1)
        dref = torch.zeros(C, Rt * Rt, dtype=torch.float64).scatter_add_(1, ix, gw.reshape(C, -1))
        s = torch.zeros(C, Rt * Rt, dtype=torch.float64).scatter_add_(1, ix, gw.abs().reshape(C, -1))
        n = torch.zeros(C, Rt * Rt, dtype=torch.float64).scatter_add_(1, ix, keep.double().reshape(C, -1))
        err = (tb.grad.cpu().double().reshape(C, Rt * Rt) - dref).abs()
        assert bool((err <= (n + 4) * ULP * s).all()), float((err / ((n + 4) * ULP * s + 1e-300)).max())
        assert float(s.sum()) > 0


def test_render_views_slices_and_sky_gradient_mass(dev):
    from src.latent_nerf.training.shape import make_icosphere
    from src.latent_paint.models.mesh import Mesh
    from src.latent_paint.models.render import Renderer
    H, W, C, B = 40, 48, 4, 3
    Rn = Renderer(dev, dim=(W, H))
    ev, ef = make_icosphere(3, 20.0)
    env = Mesh(vertices=ev, faces=ef)
    cols = torch.rand(1, ef.shape[0], 3, C, device=dev, requires_grad=True)
    el, az, ra = [v[0] for v in VIEWS3], [v[1] for v in VIEWS3], [v[2] for v in VIEWS3]
    back, bmask = Rn.render_views(env, cols, el, az, ra, 0.1)
    assert back.shape == (B, C, H, W) and float(bmask.min()) == 1.0      # the camera is inside the sphere
    for b in range(B):
        sb, sm = Rn.render_single_view(env, cols, el[b], az[b], ra[b], 0.1)
        assert torch.equal(back[b:b + 1], sb) and torch.equal(bmask[b:b + 1], sm), b
    back.sum().backward()
    assert abs(float(cols.grad.sum()) - C * B * H * W) < 1e-2 * C * B * H * W
    with pytest.raises(ValueError, match="one length"):
        Rn.render_views(env, cols, el, az[:2], ra, 0.1)


# --------------------------------------------------------------------------------------------- 7. model and trainer
def _paint_cfg(tmp_path, **over):
    import os
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "paint", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(R.SHAPES, "blub.obj"), "guide.texture_resolution": 64}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def test_model_render_takes_sequences(dev, tmp_path):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    cfg = _paint_cfg(tmp_path)
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=64)
    thetas, phis, radii = [v[0] for v in VIEWS3], [v[1] for v in VIEWS3], [v[2] for v in VIEWS3]
    with torch.no_grad():
        out = model.render(thetas, phis, radii)
        assert out["image"].shape == (3, 4, 64, 64) and out["mask"].shape == (3, 1, 64, 64)
        for b in range(3):
            one = model.render(thetas[b], phis[b], radii[b])
            for key in ("image", "mask", "background", "foreground"):
                assert torch.equal(out[key][b:b + 1], one[key]), (key, b)
        test = model.render(thetas, phis, radii, decode_func=lambda t: t[:, :3].sigmoid(), test=True, dims=(48, 48))
        assert test["image"].shape == (3, 3, 48, 48)
        with pytest.raises(ValueError, match="all scalars or all sequences"):
            model.render(thetas, 0.5, radii)


def test_trainer_steps_on_two_views_at_a_time(dev, tmp_path):
    from src.latent_paint.training.trainer import Trainer
    over = {"optim.iters": 3, "log.save_interval": 3, "log.eval_size": 1, "log.full_eval_size": 1,
            "render.eval_grid_size": 64, "render.batch_size": 2, "log.save_mesh": False}
    tr = Trainer(_paint_cfg(tmp_path, **over), device=dev)
    tex0 = tr.mesh_model.texture_img.detach().clone()
    seen = []
    render = tr.mesh_model.render

    def counting(theta, phi, radius, **kw):
        if not kw.get("test"):
            seen.append(len(theta))
        return render(theta, phi, radius, **kw)
    tr.mesh_model.render = counting
    tr.train()
    assert tr.train_step == 3 and seen == [2, 2, 2]                       # six views in three steps
    assert (tr.ckpt_path / "step_000003.pth").exists()
    assert float((tr.mesh_model.texture_img.detach() - tex0).abs().max()) > 1e-3


class _OnesGuidance:
    """d(loss)/d(pred) = +1 everywhere; takes one text embedding per call, like the diffusion adapter."""

    def __init__(self):
        self.calls = []

    def get_text_embeds(self, prompt):
        return prompt

    def train_step(self, text_z, latents, dirs=None):
        self.calls.append((text_z, latents.shape[0]))
        return torch.ones_like(latents)


def test_batched_step_gradient_is_the_mean_of_the_single_view_gradients(dev, tmp_path):
    from src.latent_paint.training.trainer import DIRECTION_WORDS, Trainer
    guide = _OnesGuidance()
    tr = Trainer(_paint_cfg(tmp_path, **{"render.batch_size": 2, "optim.lr": 0.0}), device=dev, guidance=guide)
    model = tr.mesh_model
    assert model.renderer.interpolation_mode == "nearest"
    data = tr.dataloaders["train"]._data.collate([0, 1])
    assert len(data["theta"]) == 2
    for p in model.get_params():
        p.grad = None
    pred, grad = tr.train_render(data)
    assert pred.shape[0] == 2 and bool((grad == 0.5).all())
    # one guidance call per direction present, each with that direction's prompt
    dirs = [int(d) for d in data["dir"]]
    assert sorted(n for _, n in guide.calls) == sorted(dirs.count(d) for d in set(dirs))
    assert all(z == "a goldfish, %s view" % DIRECTION_WORDS[d] for (z, _), d in zip(guide.calls, sorted(set(dirs))))
    batch = model.texture_img.grad.clone()
    total = torch.zeros_like(batch)
    for b in range(2):
        model.texture_img.grad = None
        out = model.render(data["theta"][b], data["phi"][b], data["radius"][b])
        out["image"].backward(gradient=torch.ones_like(out["image"]))
        total += model.texture_img.grad
    assert float(total.abs().sum()) > 0
    assert torch.equal(batch, total / 2)          # pixel counts and halves of them: exact in any order
