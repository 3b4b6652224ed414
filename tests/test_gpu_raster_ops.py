"""The Latent-Paint raster ops of csrc/raster.hip, one at a time, against plain references:

* lnerf_rasterize: bit-exact against oracle/raster_oracle.rasterize (which follows the kernel's f32 arithmetic) on
  synthetic scenes built for the hard cases -- shared edges and vertices on pixel centres, depth ties, faces behind
  the camera or across z = 0, zero-area faces, both windings, several 128-face LDS tiles, H != W.
* lnerf_raster_prepare: against float64.  The kernel rounds v - pos (1 ulp), forms each camera coordinate with two
  fmaf and a product (<= 2 ulp of S = sum |rot_i| |v_i - pos_i|), then x * f / (-z) (2 more roundings).  So
  |z - z64| <= 4 ulp(S) and |xy - xy64| <= 4 ulp * (f S + |xy| S) / |z| + 2 ulp(|xy|): PREPARE_ULPS = 8 covers it.
* interpolate_attributes forward / backward and texture_map forward / backward (nearest, bilinear, bicubic):
  against float64.  The texel coordinate is restated in f32 (the same bits as the kernel's tex_coords), the
  interpolation in float64.  Forward sums of k terms are within k + 2 ulp of their absolute sum; the backward
  (float atomics in any order) within (n + 4) ulp of each element's absolute sum, n = its number of addends.
  Nearest lookups are exact.  The bicubic weights are cubics whose intermediate terms reach 6, so each 1-D weight is
  within 32 ulp (absolute) and each 2-D weight within BICUBIC_W_ULPS = 128 ulp of its float64 value: that adds
  128 ulp of the absolute sum of the taps' texels (forward) or upstream gradients (backward)."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import raster_oracle as RO

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
PREPARE_ULPS = 8
BICUBIC_W_ULPS = 128


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _rasterize(dev, H, W, face_z, face_xy):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    F_ = face_z.shape[0]
    fz, fxy = face_z.contiguous().to(dev), face_xy.contiguous().to(dev)
    idx = torch.full((H * W,), -9, dtype=torch.int32, device=dev)
    bary = torch.full((H * W, 3), 7.0, device=dev)
    _b.call("lnerf_rasterize", H, W, _p(fz), _p(fxy), F_, _p(idx), _p(bary), None)
    return idx.cpu().long(), bary.cpu()


def _pixel_centres(H, W):
    """The kernel's pixel centres in NDC, with its f32 arithmetic."""
    j = torch.arange(W, dtype=torch.float32)
    i = torch.arange(H, dtype=torch.float32)
    return (2 * j + 1) / W - 1, 1 - (2 * i + 1) / H


def _grid_scene(H, W, step=4):
    """A quad grid with every vertex on a pixel centre, each quad split into two triangles (shared edges through
    pixel centres).  Then: a duplicate of the first 10 faces at the same depth (coplanar tie, the originals have
    the lower index), the same faces with the other winding, a zero-area face, faces behind the camera and across
    z = 0."""
    px, py = _pixel_centres(H, W)
    xs, ys = px[::step], py[::step]
    g = torch.Generator().manual_seed(1)
    depth = -(1.0 + torch.rand(len(ys), len(xs), generator=g))
    faces_xy, faces_z = [], []
    for a in range(len(ys) - 1):
        for b in range(len(xs) - 1):
            v = [(xs[b], ys[a], depth[a, b]), (xs[b + 1], ys[a], depth[a, b + 1]),
                 (xs[b], ys[a + 1], depth[a + 1, b]), (xs[b + 1], ys[a + 1], depth[a + 1, b + 1])]
            for tri in ((0, 2, 1), (1, 2, 3)):
                faces_xy.append([[v[k][0], v[k][1]] for k in tri])
                faces_z.append([v[k][2] for k in tri])
    fxy = torch.tensor(faces_xy, dtype=torch.float32)
    fz = torch.tensor(faces_z, dtype=torch.float32)
    extra_xy = [fxy[:10], fxy[:10].flip(1), fxy[:1].clone()]
    extra_z = [fz[:10], fz[:10].flip(1), fz[:1].clone()]
    extra_xy[2][0, 2] = extra_xy[2][0, 0]                      # degenerate: two equal vertices
    back = fxy[10:20].clone(), fz[10:20].abs() + 0.5           # behind the camera (z > 0), would win on depth
    cross = fxy[20:30].clone(), fz[20:30].clone()
    cross[1][:, 1] = 0.5                                       # crosses z = 0
    fxy = torch.cat([fxy] + extra_xy + [back[0], cross[0]])
    fz = torch.cat([fz] + extra_z + [back[1], cross[1]])
    return fz.contiguous(), fxy.contiguous()


def _random_scene(F_, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(F_, 1, 2, generator=g) - 0.5) * 2.4
    fxy = c + (torch.rand(F_, 3, 2, generator=g) - 0.5) * 0.9
    fz = -(0.5 + 4.0 * torch.rand(F_, 3, generator=g))
    fz[::17, 0] = -fz[::17, 0]                                  # some faces cross z = 0
    fz[5:300:40] = fz[4:300:40]                                 # equal depths ...
    fxy[5:300:40] = fxy[4:300:40].flip(1)                       # ... on the same triangle, the other winding
    fxy[7:300:50, 2] = 0.5 * (fxy[7:300:50, 0] + fxy[7:300:50, 1])   # collinear: zero area (to rounding)
    fxy[-1] = torch.tensor([[-0.6, -0.5], [0.7, -0.4], [0.1, 0.6]])   # the closest face is the last of a partial tile
    fz[-1] = torch.tensor([-0.3, -0.4, -0.35])
    return fz.contiguous(), fxy.contiguous()


@pytest.mark.parametrize("scene", ["grid", "random300", "random129"])
def test_rasterize_bit_exact(dev, scene):
    if scene == "grid":
        H, W = 37, 53           # H != W, H*W = 1961: a partial last workgroup
        fz, fxy = _grid_scene(H, W)
    else:
        H, W = 45, 29
        fz, fxy = _random_scene(int(scene[6:]), seed=int(scene[6:]))
    assert (H * W) % 256 != 0
    idx, bary = _rasterize(dev, H, W, fz, fxy)
    ridx, rbary = RO.rasterize(H, W, fz, fxy)
    assert torch.equal(idx, ridx)
    assert torch.equal(bary, rbary)
    hit = ridx >= 0
    assert int(hit.sum()) > H * W // 4 and int((~hit).sum()) > 0
    if scene == "grid":
        n_grid = fz.shape[0] - 41
        late = ridx - n_grid       # exact duplicates lose the tie; zero-area, back and crossing faces never win
        assert not bool(((late >= 0) & (late < 10)).any()) and not bool((late >= 20).any())
        assert bool((rbary[hit] == 0).any(1).any())              # pixels on edges: a zero weight is inside
    else:
        assert int(ridx.max()) == fz.shape[0] - 1                # the tail face of the last LDS tile wins pixels
        assert int(((ridx >= 128) & (ridx < 256)).sum()) > 0 or fz.shape[0] <= 256


def test_raster_prepare_within_a_few_ulp(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    from src.latent_paint.models.render import Renderer
    g = torch.Generator().manual_seed(3)
    V, F_ = 500, 700
    verts = (torch.rand(V, 3, generator=g) - 0.5).float()
    faces = torch.randint(0, V, (F_, 3), generator=g, dtype=torch.int32)
    verts_d, faces_d = verts.to(dev), faces.to(dev)
    for elev, azim, r, h in ((65.0, 40.0, 1.4, 0.1), (100.0, 250.0, 2.5, -0.2)):
        cam = Renderer.get_camera_from_view(math.radians(elev), math.radians(azim), r, h)
        fz = torch.empty(F_, 3, device=dev)
        fxy = torch.empty(F_, 3, 2, device=dev)
        _b.call("lnerf_raster_prepare", _p(verts_d), V, _p(faces_d), F_, cam, _p(fz), _p(fxy), None)
        c = torch.tensor(list(cam), dtype=torch.float32).double()
        rot, pos, f = c[:9].reshape(3, 3), c[9:12], c[12:14]
        d = verts.double()[faces.long()] - pos                   # [F,3,3]
        cam64 = d @ rot.T
        S = d.abs() @ rot.abs().T                                # sum |rot_i| |d_i| per coordinate
        z64 = cam64[..., 2]
        xy64 = cam64[..., :2] * f / (-z64[..., None])
        assert float(z64.max()) < -0.2                           # every vertex in front of the camera
        ez = (fz.cpu().double() - z64).abs()
        assert bool((ez <= PREPARE_ULPS * ULP * S[..., 2]).all()), float((ez / S[..., 2]).max() / ULP)
        bound = PREPARE_ULPS * ULP * ((f * S[..., :2] + xy64.abs() * S[..., 2:]) / z64.abs()[..., None] + xy64.abs())
        exy = (fxy.cpu().double() - xy64).abs()
        assert bool((exy <= bound).all()), float((exy / bound).max())


def _call_interp(dev, face_idx, bary, attr):
    from src.latent_paint.models.render import _InterpAttr
    a = attr.to(dev).requires_grad_()
    out = _InterpAttr.apply(a, face_idx.to(dev).int().contiguous(), bary.to(dev).contiguous())
    return a, out


@pytest.mark.parametrize("D", [1, 2, 3, 4, 16])
def test_interpolate_attributes_forward_backward(dev, D):
    g = torch.Generator().manual_seed(D)
    P, F_ = 3000, 50
    for one_face in (False, True):
        face_idx = torch.randint(-1, F_, (P,), generator=g)
        if one_face:
            face_idx[:] = 7                                       # every pixel on one face: full atomic contention
        b = torch.rand(P, 3, generator=g)
        bary = b / b.sum(1, keepdim=True)
        attr = torch.randn(F_, 3, D, generator=g)
        a, out = _call_interp(dev, face_idx, bary, attr)
        a64 = attr.double().requires_grad_()
        ref = RO.interpolate(face_idx, bary.double(), a64)
        scale = (bary.double()[..., None] * attr.double()[face_idx.clamp(min=0)].abs()).sum(1)
        assert bool(((out.detach().cpu().double() - ref).abs() <= 4 * ULP * scale).all())
        assert bool((out.detach().cpu()[face_idx < 0] == 0).all())
        dfeat = torch.randn(P, D, generator=g)
        out.backward(dfeat.to(dev))
        ref.backward(dfeat.double())
        # per element: its addends b * g, their count n and absolute sum
        fg = face_idx >= 0
        n = torch.zeros(F_, 3, D, dtype=torch.float64).index_add_(0, face_idx[fg], torch.ones(int(fg.sum()), 3, D,
                                                                                            dtype=torch.float64))
        s = torch.zeros(F_, 3, D, dtype=torch.float64).index_add_(
            0, face_idx[fg], (bary.double()[fg][..., None] * dfeat.double()[fg][:, None, :]).abs())
        err = (a.grad.cpu().double() - a64.grad).abs()
        assert bool((err <= (n + 4) * ULP * s).all()), float((err / ((n + 4) * ULP * s + 1e-300)).max())


def test_interpolate_attributes_rejects_d17(dev):
    from src.latent_nerf.raymarching import backend as _b
    face_idx = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(_b.LnerfError, match="bad sizes"):
        _call_interp(dev, face_idx, torch.full((8, 3), 1 / 3), torch.randn(1, 3, 17))


# ------------------------------------------------------------------------------------------------- texture map
def _tex_coords(uv, R, clip):
    """csrc/raster.hip tex_coords in f32, the same operations in the same order."""
    u = uv[:, 0].clamp(0, 1)
    v = uv[:, 1].clamp(0, 1)
    gx = u * 2.0 - 1.0
    gy = -(v * 2.0 - 1.0)
    x = ((gx + 1.0) * float(R) - 1.0) * 0.5
    y = ((gy + 1.0) * float(R) - 1.0) * 0.5
    if clip:
        x = x.clamp(0, R - 1)
        y = y.clamp(0, R - 1)
    return x, y


def _cubic64(t):
    A = -0.75
    t = t.double()

    def near(s):
        return ((A + 2) * s - (A + 3)) * s * s + 1

    def far(s):
        return ((A * s - 5 * A) * s + 8 * A) * s - 4 * A
    return torch.stack([far(t + 1), near(t), near(1 - t), far(2 - t)], -1)


def _taps(uv, R, mode):
    """(texel index [P,K] into R*R, float64 weight [P,K]) of every pixel's lookup."""
    x, y = _tex_coords(uv, R, mode != "bicubic")
    if mode == "nearest":
        return (torch.round(y).long() * R + torch.round(x).long())[:, None], torch.ones(uv.shape[0], 1,
                                                                                       dtype=torch.float64)
    xf, yf = torch.floor(x), torch.floor(y)
    ax, ay = (x - xf).double(), (y - yf).double()
    x0, y0 = xf.long(), yf.long()
    if mode == "bilinear":
        x1, y1 = (x0 + 1).clamp(max=R - 1), (y0 + 1).clamp(max=R - 1)
        idx = torch.stack([y0 * R + x0, y0 * R + x1, y1 * R + x0, y1 * R + x1], -1)
        w = torch.stack([(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay], -1)
        return idx, w
    wx, wy = _cubic64(x - xf), _cubic64(y - yf)
    k = torch.arange(4)
    xi = (x0[:, None] - 1 + k).clamp(0, R - 1)
    yi = (y0[:, None] - 1 + k).clamp(0, R - 1)
    idx = (yi[:, :, None] * R + xi[:, None, :]).reshape(-1, 16)
    w = (wy[:, :, None] * wx[:, None, :]).reshape(-1, 16)
    return idx, w


def _uv_cases(R, P_rand, g):
    k = torch.arange(R, dtype=torch.float32)
    centres = torch.stack(torch.meshgrid((k + 0.5) / R, (k + 0.5) / R, indexing="ij"), -1).reshape(-1, 2)
    ties = torch.stack(torch.meshgrid((k + 1) / R, (k + 1) / R, indexing="ij"), -1).reshape(-1, 2)
    edges = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [-0.3, 0.5], [1.4, -2.0], [0.5, 1.7],
                          [0.5 / R, 1 - 0.5 / R], [1.5 / R, 0.25 / R], [1 - 0.25 / R, 1 - 1.5 / R]])
    rnd = torch.rand(P_rand, 2, generator=g) * 1.4 - 0.2
    pile = torch.full((300, 2), 0.5 / R)                    # many pixels on one texel
    return torch.cat([centres[:4096], ties[:4096], edges, rnd, pile]).float().contiguous()


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
@pytest.mark.parametrize("R", [1, 2, 3, 8, 64])
def test_texture_map_forward_backward(dev, mode, R):
    from src.latent_paint.models.render import _MODES, _TextureMap
    g = torch.Generator().manual_seed(R * 7 + len(mode))
    for C in (1, 3, 4):
        uv = _uv_cases(R, 2000, g)
        P = uv.shape[0]
        for with_idx in (False, True):
            face_idx = None
            fg = torch.ones(P, dtype=torch.bool)
            if with_idx:
                fg = torch.rand(P, generator=g) > 0.2
                face_idx = torch.where(fg, torch.randint(0, 9, (P,), generator=g), torch.full((P,), -1))
            tex = torch.randn(1, C, R, R, generator=g)
            t = tex.to(dev).requires_grad_()
            out = _TextureMap.apply(t, uv.to(dev), None if face_idx is None else face_idx.int().to(dev), _MODES[mode])
            idx, w = _taps(uv, R, mode)
            werr = BICUBIC_W_ULPS * ULP if mode == "bicubic" else 0.0
            flat = tex.double().reshape(C, R * R)
            ref = (flat[:, idx] * w[None]).sum(-1).T                       # [P,C]
            ref[~fg] = 0
            got = out.detach().cpu().double()
            if mode == "nearest":
                assert torch.equal(got, ref), (C, with_idx)
            else:
                scale = (flat[:, idx].abs() * w.abs()[None]).sum(-1).T
                bound = (w.shape[1] + 2) * ULP * scale + werr * flat[:, idx].abs().sum(-1).T
                err = (got - ref).abs()
                assert bool((err <= bound).all()), (C, with_idx, float(err.max()))
            dout = torch.randn(P, C, generator=g)
            out.backward(dout.to(dev))
            gw = (w[None] * dout.double().T[:, :, None])                  # [C,P,K]
            keep = fg[None, :, None].expand_as(gw)
            gw = torch.where(keep, gw, torch.zeros(()).double())
            ix = idx[None].expand(C, -1, -1)
            dref = torch.zeros(C, R * R, dtype=torch.float64).scatter_add_(1, ix.reshape(C, -1), gw.reshape(C, -1))
            s = torch.zeros(C, R * R, dtype=torch.float64).scatter_add_(1, ix.reshape(C, -1), gw.abs().reshape(C, -1))
            n = torch.zeros(C, R * R, dtype=torch.float64).scatter_add_(1, ix.reshape(C, -1),
                                                                        keep.double().reshape(C, -1))
            gabs = torch.where(keep, dout.double().T[:, :, None].abs().expand_as(gw), torch.zeros(()).double())
            sg = torch.zeros(C, R * R, dtype=torch.float64).scatter_add_(1, ix.reshape(C, -1), gabs.reshape(C, -1))
            err = (t.grad.cpu().double().reshape(C, R * R) - dref).abs()     # per texel, not as a sum
            assert bool((err <= (n + 4) * ULP * s + werr * sg).all()), (C, with_idx, float(err.max()))


@pytest.mark.parametrize("mode", ["nearest", "bilinear", "bicubic"])
def test_texture_map_follows_grid_sample(dev, mode):
    """Away from nearest-rounding ties the lookup is F.grid_sample(align_corners=False, padding_mode='border') on
    (u, 1 - v) with uv clamped to [0, 1], in float64."""
    from src.latent_paint.models.render import _MODES, _TextureMap
    g = torch.Generator().manual_seed(5)
    for R in (3, 8, 64):
        uv = (torch.rand(4000, 2, generator=g) * 1.4 - 0.2).float()
        x, y = _tex_coords(uv, R, True)
        away = ((x - x.floor() - 0.5).abs() > 1e-3) & ((y - y.floor() - 0.5).abs() > 1e-3)
        uv = uv[away].contiguous()
        tex = torch.randn(1, 4, R, R, generator=g)
        got = _TextureMap.apply(tex.to(dev), uv.to(dev), None, _MODES[mode]).cpu().double()
        grid = uv.double().clamp(0, 1) * 2 - 1
        grid = torch.stack([grid[:, 0], -grid[:, 1]], -1).reshape(1, 1, -1, 2)
        ref = F.grid_sample(tex.double(), grid, mode=mode, align_corners=False, padding_mode="border")[0, :, 0].T
        if mode == "nearest":
            assert torch.equal(got, ref), R
        else:   # a convention error (half-texel shift, v flip, tap order) is of the order of the texel values
            assert float((got - ref).abs().max()) <= 1e-4 * float(tex.abs().max()), (R, float((got - ref).abs().max()))


def test_texture_map_rejects_non_square_or_batched_textures(dev):
    from src.latent_paint.models.render import _TextureMap
    uv = torch.rand(16, 2, device=dev)
    for shape in ((1, 3, 8, 16), (2, 3, 8, 8), (3, 8, 8)):
        with pytest.raises(ValueError, match=r"\[1,C,R,R\]"):
            _TextureMap.apply(torch.zeros(shape, device=dev), uv, None, 1)
