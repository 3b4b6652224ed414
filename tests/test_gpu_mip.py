"""The mip-mapped texture lookup (csrc/texmip.hip) on the GPU against the float64 references of tests/mip_reference.py.

* lnerf_uv_footprint: the reference consumes the GPU's own f32 face_xy / face_z / face_idx read back, so no rasteriser
  tie enters.  Per pixel |rho - rho64| <= K * ULP * scale with K = FOOTPRINT_ROUNDINGS and scale the magnitude the
  reference tracks (mip_reference.py states the rules).  First order: the dropped terms are K * ULP = 4e-6 of the bound.
* lnerf_mip_build: every level is three adds and an exact multiply on the level before, so level l is within
  4 l ULP of the box average of |texture| (4 ULP per level, the previous level's error averaged along); on textures of
  small integers every average is exact.  lnerf_mip_build_backward: one add per level, L ULP of the folded |gradients|
  (+ 1 for the second-order terms).
* lnerf_texture_mip_forward: the reference reads the GPU's own pyramid (held to its bound above), takes the texel
  coordinates in f32 (the kernel's bits) and everything else in float64.  Bound: the bilinear test's tap bound
  (4 + 2) ULP * sum |w| |texel| on both levels read, plus dlam * |bil(l0 + 1) - bil(l0)| for the error of lambda --
  the trilinear mix is continuous across integer lambda, so a floor that differs between f32 and float64 costs no more
  than that term on the pair of levels below.  dlam = c * 2^-23 * max(1, lambda) with c = 1 + 2: log2f's maximum error
  in the HIP math API reference of the ROCm documentation ("Single precision mathematical functions", log2f: 1 ULP,
  i.e. one spacing 2^-23 of the result) plus one each for the product rho * R and the bias add.
* lnerf_texture_mip_backward + lnerf_mip_build_backward: per texel of level 0 after the fold, (n + 4) ULP * s with n the
  addends that reach the texel through any level and s their absolute sum (the bilinear test's bound), plus the same
  dlam term, transposed: dlam * w * |g| on the taps of the levels lambda's error can move weight between."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import mip_reference as M
from tests.test_gpu_raster_ops import _uv_cases

pytestmark = pytest.mark.gpu

ULP = M.ULP
TAP_ULPS = 4 + 2        # tests/test_gpu_raster_ops.py: a sum of k = 4 taps is within k + 2 ulp of its absolute sum
LOG2F_ULPS = 1          # HIP math API reference, log2f
SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _dlam(lam):
    return (LOG2F_ULPS + 2) * 2.0 ** -23 * lam.clamp(min=1.0)


# ------------------------------------------------------------------------------------------------------- scenes
def _triangle():
    """One large triangle lying almost in the ground plane: seen obliquely from a low camera."""
    verts = torch.tensor([[-0.8, -0.1, 0.9], [0.9, -0.05, 0.7], [0.05, 0.1, -1.0]])
    uvs = torch.tensor([[0.05, 0.1], [0.95, 0.2], [0.4, 0.9]])
    views = [(70.0, 15.0, 1.6), (80.0, 200.0, 1.3), (35.0, 100.0, 2.0)]
    return verts, torch.tensor([[0, 1, 2]]), uvs[None], views, 0.0


def _quad(z_near=0.8, z_far=-2.5):
    """A long ground-plane quad of two triangles from just in front of the camera into the distance."""
    verts = torch.tensor([[-0.5, 0.0, z_near], [0.5, 0.0, z_near], [0.5, 0.0, z_far], [-0.5, 0.0, z_far]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    uvs = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    views = [(80.0, 0.0, 1.2), (75.0, 10.0, 1.25), (60.0, 340.0, 1.5)]
    return verts, faces, uvs[faces], views, 0.0


def _facing_quad():
    """The unit quad in the plane z = 0 with the whole texture on it."""
    verts = torch.tensor([[-0.5, -0.5, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0], [-0.5, 0.5, 0.0]])
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])
    uvs = torch.tensor([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    return verts, faces, uvs[faces][None]


def _blub():
    from src.latent_paint.models.mesh import Mesh
    mesh = Mesh(os.path.join(SHAPES, "blub.obj"))
    mesh.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    views = [(60.0, 30.0, 1.25), (100.0, 200.0, 1.0), (20.0, 120.0, 1.5)]
    return mesh.vertices, mesh.faces, mesh.vt[mesh.ft.long()], views, 0.25


def _rasterize(dev, scene, side, B):
    from src.latent_paint.models.render import Renderer, uv_footprint
    verts, faces, face_uv, views, look = scene
    views = views[:B]
    r = Renderer(dev, dim=(side, side), interpolation_mode="mipmap")
    face_idx, _, B_, H, W, face_xy, face_z = r._rasterize_views_faces(
        verts.to(dev), faces.to(dev), [math.radians(v[0]) for v in views], [math.radians(v[1]) for v in views],
        [v[2] for v in views], look, (side, side))
    face_uv = face_uv.reshape(-1, 3, 2).float().contiguous().to(dev)
    rho = uv_footprint(face_idx, face_xy, face_z, face_uv, B_, H, W)
    return face_idx.cpu(), face_xy.cpu(), face_z.cpu(), face_uv.cpu(), rho.cpu(), H, W


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("scene,side", [("triangle", 8), ("triangle", 16), ("quad", 16), ("blub", 32)])
def test_footprint_within_its_rounding_bound(dev, scene, side, B):
    sc = {"triangle": _triangle, "quad": _quad, "blub": _blub}[scene]()
    face_idx, face_xy, face_z, face_uv, rho, H, W = _rasterize(dev, sc, side, B)
    assert rho.shape == (B * H * W,) and face_xy.shape[0] == B
    ref, scale, k = M.footprint(face_idx, face_xy, face_z, face_uv, B, H, W)
    # K = 64: the count of roundings the result has accumulated in the kernel as written (mip_reference.py spells the
    # chain out; tests/test_mip_cpu.py holds the tracker to the same number)
    K = M.FOOTPRINT_ROUNDINGS
    assert k == K == 64
    fg = face_idx >= 0
    err = (rho.double() - torch.from_numpy(ref)).abs()
    bound = K * ULP * torch.from_numpy(scale)
    ratio = float((err[fg] / bound[fg]).max())
    print("footprint %s %dx%d B=%d: %d foreground pixels, max err / bound = %.3g, max scale / rho = %.3g" % (
        scene, side, side, B, int(fg.sum()), ratio, float((torch.from_numpy(scale)[fg] / torch.from_numpy(ref)[fg]).max())))
    assert int(fg.sum()) >= (4 if scene == "triangle" else 40) * B and int((~fg).sum()) > 0
    assert bool((rho[~fg] == 0).all())                           # background: exactly 0
    assert bool((rho[fg] > 0).all()) and bool(torch.isfinite(rho).all())
    assert bool((err <= bound).all()), ratio                     # no pixel excluded
    if scene == "quad":   # strong perspective: the footprint varies by more than 10 x over one face
        assert float(rho[fg].max() / rho[fg].min()) > 10


# ------------------------------------------------------------------------------------------------------- pyramid
def _levels_for(R):
    full = M.full_levels(R)
    return sorted({full, full // 2})


@pytest.mark.parametrize("R", [2, 8, 12, 64])
def test_pyramid_forward_and_backward(dev, R):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p
    from src.latent_paint.models.render import mip_build, mip_levels, mip_texels
    g = torch.Generator().manual_seed(R)
    assert mip_levels(R) == M.full_levels(R)
    for C in (1, 3, 4):
        for L in _levels_for(R):
            tex = torch.randn(C, R, R, generator=g)
            ints = torch.randint(-8, 9, (C, R, R), generator=g).float()
            if L == 0:
                assert mip_build(tex.to(dev), 0) is None
                continue
            offs, S = M.level_offsets(R, L)
            assert S == mip_texels(R, L)
            got = M.unpack(mip_build(tex.to(dev), L).cpu(), R, L)
            ref = M.pyramid(tex, L)
            mag = tex.double().abs()
            for l in range(1, L + 1):
                mag = M.pyramid_abs_step(mag)
                err = (got[l - 1].double() - ref[l]).abs()
                assert got[l - 1].shape == (C, R >> l, R >> l)
                assert bool((err <= 4 * l * ULP * mag).all()), (C, L, l, float((err / (ULP * mag)).max()))
            exact = M.unpack(mip_build(ints.to(dev), L).cpu(), R, L)     # sums of <= 4^L small integers over 4^L
            for a, b in zip(exact, M.pyramid(ints, L)[1:]):
                assert torch.equal(a.double(), b), (C, L)
            # the backward: folds dpyr into dtex, which it accumulates into
            dtex0 = torch.randn(C, R, R, generator=g)
            dlev = [torch.randn(C, R >> l, R >> l, generator=g) for l in range(1, L + 1)]
            dtex, dpyr = dtex0.to(dev), M.pack(dlev).contiguous().to(dev)
            assert dpyr.shape == (C, S)
            _b.call("lnerf_mip_build_backward", _p(dpyr), C, R, L, _p(dtex), None)
            want = M.pyramid_transpose([dtex0] + dlev)
            s = M.pyramid_transpose([dtex0.abs()] + [d.abs() for d in dlev])
            err = (dtex.cpu().double() - want).abs()                      # per texel
            assert bool((err <= (L + 1) * ULP * s).all()), (C, L, float((err / (ULP * s)).max()))


# ------------------------------------------------------------------------------------------------------- lookup
def _rho_cases(P, R, L, g):
    """rho per pixel so that lambda = log2(rho R) (+ bias) is: negative before the clamp, exactly 0, every exact
    integer up to L (exact where R is a power of two, else within an ulp of it: the floor may differ between f32 and
    float64 there), fractions, >= L, beyond L; and rho R <= 0."""
    lam = torch.rand(P, generator=g) * (L + 0.5) - 0.25                   # fractions, a few below 0 and above L
    rho = (2.0 ** lam.double() / R).float()
    kinds = [1.0 / 8 / R, 1.0 / R] + [2.0 ** l / R for l in range(1, L + 1)] + [2.0 ** L / R, 2.0 ** (L + 2) / R, 0.0, -1.0,
                                                                              2.0 ** -140]
    for n, v in enumerate(kinds):
        rho[n::3 * len(kinds)] = v
    return rho.contiguous()


def _lookup_reference(levels, uv, rho, fg, R, L, bias):
    vals, scales, taps = M.bilinear_levels(levels, uv)
    lam = M.lod(rho, R, L, bias)
    w, l0, t = M.level_weights(lam, L)
    ref = (w[:, :, None] * vals).sum(0)
    used = (w > 0).double()
    bound = TAP_ULPS * ULP * (used[:, :, None] * scales).sum(0)
    # the error of lambda moves weight between l0 and l0 + 1, or, where f32 and float64 may floor differently
    # (t within dlam of 0), between l0 - 1 and l0
    dl = _dlam(lam)
    P = uv.shape[0]
    ar = torch.arange(P)
    step = torch.zeros_like(ref)
    up = l0 < L
    step[up] = (vals[(l0 + 1).clamp(max=L), ar][up] - vals[l0, ar][up]).abs()
    low = (t <= dl) & (l0 >= 1)
    step[low] = torch.maximum(step[low], (vals[l0, ar][low] - vals[(l0 - 1).clamp(min=0), ar][low]).abs())
    bound = bound + dl[:, None] * step
    ref[~fg], bound[~fg] = 0, 0
    # which levels a pixel's gradient can reach, for the backward's dlam term
    reach = torch.zeros(L + 1, P, dtype=torch.bool)
    reach[l0, ar] = True
    reach[(l0 + 1).clamp(max=L), ar] = True
    reach[(l0 - 1).clamp(min=0), ar] |= low
    return ref, bound, lam, w, taps, dl, reach


@pytest.mark.parametrize("bias", [0.0, 0.75])
@pytest.mark.parametrize("R", [1, 2, 8, 12, 64])
def test_lookup_forward_backward(dev, R, bias):
    from src.latent_paint.models.render import mip_build, mip_lookup, mip_lookup_backward
    g = torch.Generator().manual_seed(R * 11 + int(bias * 4))
    L = M.full_levels(R)
    worst_f, worst_b = 0.0, 0.0
    for C in (1, 3, 4):
        uv = _uv_cases(R, 2000, g)
        P = uv.shape[0]
        rho = _rho_cases(P, R, L, g)
        for with_idx in (False, True):
            fg = torch.ones(P, dtype=torch.bool)
            face_idx = None
            if with_idx:
                fg = torch.rand(P, generator=g) > 0.2
                face_idx = torch.where(fg, torch.randint(0, 9, (P,), generator=g), torch.full((P,), -1)).int().to(dev)
            tex = torch.randn(C, R, R, generator=g)
            tex_d, uv_d, rho_d = tex.to(dev), uv.to(dev), rho.to(dev)
            pyr = mip_build(tex_d, L)
            out = mip_lookup(tex_d, pyr, uv_d, rho_d, face_idx, L, bias).cpu().double()
            levels = [tex] + (M.unpack(pyr.cpu(), R, L) if L else [])
            ref, bound, lam, w, taps, dl, reach = _lookup_reference(levels, uv, rho, fg, R, L, bias)
            if bias == 0.0 and L >= 1:   # the cases the rho set is built for are all there
                assert bool((lam == 0).any()) and bool((lam == L).any()) and bool(((lam > 0) & (lam < L)).any())
                assert bool(((rho.double() * R > 0) & (rho.double() * R < 1)).any()) and bool((rho <= 0).any())
                assert R & (R - 1) or all(bool((lam == l).any()) for l in range(L + 1))
            err = (out - ref).abs()
            worst_f = max(worst_f, float((err / bound.clamp(min=1e-300)).max()))
            assert bool((err <= bound).all()), (C, with_idx, float(err.max()), worst_f)
            assert bool((out[~fg] == 0).all())
            # ---- backward: level 0 after the fold, per texel
            dout = torch.randn(P, C, generator=g)
            got = mip_lookup_backward(dout.to(dev), (C, R), uv_d, rho_d, face_idx, L, bias).cpu().double()
            d, s, n, slack = [], [], [], []
            gT = torch.where(fg[None], dout.double().T, torch.zeros(()).double())          # [C,P]
            for l, (idx, tw) in enumerate(taps):
                r2 = (R >> l) ** 2
                ix = idx[None].expand(C, -1, -1).reshape(C, -1)
                gw = (w[l][None, :, None] * tw[None] * gT[:, :, None]).reshape(C, -1)
                live = ((w[l] > 0) & fg)[None, :, None].expand(C, -1, 4).double().reshape(C, -1)
                sl = ((reach[l] & fg).double() * dl)[None, :, None] * tw[None] * gT.abs()[:, :, None]
                zero = torch.zeros(C, r2, dtype=torch.float64)
                side = R >> l
                d.append(zero.scatter_add(1, ix, gw).reshape(C, side, side))
                s.append(zero.scatter_add(1, ix, gw.abs()).reshape(C, side, side))
                n.append(zero.scatter_add(1, ix, live).reshape(C, side, side))
                slack.append(zero.scatter_add(1, ix, sl.reshape(C, -1)).reshape(C, side, side))
            want, s0, slack0 = M.pyramid_transpose(d), M.pyramid_transpose(s), M.pyramid_transpose(slack)
            n0 = n[-1]
            for nl in reversed(n[:-1]):                                   # counts fold with weight 1
                n0 = nl + n0.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            berr = (got - want).abs()
            bbound = (n0 + 4) * ULP * s0 + slack0
            worst_b = max(worst_b, float((berr / bbound.clamp(min=1e-300)).max()))
            assert bool((berr <= bbound).all()), (C, with_idx, float(berr.max()), worst_b)
    print("lookup R=%d bias=%.2f: max forward err / bound = %.3g, max backward err / bound = %.3g" % (R, bias, worst_f,
                                                                                                      worst_b))


@pytest.mark.parametrize("R", [1, 2, 8, 12, 64])
def test_lookup_is_bilinear_bit_for_bit_where_the_footprint_is_at_most_a_texel(dev, R):
    from src.latent_paint.models.render import _MODES, _TextureMap, mip_build, mip_lookup
    g = torch.Generator().manual_seed(R)
    L = M.full_levels(R)
    for C in (1, 3, 4):
        uv = _uv_cases(R, 2000, g).to(dev)
        P = uv.shape[0]
        rho = (torch.rand(P, generator=g) / R).float()                    # rho R <= 1
        rho[::7], rho[1::7], rho[2::7] = 1.0 / R, 0.0, 0.5 / R
        assert float((rho * R).max()) <= 1.0
        face_idx = torch.where(torch.rand(P, generator=g) > 0.2, 3, -1).int().to(dev)
        tex = torch.randn(1, C, R, R, generator=g).to(dev)
        for idx in (None, face_idx):
            got = mip_lookup(tex[0], mip_build(tex[0], L), uv, rho.to(dev), idx, L, 0.0)
            assert torch.equal(got, _TextureMap.apply(tex, uv, idx, _MODES["bilinear"])), (C, idx is None)


# ------------------------------------------------------------------------------------------------------- end to end
def _render(dev, mode, tex, side, view, scene=None, **kw):
    from src.latent_paint.models.render import Renderer
    verts, faces, uv_attr = scene or _facing_quad()
    r = Renderer(dev, dim=(side, side), interpolation_mode=mode, **kw)
    elev, azim, radius = view
    return r.render_views_texture(verts.to(dev), faces.to(dev), uv_attr.to(dev), tex, [math.radians(elev)],
                                  [math.radians(azim)], [radius], 0.0)


FAR, CLOSE = (75.0, 20.0, 3.0), (85.0, 10.0, 0.8)


def _reference_lambda(dev, side, view, R, L):
    """lambda per pixel in float64 from the GPU's own rasterisation of the facing quad, and the foreground mask."""
    verts, faces, uv_attr = _facing_quad()
    scene = (verts, faces, uv_attr[0], [view], 0.0)
    face_idx, face_xy, face_z, face_uv, rho_gpu, H, W = _rasterize(dev, scene, side, 1)
    rho, _, _ = M.footprint(face_idx, face_xy, face_z, face_uv, 1, H, W)
    return M.lod(torch.from_numpy(rho), R, L, 0.0), face_idx >= 0, rho_gpu


def test_constant_texture_renders_as_that_constant(dev):
    R, side = 64, 16
    const = torch.tensor([0.75, -1.5, 3.0, 0.1])
    tex = const.view(1, 4, 1, 1).expand(1, 4, R, R).contiguous().to(dev)
    img, mask = _render(dev, "mipmap", tex, side, FAR)
    m = mask[0, 0].cpu() > 0
    assert 8 < int(m.sum()) < side * side
    got = img[0].cpu().double()
    # box averages of a constant are exact; a bilinear sum of four equal texels is within (4 + 2) ulp, the mix adds 3
    err = (got[:, m] - const.double()[:, None]).abs()
    assert bool((err <= (TAP_ULPS + 3) * ULP * const.double().abs()[:, None]).all()), float(err.max())
    assert bool((got[:, ~m] == 0).all())


def test_checkerboard_vanishes_where_the_footprint_exceeds_two_texels(dev):
    from src.latent_paint.models.render import mip_build
    R, side, L = 64, 16, 6
    k = torch.arange(R)
    board = (1.0 - 2.0 * ((k[:, None] + k[None, :]) % 2)).float()          # +-1, period 2 texels
    tex = board.expand(1, 3, R, R).contiguous().to(dev)
    assert bool((mip_build(tex[0], L) == 0).all())                        # every level >= 1 is exactly 0
    lam, fg, _ = _reference_lambda(dev, side, FAR, R, L)
    coarse = fg & (lam >= 1)
    assert int(coarse.sum()) > 8
    img, _ = _render(dev, "mipmap", tex, side, FAR)
    got = img[0].reshape(3, -1).cpu()
    assert bool((got[:, coarse] == 0).all())
    bil, _ = _render(dev, "bilinear", tex, side, FAR)
    assert float(bil[0].reshape(3, -1).cpu()[:, coarse].abs().max()) > 0.1   # the point lookup aliases


def test_far_view_gradient_reaches_every_texel_under_the_footprints(dev):
    R, side, L, C = 64, 16, 6, 2
    tex = torch.zeros(1, C, R, R, device=dev, requires_grad=True)
    img, mask = _render(dev, "mipmap", tex, side, FAR)
    img.backward(torch.ones_like(img))
    hit = tex.grad[0].cpu() != 0
    assert torch.equal(hit[0], hit[1])
    # the reference's count: the taps of the two levels around each foreground pixel's lambda, folded to level 0
    lam, fg, _ = _reference_lambda(dev, side, FAR, R, L)
    verts, faces, uv_attr = _facing_quad()
    from src.latent_paint.models.render import Renderer, _InterpAttr
    r = Renderer(dev, dim=(side, side), interpolation_mode="mipmap")
    face_idx, bary, _, _, _ = r._rasterize_views(verts.to(dev), faces.to(dev), [math.radians(FAR[0])],
                                                 [math.radians(FAR[1])], [FAR[2]], 0.0, (side, side))
    uv = _InterpAttr.apply(uv_attr[0].to(dev).contiguous(), face_idx, bary).cpu()
    w, _, _ = M.level_weights(lam, L)
    marks = []
    for l in range(L + 1):
        idx, tw = M.bilinear_taps(uv, R >> l)
        live = ((w[l] > 0) & fg)[:, None] & (tw > 0)
        flat = torch.zeros((R >> l) ** 2, dtype=torch.float64).scatter_add(0, idx.reshape(-1), live.double().reshape(-1))
        marks.append(flat.reshape(1, R >> l, R >> l))
    want = M.pyramid_transpose(marks)[0] > 0
    n_px = int(fg.sum())
    print("far view: %d foreground pixels, %d texels with a gradient (bilinear reaches at most %d)" % (
        n_px, int(hit[0].sum()), 4 * n_px))
    assert int(hit[0].sum()) == int(want.sum()) and torch.equal(hit[0], want)
    assert int(hit[0].sum()) > 4 * side * side                            # more than bilinear can reach from H * W pixels
    bil_tex = torch.zeros(1, C, R, R, device=dev, requires_grad=True)
    bil, _ = _render(dev, "bilinear", bil_tex, side, FAR)
    bil.backward(torch.ones_like(bil))
    assert int((bil_tex.grad[0, 0] != 0).sum()) <= 4 * n_px


def test_close_view_is_the_bilinear_render_bit_for_bit(dev):
    R, side = 8, 32
    _, fg, rho = _reference_lambda(dev, side, CLOSE, R, 3)
    assert int(fg.sum()) > side * side // 2 and float(rho.max()) * R <= 1.0   # at most one texel under every pixel
    g = torch.Generator().manual_seed(4)
    tex = torch.randn(1, 4, R, R, generator=g).to(dev)
    img, mask = _render(dev, "mipmap", tex, side, CLOSE)
    bil, bmask = _render(dev, "bilinear", tex, side, CLOSE)
    assert torch.equal(img, bil) and torch.equal(mask, bmask)
    # ... and so is any view of a texture with no levels (odd side), or with the levels capped at 0
    odd = torch.randn(1, 4, 9, 9, generator=g).to(dev)
    assert torch.equal(_render(dev, "mipmap", odd, 16, FAR)[0], _render(dev, "bilinear", odd, 16, FAR)[0])
    big = torch.randn(1, 4, 64, 64, generator=g).to(dev)
    assert torch.equal(_render(dev, "mipmap", big, 16, FAR, max_mip_level=0)[0], _render(dev, "bilinear", big, 16, FAR)[0])
    assert not torch.equal(_render(dev, "mipmap", big, 16, FAR)[0], _render(dev, "bilinear", big, 16, FAR)[0])
    # a positive bias moves every pixel up the pyramid: the render changes again
    assert not torch.equal(_render(dev, "mipmap", big, 16, FAR, lod_bias=1.0)[0], _render(dev, "mipmap", big, 16, FAR)[0])


def _paint_cfg(tmp_path, **over):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "mip", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(SHAPES, "blub.obj"), "guide.texture_resolution": 64,
            "guide.texture_interpolation_mode": "mipmap"}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def test_trainer_step_and_checkpoint_with_mipmap(dev, tmp_path):
    from src.latent_paint.training.trainer import Trainer
    tr = Trainer(_paint_cfg(tmp_path), device=dev)
    r = tr.mesh_model.renderer
    assert (r.interpolation_mode, r.max_mip_level, r.lod_bias) == ("mipmap", -1, 0.0)
    tex0 = tr.mesh_model.texture_img.detach().clone()
    data = next(iter(tr.dataloaders["train"]))
    tr.train_step += 1
    tr.optimizer.zero_grad()
    pred, _ = tr.train_render(data)
    tr.optimizer.step()
    assert pred.shape == (1, 4, 64, 64) and bool(torch.isfinite(pred).all())
    moved = (tr.mesh_model.texture_img.detach() - tex0).abs() > 0
    assert int(moved.sum()) > 1000                            # Adam at eps = 1e-15 moves every texel that got a gradient
    path = tr.save_checkpoint(full=True)
    tr2 = Trainer(_paint_cfg(tmp_path, **{"optim.resume": True, "guide.texture_max_mip_level": 2,
                                          "guide.texture_lod_bias": 0.5}), device=dev)
    assert path.exists() and tr2.train_step == 2
    assert torch.equal(tr2.mesh_model.texture_img, tr.mesh_model.texture_img)
    assert not torch.equal(tr2.mesh_model.texture_img.detach(), tex0)
    r2 = tr2.mesh_model.renderer
    assert (r2.max_mip_level, r2.lod_bias) == (2, 0.5)


def test_render_test_with_a_decoded_texture_of_another_side(dev, tmp_path):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    cfg = _paint_cfg(tmp_path)
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=64)
    decode = lambda side: (lambda t: F.interpolate(t[:, :3].sigmoid(), (side, side), mode="bilinear"))
    view = (math.radians(60.0), math.radians(30.0), 1.25)
    with torch.no_grad():
        big = model.render(*view, decode_func=decode(512), test=True, dims=(48, 48))      # 8 R: nine levels
        odd = model.render(*view, decode_func=decode(63), test=True, dims=(48, 48))       # no level: plain bilinear
        model.renderer.interpolation_mode = "bilinear"
        odd_bil = model.render(*view, decode_func=decode(63), test=True, dims=(48, 48))
        big_bil = model.render(*view, decode_func=decode(512), test=True, dims=(48, 48))
    assert big["image"].shape == (1, 3, 48, 48) and big["texture_map"].shape == (1, 3, 512, 512)
    assert bool(torch.isfinite(big["image"]).all()) and float(big["image"][0, :, 0, 0].min()) == 1.0   # white background
    assert torch.equal(big["mask"], big_bil["mask"]) and 0.05 < float(big["mask"].mean()) < 0.9
    assert torch.equal(odd["image"], odd_bil["image"])
    # a 48^2 view of a 512^2 texture is minified: the filtered render differs from the point lookup, within the
    # texture's range
    assert not torch.equal(big["image"], big_bil["image"])
    assert float(big["image"].min()) >= 0.0 and float(big["image"].max()) <= 1.0 + 1e-6
