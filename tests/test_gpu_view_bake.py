"""View-projected albedo on the MI355X: lnerf_uv_project_views against a float64 restatement of its rule (this file,
`ref_*`), exact properties on quads, view_zbuffer against the rasteriser's own calls, and the two exports end to end
(NeRFRenderer.export_mesh(bake_views=K), TexturedMeshModel.export_mesh(bake_views=K))."""
import itertools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")
COS_MIN, POWER, SLACK = 0.2, 4.0, 2.0          # the defaults of project_views


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------ float64 restatement of the rule
def ref_steps(pos, nrm, cams, zbuf, cos_min, slack, du=0.0, dv=0.0, dc=0.0, dz=0.0):
    """Steps 1-5 of include/lnerf_hip.h (lnerf_uv_project_views) in float64 for every (point, view) pair.
    pos, nrm [P,3], cams [K,14], zbuf [K,H,W].  du, dv (pixels), dc and dz (a fraction of |z|) move u, v, the cosine
    and the depth that is tested: the probes of the fragility rule.
    -> dict(step [P,K]: 0 = accepted, else the step that rejected; c, i0, j0, tu, tv [P,K])."""
    K, H, W = zbuf.shape
    rot, eye, fx, fy = cams[:, :9].reshape(K, 3, 3), cams[:, 9:12], cams[:, 12], cams[:, 13]
    d = eye[None] - pos[:, None]                                           # [P,K,3]
    c = (nrm[:, None] * d).sum(-1) / np.linalg.norm(d, axis=-1) + dc
    p = np.einsum("kij,pkj->pki", rot, -d)
    pz = p[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        X, Y = fx * p[..., 0] / -pz, fy * p[..., 1] / -pz
        u, v = ((X + 1) * W - 1) / 2 + du, ((1 - Y) * H - 1) / 2 + dv
        j0, i0 = np.floor(u), np.floor(v)
        inside = (pz < 0) & (j0 >= 0) & (j0 + 1 <= W - 1) & (i0 >= 0) & (i0 + 1 <= H - 1)
        tu, tv = u - j0, v - i0
        j = np.where(inside, j0, 0).astype(np.int64)
        i = np.where(inside, i0, 0).astype(np.int64)
        k = np.arange(K)[None]
        taps = np.stack([zbuf[k, i, j], zbuf[k, i, j + 1], zbuf[k, i + 1, j], zbuf[k, i + 1, j + 1]], -1)
        near = (tv >= 0.5) * 2 + (tu >= 0.5)
        zt = np.take_along_axis(taps, near[..., None], -1)[..., 0]
        bias = slack * -pz * 2 / np.minimum(fx * W, fy * H) * np.sqrt(np.maximum(1 - c * c, 0)) / c + 1e-4 * -pz
        fails = [~(c >= cos_min), ~(pz < 0), ~inside, ~(taps < 0).all(-1), ~(pz + dz * np.abs(pz) >= zt - bias)]
    step = np.zeros(c.shape, np.int64)
    for n in (5, 4, 3, 2, 1):
        step = np.where(fails[n - 1], n, step)
    return dict(step=step, c=c, i0=i, j0=j, tu=tu, tv=tv)


def ref_project(pos, nrm, cams, zbuf, images, cos_min=COS_MIN, power=POWER, slack=SLACK):
    """The whole rule in float64 -> (out [P,C], weight [P], count [P], step [P,K])."""
    pos, nrm, cams, zbuf, images = (np.asarray(a, np.float64) for a in (pos, nrm, cams, zbuf, images))
    s = ref_steps(pos, nrm, cams, zbuf, cos_min, slack)
    ok = s["step"] == 0
    K, C = images.shape[:2]
    k, i, j, tu, tv = np.arange(K)[None], s["i0"], s["j0"], s["tu"][..., None], s["tv"][..., None]
    tap = lambda di, dj: images[k, :, i + di, j + dj]                            # [P,K,C]
    col = (1 - tu) * (1 - tv) * tap(0, 0) + tu * (1 - tv) * tap(0, 1) + (1 - tu) * tv * tap(1, 0) + tu * tv * tap(1, 1)
    w = np.where(ok, np.where(ok, s["c"], 1.0) ** power, 0.0)
    weight = w.sum(1)
    acc = (w[..., None] * np.where(ok[..., None], col, 0.0)).sum(1)
    out = np.where(weight[:, None] > 0, acc / np.where(weight > 0, weight, 1.0)[:, None], 0.0)
    return out, weight, ok.sum(1), s["step"]


def ref_fragile(pos, nrm, cams, zbuf, cos_min=COS_MIN, slack=SLACK):
    """[P] bool: some accept / reject decision of the point changes when u or v moves by 2e-4 px, c by 1e-5 or z by
    1e-5 |z| (every combination of signs): a decision float32 may take the other way."""
    pos, nrm, cams, zbuf = (np.asarray(a, np.float64) for a in (pos, nrm, cams, zbuf))
    base = ref_steps(pos, nrm, cams, zbuf, cos_min, slack)["step"] == 0
    frag = np.zeros(pos.shape[0], bool)
    for du, dv, dc, dz in itertools.product((-2e-4, 0.0, 2e-4), (-2e-4, 0.0, 2e-4), (-1e-5, 0.0, 1e-5), (-1e-5, 0.0, 1e-5)):
        ok = ref_steps(pos, nrm, cams, zbuf, cos_min, slack, du, dv, dc, dz)["step"] == 0
        frag |= (ok != base).any(1)
    return frag


# ------------------------------------------------------------------------------ scenes
def _icosphere(subdiv, radius, centre=(0.0, 0.0, 0.0)):
    from src.latent_nerf.training.shape import make_icosphere
    v, f = make_icosphere(subdiv, radius)
    return v.numpy() + np.float32(centre), f.numpy()


def two_spheres():
    """An r = 0.5 icosphere at the origin (320 faces) and an r = 0.2 one at (0.6, 0.1, 0.3) (80 faces): real occlusion."""
    v0, f0 = _icosphere(2, 0.5)
    v1, f1 = _icosphere(1, 0.2, (0.6, 0.1, 0.3))
    assert len(f0) == 320 and len(f1) == 80
    return np.concatenate([v0, v1]).astype(np.float32), np.concatenate([f0, f1 + len(v0)])


def winding_normals(v, f):
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def sample_surface(v, f, P, rng):
    """P points uniform over the surface, with the winding normal of their face -> (pos, nrm) f32."""
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    area = np.linalg.norm(n, axis=-1)
    face = rng.choice(len(f), P, p=area / area.sum())
    r1, r2 = np.sqrt(rng.uniform(0, 1, P)), rng.uniform(0, 1, P)
    b = np.stack([1 - r1, r1 * (1 - r2), r1 * r2], -1)
    pos = (b[..., None] * tri[face]).sum(1)
    return pos.astype(np.float32), (n[face] / area[face, None]).astype(np.float32)


def smooth_images(K, C, H, W):
    """A smooth function of (k, channel, i, j), at most 0.06 per pixel steep: the bilinear weights matter, and the
    float32 error of u and v (about 1e-5 px) moves a colour by less than 1e-6."""
    k, c, i, j = np.meshgrid(np.arange(K), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    return (0.5 + 0.3 * np.sin(0.11 * i + 0.07 * j * (1 + 0.1 * c) + k) + 0.1 * np.cos(0.13 * j - 0.05 * i + c)).astype(np.float32)


def fibonacci_cameras(K, radius, fovy, H, W, dev):
    from src.latent_nerf.raymarching import bake_view_poses
    from src.view_bake import view_cameras
    return view_cameras(bake_view_poses(K), radius, fovy, H, W, dev)[0]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _close(got, want, bound=1e-5):
    return np.abs(got - want) <= bound * np.maximum(1.0, np.abs(want))


# ------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("C", [3, 4, 1])
def test_kernel_matches_float64_restatement(dev, C):
    from src.latent_nerf.raymarching import project_views, view_zbuffer
    v, f = two_spheres()
    assert (np.einsum("fi,fi->f", winding_normals(v, f[:320]), v[f[:320]].mean(1)) > 0).all()   # wound outwards
    P, K, H, W = 4096, 6, 48, 48
    pos, nrm = sample_surface(v, f, P, np.random.default_rng(5))
    cams = fibonacci_cameras(K, 1.8, 55.0, H, W, dev)
    images = smooth_images(K, C, H, W)
    zbuf = view_zbuffer(_t(v, dev), _t(f, dev), cams, H, W)
    out, weight, count = project_views(_t(pos, dev), _t(nrm, dev), cams, zbuf, _t(images, dev))
    torch.cuda.synchronize()
    cams_h, zbuf_h = cams.cpu().numpy(), zbuf.cpu().numpy()
    want_out, want_weight, want_count, step = ref_project(pos, nrm, cams_h, zbuf_h, images)
    fragile = ref_fragile(pos, nrm, cams_h, zbuf_h)
    solid = ~fragile
    print("fragile %.3f %%, seen %.2f %%, rejected per step %s" % (100 * fragile.mean(), 100 * (want_count > 0).mean(),
                                                                  [int((step == n).sum()) for n in (1, 2, 3, 4, 5)]))
    assert fragile.mean() <= 0.01
    # the scene exercises the rule
    for n in (1, 3, 4, 5):
        assert (step == n).any(), "no pair is rejected by step %d" % n
    assert (want_count > 0).mean() >= 0.90
    got_out, got_weight, got_count = out.cpu().numpy(), weight.cpu().numpy(), count.cpu().numpy()
    assert got_out.shape == (P, C) and got_count.dtype == np.int32
    assert np.array_equal(got_count[solid], want_count[solid])
    assert _close(got_weight[solid], want_weight[solid]).all(), np.abs(got_weight - want_weight)[solid].max()
    assert _close(got_out[solid], want_out[solid]).all(), np.abs(got_out - want_out)[solid].max()
    assert (got_out[got_count == 0] == 0).all() and (got_weight[got_count == 0] == 0).all()


def test_more_views_than_one_camera_tile_and_a_ragged_block(dev):
    """K = 70 views (the kernel stages 64 camera records at a time) over P = 1000 points (no multiple of the workgroup)."""
    from src.latent_nerf.raymarching import project_views, view_zbuffer
    v, f = two_spheres()
    P, K, H, W = 1000, 70, 24, 32
    pos, nrm = sample_surface(v, f, P, np.random.default_rng(9))
    cams = fibonacci_cameras(K, 1.8, 55.0, H, W, dev)
    images = smooth_images(K, 2, H, W)
    zbuf = view_zbuffer(_t(v, dev), _t(f, dev), cams, H, W)
    out, weight, count = project_views(_t(pos, dev), _t(nrm, dev), cams, zbuf, _t(images, dev))
    torch.cuda.synchronize()
    cams_h, zbuf_h = cams.cpu().numpy(), zbuf.cpu().numpy()
    want_out, want_weight, want_count, step = ref_project(pos, nrm, cams_h, zbuf_h, images)
    solid = ~ref_fragile(pos, nrm, cams_h, zbuf_h)
    assert solid.mean() >= 0.9 and (step[:, 64:] == 0).any()            # views of the second tile are accepted too
    assert np.array_equal(count.cpu().numpy()[solid], want_count[solid])
    # K = 70 terms: the bound of the 6-view test scaled by the accumulated terms, (70 + 10) / (6 + 10)
    bound = 1e-5 * (K + 10) / 16
    assert _close(weight.cpu().numpy()[solid], want_weight[solid], bound).all()
    assert _close(out.cpu().numpy()[solid], want_out[solid], bound).all()
    empty = project_views(torch.zeros(0, 3, device=dev), torch.zeros(0, 3, device=dev), cams, zbuf, _t(images, dev))
    assert empty[0].shape == (0, 2) and empty[2].shape == (0,)


# ------------------------------------------------------------------------------ 2. exact properties on quads
def _quad(half, z, flip=False):
    v = np.float32([[-half, -half, z], [half, -half, z], [half, half, z], [-half, half, z]])
    f = np.array([[0, 1, 2], [0, 2, 3]])                                  # counter-clockwise seen from +z: normal +z
    return v, (f[:, ::-1] if flip else f)


FX = 1.0 / math.tan(math.radians(30.0))                                  # fov 60 degrees
HEAD_ON = [1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 2.0, FX, FX]                 # eye (0, 0, 2), looking down -z
BEHIND = [-1, 0, 0, 0, 1, 0, 0, 0, -1, 0, 0, -2.0, FX, FX]               # eye (0, 0, -2), looking up +z
PX = 2.0 / FX * 2 / 32                                                   # a pixel's side on the plane z = 0, 32 x 32


def _quad_points(n, rng, half=1.0):
    pos = np.zeros((n, 3), np.float32)
    pos[:, :2] = rng.uniform(-half, half, (n, 2))
    return pos, np.tile(np.float32([0, 0, 1]), (n, 1))


def _ulps(got, want):
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def test_exact_properties_on_quads(dev):
    from src.latent_nerf.raymarching import project_views, view_zbuffer
    H = W = 32
    rng = np.random.default_rng(2)
    va, fa = _quad(1.0, 0.0)
    pos, nrm = _quad_points(3001, rng)
    cam = torch.tensor([HEAD_ON], device=dev)
    z_a = view_zbuffer(_t(va, dev), _t(fa, dev), cam, H, W)
    assert int((z_a < 0).sum()) == 28 * 28                               # the quad spans 27.7 px: 28 pixel centres a side
    # a constant image comes back within 2 ulp wherever a view is accepted
    colour = np.float32([0.3, 0.7712345, 0.05])
    const = torch.from_numpy(colour).to(dev).view(1, 3, 1, 1).expand(1, 3, H, W).contiguous()
    out, weight, count = project_views(_t(pos, dev), _t(nrm, dev), cam, z_a, const)
    cnt = count.cpu().numpy()
    r = np.abs(pos[:, :2]).max(1)
    assert (cnt[r < 1.0 - 2 * PX] == 1).all() and 0.7 < cnt.mean() < 1.0      # the rim's taps touch the background
    assert _ulps(out.cpu().numpy()[cnt == 1], np.tile(colour, ((cnt == 1).sum(), 1))).max() <= 2
    # two calls are bitwise equal
    again = project_views(_t(pos, dev), _t(nrm, dev), cam, z_a, const)
    assert all(torch.equal(a, b) for a, b in zip((out, weight, count), again))
    # a nearer quad (half 0.3 at z = 0.8) shadows the square of half 0.5 on the far one
    vb, fb = _quad(0.3, 0.8)
    both_v, both_f = np.concatenate([va, vb]), np.concatenate([fa, fb + 4])
    z_ab = view_zbuffer(_t(both_v, dev), _t(both_f, dev), cam, H, W)
    cnt = project_views(_t(pos, dev), _t(nrm, dev), cam, z_ab, const)[2].cpu().numpy()
    inner, outer = r < 0.5 - 2 * PX, (r > 0.5 + 2 * PX) & (r < 1.0 - 2 * PX)
    assert inner.sum() > 300 and outer.sum() > 300
    assert (cnt[inner] == 0).all() and (cnt[outer] == 1).all()
    # a camera behind the quad sees its back: nothing is accepted
    back = torch.tensor([BEHIND], device=dev)
    z_back = view_zbuffer(_t(va, dev), _t(fa, dev), back, H, W)
    assert int((z_back < 0).sum()) == 28 * 28
    assert int(project_views(_t(pos, dev), _t(nrm, dev), back, z_back, const)[2].sum()) == 0
    # cos_min above the largest cosine of the points: nothing is accepted
    d = np.float64([0, 0, 2.0]) - pos.astype(np.float64)
    cos = d[:, 2] / np.linalg.norm(d, axis=1)
    far = cos < 0.998
    assert far.sum() > 2500
    cnt = project_views(_t(pos[far], dev), _t(nrm[far], dev), cam, z_a, const, cos_min=0.999)[2]
    assert int(cnt.sum()) == 0
    assert int(project_views(_t(pos[far], dev), _t(nrm[far], dev), cam, z_a, const, cos_min=0.5)[2].sum()) > 1500


def test_view_order_changes_only_the_rounding(dev):
    from src.latent_nerf.raymarching import project_views, view_zbuffer
    v, f = two_spheres()
    P, K, H, W = 2000, 5, 32, 32
    pos, nrm = sample_surface(v, f, P, np.random.default_rng(4))
    cams = fibonacci_cameras(K, 1.8, 55.0, H, W, dev)
    images = _t(smooth_images(K, 3, H, W), dev)
    zbuf = view_zbuffer(_t(v, dev), _t(f, dev), cams, H, W)
    a = project_views(_t(pos, dev), _t(nrm, dev), cams, zbuf, images)
    perm = torch.tensor([3, 0, 4, 2, 1], device=dev)
    b = project_views(_t(pos, dev), _t(nrm, dev), cams[perm].contiguous(), zbuf[perm].contiguous(), images[perm].contiguous())
    assert torch.equal(a[2], b[2]) and int((a[2] > 1).sum()) > 200
    assert _close(b[1].cpu().numpy(), a[1].cpu().numpy()).all() and _close(b[0].cpu().numpy(), a[0].cpu().numpy()).all()


# ------------------------------------------------------------------------------ 3. view_zbuffer
def test_view_zbuffer_is_the_rasterisers_depth(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching import view_zbuffer
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    from src.latent_paint.models.render import _InterpAttr
    v, f = _icosphere(2, 0.5)
    K, H, W = 3, 40, 56
    cams = fibonacci_cameras(K, 1.8, 55.0, H, W, dev)
    verts, faces = _t(v, dev), _t(f, dev).to(torch.int32).contiguous()
    F = faces.shape[0]
    face_z, face_xy = torch.empty(K, F, 3, device=dev), torch.empty(K, F, 3, 2, device=dev)
    face_box = torch.empty(K, F, 4, device=dev, dtype=torch.int16)
    _b.call("lnerf_raster_prepare_batch", _p(verts), verts.shape[0], _p(faces), F, _p(cams), K, H, W, _p(face_z),
            _p(face_xy), _p(face_box), _stream())
    face_idx = torch.empty(K, H * W, device=dev, dtype=torch.int32)
    bary = torch.empty(K, H * W, 3, device=dev)
    _b.call("lnerf_rasterize_batch", K, H, W, _p(face_z), _p(face_xy), _p(face_box), F, _p(face_idx), _p(bary), _stream())
    want = torch.stack([_InterpAttr.apply(face_z[k].reshape(F, 3, 1).contiguous(), face_idx[k], bary[k])[:, 0]
                        for k in range(K)]).view(K, H, W)
    fg = (face_idx >= 0).view(K, H, W)
    zbuf = view_zbuffer(verts, faces, cams, H, W)
    assert zbuf.shape == (K, H, W) and 0.05 < float(fg.float().mean()) < 0.5
    assert torch.equal(zbuf[fg].view(torch.int32), want[fg].view(torch.int32))
    assert bool((zbuf[fg] < 0).all()) and bool((zbuf[~fg] >= 0).all())
    # the sphere's nearest point is 1.3 from every eye
    assert abs(float(zbuf[fg].max()) + 1.3) < 0.02
    # erode = 2: exactly the pixels within 2 (Chebyshev) of a background pixel go
    bg = (~fg).cpu().numpy()
    pad = np.pad(bg, ((0, 0), (2, 2), (2, 2)))
    grown = np.zeros_like(bg)
    for di in range(5):
        for dj in range(5):
            grown |= pad[:, di:di + H, dj:dj + W]
    eroded = view_zbuffer(verts, faces, cams, H, W, erode=2)
    assert np.array_equal((eroded >= 0).cpu().numpy(), grown) and grown.sum() > bg.sum()
    keep = torch.from_numpy(~grown).to(dev)
    assert torch.equal(eroded[keep], zbuf[keep])
    with pytest.raises(ValueError, match="erode"):
        view_zbuffer(verts, faces, cams, H, W, erode=-1)
    with pytest.raises(ValueError, match="cams"):
        view_zbuffer(verts, faces, cams[:, :13], H, W)


# ------------------------------------------------------------------------------ 4. NeRF export
def _nerf(dev, nerf_type="latent"):
    """The fixture of tests/test_gpu_uv_bake.py (f32)."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    cfg = RenderConfig(grid_size=32, train_h=16, train_w=16, nerf_type=NeRFType(nerf_type))
    return NeRFNetwork(cfg, log2_hashmap_size=14).to(dev), cfg


def _constant_views(colours, side):
    """A view_decoder that ignores its input: view k is the constant colour colours[k] at side x side."""
    q = torch.tensor(colours, dtype=torch.float32)

    def decoder(renders):
        assert renders.shape[0] == q.shape[0]
        return q.to(renders.device).view(-1, 3, 1, 1).expand(-1, 3, side, side).contiguous()
    return decoder


def test_nerf_export_bakes_the_decoded_views(dev, tmp_path):
    from PIL import Image
    net, cfg = _nerf(dev)
    K, R = 16, 256
    kw = dict(resolution=64, S=32, thresh=cfg.density_thresh, texture_resolution=R)
    plain = net.export_mesh(str(tmp_path / "plain"), **kw)
    assert {p.name for p in (tmp_path / "plain").iterdir()} == {"mesh.obj", "mesh.mtl", "albedo.png", "latent_texture.pt"}
    assert "view_rgb" not in plain
    # view k has the colour a + s_k (b - a): the convex hull of the colours is the segment from a to b
    a, b = np.float32([0.9, 0.2, 0.1]), np.float32([0.1, 0.6, 0.8])
    s = np.linspace(0.0, 1.0, K, dtype=np.float32)
    colours = (a[None] + s[:, None] * (b - a)[None]).tolist()
    out = net.export_mesh(str(tmp_path / "views"), bake_views=K, view_size=64, view_decoder=_constant_views(colours, 128), **kw)
    names = {p.name for p in (tmp_path / "views").iterdir()}
    assert names == {"mesh.obj", "mesh.mtl", "albedo.png", "albedo_preview.png", "latent_texture.pt"}
    assert out["view_rgb"].shape == (3, R, R) and out["view_weight"].shape == (R, R) and out["view_count"].shape == (R, R)
    assert out["view_count"].dtype == torch.int32
    for key in ("rgb", "texture", "mask", "verts", "faces", "vt", "ft"):          # the point bake is untouched
        assert torch.equal(out[key], plain[key]), key
    for name in ("latent_texture.pt", "mesh.obj", "mesh.mtl"):
        assert (tmp_path / "views" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    assert (tmp_path / "views" / "albedo_preview.png").read_bytes() == (tmp_path / "plain" / "albedo.png").read_bytes()
    img = np.asarray(Image.open(tmp_path / "views" / "albedo.png"))
    assert np.array_equal(img, (out["view_rgb"].permute(1, 2, 0).cpu().numpy() * 255).round().astype(np.uint8))
    covered, seen = out["mask"] == 2, out["view_count"] > 0
    assert int((covered & seen).sum()) > 1000 and not bool((seen & ~covered).any())
    got = out["view_rgb"].permute(1, 2, 0)[covered & seen].cpu().numpy().astype(np.float64)
    t = (got - a) @ (b - a).astype(np.float64) / float(((b - a).astype(np.float64) ** 2).sum())
    assert (t >= -1e-5).all() and (t <= 1 + 1e-5).all()
    assert np.abs(got - (a + t[:, None] * (b - a))).max() <= 1e-5
    assert float(t.max() - t.min()) > 0.5                                          # several views did contribute
    unseen = covered & ~seen                                  # (16 views may well see all of this surface: see below)
    assert torch.equal(out["view_rgb"][:, unseen], out["rgb"][:, unseen])
    # every pixel eroded: no view is accepted anywhere, and every covered texel is the point bake's
    none = net.export_mesh(str(tmp_path / "none"), bake_views=K, view_size=64, view_decoder=_constant_views(colours, 128),
                           view_erode=1000, **kw)
    assert int(none["view_count"].sum()) == 0 and int(covered.sum()) > 1000
    assert torch.equal(none["view_rgb"][:, covered], none["rgb"][:, covered])
    # a moderate erosion leaves some texels to the views and hands the rest back
    some = net.export_mesh(str(tmp_path / "some"), bake_views=K, view_size=64, view_decoder=_constant_views(colours, 128),
                           view_erode=8, **kw)
    part = some["view_count"] > 0
    print("erode 8: %d of %d covered texels seen" % (int((covered & part).sum()), int(covered.sum())))
    assert bool((out["view_count"] >= some["view_count"]).all())
    assert torch.equal(some["view_rgb"][:, covered & ~part], some["rgb"][:, covered & ~part])
    # one colour everywhere comes back within 2 ulp
    q = np.float32([0.25, 0.5, 0.8123])
    one = net.export_mesh(str(tmp_path / "one"), bake_views=K, view_size=64, view_decoder=_constant_views([q.tolist()] * K, 128),
                          **kw)
    sel = (one["mask"] == 2) & (one["view_count"] > 0)
    assert torch.equal(one["view_count"], out["view_count"])
    got = one["view_rgb"].permute(1, 2, 0)[sel].cpu().numpy()
    assert _ulps(got, np.tile(q, (len(got), 1))).max() <= 2
    # the default decoder at the render size, and the argument checks
    same = net.export_mesh(str(tmp_path / "same"), bake_views=4, view_size=32, **kw)
    assert same["view_rgb"].shape == (3, R, R) and float(same["view_rgb"].min()) >= 0 and float(same["view_rgb"].max()) <= 1
    with pytest.raises(ValueError, match="texture_resolution"):
        net.export_mesh(str(tmp_path / "bad"), resolution=64, S=32, thresh=cfg.density_thresh, bake_views=4)
    with pytest.raises(ValueError, match="view_decoder"):
        net.export_mesh(str(tmp_path / "bad"), bake_views=4, view_size=32, view_decoder=lambda z: z[:, :2], **kw)


def test_sphere_is_covered_by_sixteen_views(dev):
    """NeRFRenderer.bake_views on the marching-cubes sphere of tests/test_gpu_uv_bake.py (r = 0.6, 32^3 lattice, the
    per-triangle atlas) with the export's cameras (16 Fibonacci views, radius 1.8, fovy 55 degrees, 64 x 64): at least
    99.5 % of the covered texels are seen by a view.  The fixture's own field is a random network, not a ball, so the
    sphere is meshed from an analytic volume.  Measured on the MI355X: 19 272 covered texels, 100.000 % seen, 3.67
    views per texel on average."""
    from src.latent_nerf.raymarching import marching_cubes
    from src.uv_atlas import atlas_min_resolution, per_triangle_atlas
    net, _ = _nerf(dev)
    a = torch.linspace(-1, 1, 32)
    X, Y, Z = torch.meshgrid(a, a, a, indexing="ij")
    vol = (0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).float().to(dev)
    v, f, _ = marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    vt, ft = per_triangle_atlas(f.shape[0], dev)
    R = atlas_min_resolution(f.shape[0])
    K, side = 16, 64
    cams = fibonacci_cameras(K, 1.8, 55.0, side, side, dev)
    q = torch.tensor([0.2, 0.4, 0.6], device=dev)
    images = q.view(1, 3, 1, 1).expand(K, 3, side, side).contiguous()
    fallback = torch.full((3, R, R), 0.5, device=dev)
    out = net.bake_views(v, f, vt, ft, images, cams, R, fallback=fallback)
    covered = out["mask"] == 2
    share = float((out["view_count"][covered] > 0).float().mean())
    print("sphere: %d covered texels, %.3f %% seen, mean views %.2f" % (int(covered.sum()), 100 * share,
                                                                          float(out["view_count"][covered].float().mean())))
    assert int(covered.sum()) > 5000 and share >= 0.995, share
    seen = covered & (out["view_count"] > 0)
    assert _ulps(out["rgb"].permute(1, 2, 0)[seen].cpu().numpy(), np.tile(q.cpu().numpy(), (int(seen.sum()), 1))).max() <= 2
    assert bool((out["rgb"][:, covered & ~seen] == 0.5).all())
    assert bool((out["view_weight"][seen] > 0).all()) and bool((out["view_weight"][~seen] == 0).all())
    assert int((out["mask"] == 1).sum()) > 0                                       # the gutter was dilated
    # cos_min = 0.95: a view then takes a cap of 18 degrees around its direction, 2.4 % of the sphere, so 16 views
    # leave texels that no view takes; they hold the fallback, the others the colour
    out = net.bake_views(v, f, vt, ft, images, cams, R, fallback=fallback, cos_min=0.95)
    seen = covered & (out["view_count"] > 0)
    unseen = covered & ~seen
    assert int(seen.sum()) > 500 and int(unseen.sum()) > int(seen.sum())
    assert bool((out["rgb"][:, unseen] == 0.5).all())
    assert _ulps(out["rgb"].permute(1, 2, 0)[seen].cpu().numpy(), np.tile(q.cpu().numpy(), (int(seen.sum()), 1))).max() <= 2


@pytest.mark.parametrize("decode_eval", [False, True])
def test_nerf_trainer_bakes_views_into_the_export(dev, tmp_path, decode_eval):
    """log.mesh_bake_views through Trainer.full_eval; with log.decode_eval the renders go through the guidance object's
    decoder (the synthetic guidance has none: decode_with then gives the linear preview at 8 x, so 32 -> 256)."""
    from PIL import Image

    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    flat = {"log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32, "render.eval_h": 32,
            "render.eval_w": 32, "render.grid_size": 32, "optim.iters": 4, "log.save_interval": 100,
            "log.eval_size": 1, "log.full_eval_size": 2, "optim.fp16": False, "guide.text": "a lego man",
            "log.exp_name": "t", "log.save_mesh": True, "log.mesh_texture_resolution": 256, "log.mesh_bake_views": 6,
            "log.mesh_bake_view_size": 32, "log.decode_eval": decode_eval}
    tr = Trainer(apply_overrides(TrainConfig(), flat), device=dev)
    tr.train()
    names = {p.name for p in (tr.exp_path / "mesh").iterdir()}
    assert {"mesh.obj", "mesh.mtl", "albedo.png", "albedo_preview.png", "latent_texture.pt"} <= names
    a = np.asarray(Image.open(tr.exp_path / "mesh" / "albedo.png"))
    b = np.asarray(Image.open(tr.exp_path / "mesh" / "albedo_preview.png"))
    assert a.shape == b.shape == (256, 256, 3)
    assert tr.nerf.training                                                        # the renders left the mode as it was


# ------------------------------------------------------------------------------ 5. Latent-Paint export
class _LinearGuidance:
    """A guidance stub whose decoder is the linear preview at the texture's own resolution."""

    def decode_latents(self, latents):
        from src.latent_nerf.training.guidance import linear_decode_latents
        return linear_decode_latents(latents, upsample=1)


def test_latent_paint_export_projects_its_renders(dev, tmp_path):
    from PIL import Image

    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    torch.manual_seed(3)
    flat = {"log.exp_name": "paint", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(SHAPES, "blub.obj"), "guide.texture_resolution": 128,
            "guide.texture_interpolation_mode": "bilinear", "render.eval_grid_size": 96}
    cfg = apply_overrides(TrainConfig(), flat).validate()
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=128)
    guidance = _LinearGuidance()
    plain = model.export_mesh(tmp_path / "plain", guidance=guidance)
    assert {p.name for p in (tmp_path / "plain").iterdir()} == {"albedo.png", "mesh.obj", "mesh.mtl"}
    preview = guidance.decode_latents(model.texture_img.detach())[0]
    want = (preview.permute(1, 2, 0).clamp(0, 1).cpu().numpy() * 255).astype(np.uint8)   # today's albedo.png
    assert np.array_equal(np.asarray(Image.open(tmp_path / "plain" / "albedo.png")), want)
    out = model.export_mesh(tmp_path / "views", guidance=guidance, bake_views=8)
    assert {p.name for p in (tmp_path / "views").iterdir()} == {"albedo.png", "albedo_preview.png", "mesh.obj", "mesh.mtl"}
    for name in ("mesh.obj", "mesh.mtl"):
        assert (tmp_path / "views" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes()
    assert (tmp_path / "views" / "albedo_preview.png").read_bytes() == (tmp_path / "plain" / "albedo.png").read_bytes()
    assert torch.equal(out["rgb"], preview) and torch.equal(plain["rgb"], preview)
    covered, seen = out["mask"] == 2, out["view_count"] > 0
    assert 0.5 < float(seen[covered].float().mean()) <= 1.0
    unseen = covered & ~seen
    assert torch.equal(out["view_rgb"][:, unseen], preview[:, unseen])
    # one view cannot see the fish's far side: those texels keep the decoded atlas
    single = model.export_mesh(tmp_path / "single", guidance=guidance, bake_views=1)
    far = covered & (single["view_count"] == 0)
    assert int(far.sum()) > 1000 and int((covered & ~far).sum()) > 1000
    assert torch.equal(single["view_rgb"][:, far], preview[:, far])
    # a seen texel is a weighted mean of bilinear samples whose four taps are all foreground pixels of the K renders:
    # per channel it lies between the least and the largest foreground pixel of those renders (rendered again here)
    from src.latent_nerf.raymarching import bake_view_poses
    poses = bake_view_poses(8)
    views = model.render_test([t for t, _ in poses], [p for _, p in poses], [cfg.render.radius_range[1] * 1.2] * 8,
                              decode_func=lambda _t: preview[None], dims=(96, 96))
    fg = views["mask"][:, 0] > 0.5
    pixels = views["image"].clamp(0, 1).permute(1, 0, 2, 3)[:, fg]                  # [3, foreground pixels]
    assert pixels.shape[1] > 5000
    got = out["view_rgb"][:, covered & seen]
    lo, hi = pixels.min(1).values, pixels.max(1).values
    assert bool((got >= lo[:, None] - 1e-5).all()) and bool((got <= hi[:, None] + 1e-5).all())
    img = np.asarray(Image.open(tmp_path / "views" / "albedo.png"))
    assert np.array_equal(img, (out["view_rgb"].permute(1, 2, 0).cpu().numpy() * 255).round().astype(np.uint8))
    with pytest.raises(ValueError, match="bake_views"):
        model.export_mesh(tmp_path / "bad", guidance=guidance, bake_views=-1)


def test_latent_paint_export_puts_the_renders_where_they_belong(dev, tmp_path):
    """The colours of the Latent-Paint bake against what they must be.  An icosphere (1280 faces, chart atlas, 256^2 RGB
    texture) is painted with its own surface position, colour = 0.5 + 0.6 (x - centre), so a projected colour decodes
    to the surface point it was taken from, and that point must be the texel's own up to the two resamplings:
      * a bilinear tap lies within sqrt(2) pixels of the texel's projection.  At 256^2, fov 60 degrees and depth <= 2.1
        a pixel is s <= 0.0095 wide; on the sphere (r = 0.6) a screen offset d moves the surface point from polar angle
        a (to the view axis) to asin(sin a + d / r), most when the tap sits on the limb: sin a = 1 - sqrt(2) s / r gives
        a = 77.9 degrees, 12.1 degrees of arc = 0.127 (a texel is accepted up to acos 0.2 = 78.5 degrees);
      * the texture lookup of the render: texel centres hold the exact colour and the colour is affine along a face,
        so the error is the gutter's, the mean of neighbours at most 2 texels (0.01 each, up to 1.7 x stretched at a
        chart's rim) away: 0.04.
    Bound: 0.2 (0.167 plus the facets' departure from the sphere).  A camera that looks at the wrong height (dy = 0.25),
    poses that differ between the renders and the records, swapped angles or a mirrored image are off by 0.25 to
    1.2.  Measured on the MI355X: 30 272 seen texels, largest displacement 0.0092, mean 0.0001 (the bilinear mix of
    the taps' points lands far closer than any single tap)."""
    from src.latent_nerf.raymarching import uv_dilate, uv_raster
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    v, f = _icosphere(3, 1.0)
    assert len(f) == 1280
    obj = tmp_path / "sphere.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in v) +
                   "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f))
    R = 256
    flat = {"log.exp_name": "sphere", "log.exp_root": str(tmp_path), "guide.text": "a ball", "guide.shape_path": str(obj),
            "guide.texture_resolution": R, "guide.texture_interpolation_mode": "bilinear", "guide.uv_atlas": "charts",
            "render.eval_grid_size": 256}
    cfg = apply_overrides(TrainConfig(), flat).validate()
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=False, texture_resolution=R)
    centre = torch.tensor([0.0, cfg.guide.dy, 0.0], device=dev)
    assert abs(float((model.mesh.vertices - centre).norm(dim=1).max()) - 0.6) < 1e-5
    texel_face, texel_idx, pos = uv_raster(model.mesh.vertices, model.mesh.faces, model.vt, model.ft, R)
    tex = torch.zeros(3, R * R, device=dev)
    tex[:, texel_idx.long()] = (0.5 + 0.6 * (pos - centre)).T
    mask = ((texel_face.reshape(-1) >= 0).to(torch.uint8) * 2).view(R, R)
    tex = tex.view(3, R, R).contiguous()
    uv_dilate(tex, mask, 4)
    with torch.no_grad():
        model.texture_img_rgb_finetune.copy_(tex[None])
    out = model.export_mesh(tmp_path / "views", bake_views=8)
    seen = (out["mask"] == 2) & (out["view_count"] > 0)
    assert float(seen[out["mask"] == 2].float().mean()) > 0.9
    where = (out["view_rgb"].reshape(3, -1)[:, texel_idx.long()].T - 0.5) / 0.6 + centre       # [P,3], decoded
    err = (where - pos).norm(dim=1)[seen.reshape(-1)[texel_idx.long()]]
    print("sphere paint: %d seen texels, displacement max %.4f mean %.4f" % (err.numel(), float(err.max()), float(err.mean())))
    assert float(err.max()) <= 0.2, float(err.max())


def test_latent_paint_trainer_passes_the_option(dev, tmp_path):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.training.trainer import Trainer
    flat = {"log.exp_name": "paint", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(SHAPES, "blub.obj"), "guide.texture_resolution": 64, "optim.iters": 1,
            "log.save_interval": 100, "log.eval_size": 1, "log.full_eval_size": 1, "render.eval_grid_size": 64,
            "log.save_mesh": True, "log.mesh_bake_views": 4}
    tr = Trainer(apply_overrides(TrainConfig(), flat).validate(), device=dev)
    tr.train()
    names = {p.name for p in (tr.exp_path / "mesh").iterdir()}
    assert {"mesh.obj", "mesh.mtl", "albedo.png", "albedo_preview.png"} <= names
