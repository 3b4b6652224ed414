"""Float64 torch restatement of csrc/meshshade.hip (contracts: include/lnerf_hip.h, "Shaded Latent-Paint renders"): smooth
vertex normals, and per pixel the interpolated unit normal, nine-term SH lighting and depth, with autograd supplying every
backward.  The discrete winners (`face_idx`) are an INPUT, as in tests/rastergrad_reference.py, whose pieces (projection,
barycentrics, lookup, antialiasing) the whole-chain cases reuse.  Every function takes the dtype of its inputs, so the same
code run in float32 measures the tolerance of a comparison.

    python -m tests.meshshade_reference      prints the tolerance constants of tests/test_gpu_meshshade.py
"""
import itertools
import math

import torch

from tests import rastergrad_reference as RG

DEFAULT_LIGHTS = (1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)
MIN_NORM, LIGHT_MIN, LIGHT_MAX = 1e-6, 1e-8, 1.0
SH0, SH1, SH2 = 0.28209479177387814, 0.4886025119029199, 1.0925484305920792
SH20, SH20C, SH22 = 0.94617469575755997, 0.31539156525251999, 0.5462742152960396


def randn(shape, seed):
    """RG.randn rounded to float32, so that the kernel (f32) and the reference (f64) read the same numbers."""
    return RG.randn(shape, seed).float().double()


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _unit(a, info=None, key="m"):
    """a / |a| where |a| >= 1e-6, else 0 (and no gradient)."""
    ss = _dot(a, a)
    live = ss.detach().sqrt() >= MIN_NORM
    m = torch.where(live, ss, torch.ones_like(ss)).sqrt()
    if info is not None:
        info[key] = ss.detach().sqrt()
    return torch.where(live[..., None], a / m[..., None], torch.zeros_like(a))


# ------------------------------------------------------------------------------------------------ vertex normals
def corner_table_loop(faces, n_verts):
    """(corner_start, corner_list) as Python lists, by the definition: vertex i owns its corners c = 3 f + k, ascending."""
    own = [[] for _ in range(n_verts)]
    flat = [int(v) for v in faces.reshape(-1)]
    for c, v in enumerate(flat):
        if 0 <= v < n_verts:
            own[v].append(c)
    start, corners = [0], []
    for lst in own:
        corners += lst
        start.append(len(corners))
    return start, corners + [-1] * (len(flat) - len(corners))


def face_normals(verts, faces, info=None):
    """-> (n [F,3], ok [F]): unit normals; ok is False for a vertex id outside [0, V), a zero or a non-finite length."""
    V = verts.shape[0]
    faces = faces.long()
    in_range = ((faces >= 0) & (faces < V)).all(1)
    f = torch.where(in_range[:, None], faces, torch.zeros_like(faces))
    p0, p1, p2 = verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]]
    c = torch.linalg.cross(p1 - p0, p2 - p0)
    l_raw = _dot(c, c).detach().sqrt()
    ok = in_range & (l_raw > 0) & torch.isfinite(l_raw)
    l = torch.where(ok, _dot(c, c), torch.ones_like(l_raw)).sqrt()
    if info is not None:
        info["l"] = l_raw[in_range]
    return torch.where(ok[:, None], c / l[:, None], torch.zeros_like(c)), ok


def vertex_normals(verts, faces, info=None):
    """verts [V,3], faces [F,3] -> vn [V,3]: s_i = the sum of the unit normals of i's faces, vn_i = s_i / |s_i|."""
    n, ok = face_normals(verts, faces, info)
    idx = faces.long()[ok].reshape(-1)
    s = torch.zeros_like(verts).index_add(0, idx, n[ok].repeat_interleave(3, 0))
    return _unit(s, info, "m_vertex")


# ------------------------------------------------------------------------------------------------ pixel shading
def sh_basis(n):
    x, y, z = n[..., 0], n[..., 1], n[..., 2]
    return [SH0 * torch.ones_like(x), -SH1 * y, SH1 * z, -SH1 * x, SH2 * x * y, -SH2 * y * z, SH20 * z * z - SH20C,
            -SH2 * x * z, SH22 * (x * x - y * y)]


def shade(face_idx, bary, face_z, faces, vnormals, lights, H, W, info=None):
    """-> (normal [P,3], lighting [P], depth [P]), 0 on background.  lights [B,9]."""
    B, F, V = face_z.shape[0], face_z.shape[1], vnormals.shape[0]
    faces = faces.long()
    fg = (face_idx >= 0) & (face_idx < F)
    f = torch.where(fg, face_idx, torch.zeros_like(face_idx)).long()
    vid = faces[f]
    fg = fg & ((vid >= 0) & (vid < V)).all(1)
    vn = vnormals[torch.where(fg[:, None], vid, torch.zeros_like(vid))]          # [P,3,3]
    view = torch.arange(B).repeat_interleave(H * W)
    a = (bary[:, 0:1] * vn[:, 0] + bary[:, 1:2] * vn[:, 1]) + bary[:, 2:3] * vn[:, 2]
    a = torch.where(fg[:, None], a, torch.ones_like(a))
    n = _unit(a, info, "m_pixel")
    z = face_z[view, f]
    depth = -((bary[:, 0] * z[:, 0] + bary[:, 1] * z[:, 1]) + bary[:, 2] * z[:, 2])
    L = lights[view]
    acc = 0
    for k, y in enumerate(sh_basis(n)):
        acc = acc + L[:, k] * y
    lighting = acc.clamp(LIGHT_MIN, LIGHT_MAX)
    if info is not None:
        info.update(fg=fg, unclamped=acc.detach())
    zero = torch.zeros_like(depth)
    return torch.where(fg[:, None], n, torch.zeros_like(n)), torch.where(fg, lighting, zero), torch.where(fg, depth, zero)


# ------------------------------------------------------------------------------------------------ the whole chain
def shaded_chain(verts, faces, cams, face_idx, face_uv, tex, lights, H, W, antialias=True, extra=None):
    """vertices -> (image [B,H,W,C+1], normal [B,H,W,3], lighting [B,H,W], depth [B,H,W]): RG.render_chain's composition
    with the colour multiplied by the lighting before the mask is appended and the edges are antialiased."""
    B = cams.shape[0]
    face_xy, face_z = RG.prepare(verts, faces, cams)
    b = RG.bary(face_idx, face_xy, face_z, H, W)
    uv = RG.interpolate(face_idx, b, face_uv)
    col = RG.texture_lookup(tex, uv, face_idx)
    normal, lighting, depth = shade(face_idx, b, face_z, faces, vertex_normals(verts, faces, extra), lights, H, W, extra)
    mask = ((face_idx >= 0) & (face_idx < faces.shape[0])).to(col.dtype)[:, None]
    img = torch.cat([col * mask * lighting[:, None], mask], -1).reshape(B, H, W, -1)
    if extra is not None:
        extra.update(bary=b, uv=uv)
    if antialias:
        img = RG.antialias(img, face_idx, b, face_xy, face_z, faces, info=extra)
    return img, normal.reshape(B, H, W, 3), lighting.reshape(B, H, W), depth.reshape(B, H, W)


# ------------------------------------------------------------------------------------------------ the shared scenes
def _sphere(subdiv):
    from src.latent_nerf.training.shape import make_icosphere
    v, f = make_icosphere(subdiv, 1.0)
    return v.double(), f


def write_sphere_obj(path, subdiv=1):
    """make_icosphere(subdiv) as a Wavefront file for the model tests -> str(path)."""
    v, f = _sphere(subdiv)
    with open(path, "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(p.tolist()) for p in v))
        fh.write("".join("f %d %d %d\n" % tuple((t + 1).tolist()) for t in f))
    return str(path)


def fan_mesh():
    """An open fan of 6 faces around vertex 0 (rim 1..7: 1 and 7 are boundary vertices with one face each), not flat."""
    rim = [[math.cos(0.7 * k), math.sin(0.7 * k), 0.125 * ((3 * k) % 5) - 0.25] for k in range(7)]
    verts = torch.tensor([[0.0, 0.0, 0.375]] + rim, dtype=torch.float64)
    verts = (verts * 64).round() / 64
    return verts, torch.tensor([[0, k, k + 1] for k in range(1, 7)])


def fan_edge_mesh():
    """The fan plus every edge case, V = 15: vertex 8 in no face; face 6 = (9, 10, 11) collinear (zero area); face 7 =
    (3, 4, 15) with a vertex id == V; faces 8, 9 = (12, 13, 14) and (12, 14, 13), opposite, so s = 0 at their vertices.
    -> verts, faces, zero (the vertices whose normal and gradient are exactly 0)."""
    verts, faces = fan_mesh()
    more = torch.tensor([[2.0, 2.0, 2.0], [0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [2.0, 0.0, 1.0],
                         [3.0, 0.25, 0.5], [3.5, 1.0, 0.75], [2.75, 0.5, 1.5]], dtype=torch.float64)
    faces = torch.cat([faces, torch.tensor([[9, 10, 11], [3, 4, 15], [12, 13, 14], [12, 14, 13]])])
    return torch.cat([verts, more]), faces, [8, 9, 10, 11, 12, 13, 14]


def normal_meshes():
    """{name: (verts f64 [V,3], faces [F,3])} of the vertex-normal comparisons."""
    g = torch.Generator().manual_seed(41)
    big_v, big_f = _sphere(3)                                   # 642 / 1280: three groups of 256, the last partial
    big_v = (big_v + (torch.randint(-8, 9, big_v.shape, generator=g).double() / 512.0)).float().double()
    small_v, small_f = _sphere(1)
    return {"tetra": (torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, -0.5], [-0.5, 0.75, -0.5], [-0.5, -0.875, -0.25]],
                                   dtype=torch.float64), RG.TETRA_FACES.clone()),
            "fan": fan_mesh(), "ico1": (small_v, small_f), "ico3": (big_v, big_f), "fan_edges": fan_edge_mesh()[:2]}


def unit_normals(V, seed=43):
    n = randn((V, 3), seed)
    return (n / n.norm(dim=1, keepdim=True)).float().double()


def scene_lights(dtype=torch.float64):
    """Per view: the default lights in view 0, twice the default in view 1."""
    row = torch.tensor(DEFAULT_LIGHTS, dtype=dtype)
    return torch.stack([row, 2 * row])


def pixel_scene(H, W, face_idx=None):
    """RG.screen_scene() at (H, W) with random unit vertex normals on its 19 vertex ids and scene_lights().  face_idx:
    the winners (default: the f32 oracle's).  The barycentrics are the reference's, rounded to f32: what the kernel reads."""
    fxy, fz, faces = RG.screen_scene()
    idx = RG.oracle_face_idx(fxy, fz, H, W) if face_idx is None else face_idx
    bary = RG.bary(idx, fxy, fz, H, W).float().double()
    P = idx.shape[0]
    return dict(H=H, W=W, faces=faces, idx=idx, bary=bary, fz=fz, vn=unit_normals(19), lights=scene_lights(),
                gn=randn((P, 3), 44), gl=randn((P,), 45), gd=randn((P,), 46))


# (elev, azim, radius): two views that put no decision of the scene on a rounding edge (tests/test_meshshade_cpu.py asserts it)
SPHERE_VIEWS = [(1.27, 0.26, 2.23), (1.94, 1.84, 2.4)]
SPHERE_SIDE = 16
COMBOS = [c for c in itertools.product((1, 0), repeat=3) if any(c)]   # which of (grad_normal, grad_lighting, grad_depth)


def sphere_scene(constant_texture=False, dtype=torch.float64):
    """make_icosphere(1) seen by two of the trainer's cameras at 16 x 16, planar UVs inside (0, 1), a 4 x 16 x 16 texture
    (or the constant 0.625).  -> verts, faces, cams [B,14], face_uv [F,3,2], tex, lights [B,9]."""
    from src.latent_paint.models.render import Renderer
    verts, faces = _sphere(1)
    cams = torch.tensor([list(Renderer.get_camera_from_view(t, p, r, 0.0)) for t, p, r in SPHERE_VIEWS],
                        dtype=torch.float32)
    vt = torch.stack([0.5 + 0.390625 * verts[:, 0] + 0.046875 * verts[:, 2],
                      0.5 + 0.421875 * verts[:, 1] + 0.046875 * verts[:, 2]], -1)
    g = torch.Generator().manual_seed(47)
    tex = torch.randint(-16, 17, (4, 16, 16), generator=g).to(dtype) / 8.0
    if constant_texture:
        tex = torch.full_like(tex, 0.625)
    lights = torch.tensor([DEFAULT_LIGHTS, DEFAULT_LIGHTS], dtype=dtype)
    return verts.to(dtype), faces, cams.to(dtype), vt[faces].to(dtype), tex, lights


def sphere_weights(C):
    S = SPHERE_SIDE
    return randn((2, S, S, C), 48), randn((2, S, S, 3), 49), randn((2, S, S), 50)


# ------------------------------------------------------------------------------------------------ the compared cases
def case_vnormals(faces):
    """-> fn(verts, grad_vnormals) -> (vnormals, grad_verts)."""
    def fn(verts, gvn):
        verts = verts.requires_grad_()
        vn = vertex_normals(verts, faces)
        return (vn.detach(), *RG._grads([vn], [gvn], [verts]))
    return fn


def case_shade(face_idx, faces, H, W, combo=(1, 1, 1)):
    """-> fn(vnormals, bary, face_z, lights, gn, gl, gd) -> (normal, lighting, depth, grad_bary, grad_vnormals, grad_face_z)
    under the incoming gradients `combo` selects (the others are absent: NULL in the kernel's call)."""
    def fn(vn, bary, fz, lights, gn, gl, gd):
        vn, bary, fz = vn.requires_grad_(), bary.requires_grad_(), fz.requires_grad_()
        outs = shade(face_idx, bary, fz, faces, vn, lights, H, W)
        used = [(o, g) for o, g, on in zip(outs, (gn, gl, gd), combo) if on]
        grads = RG._grads([o for o, _ in used], [g for _, g in used], [bary, vn, fz])
        return (*[o.detach() for o in outs], *grads)
    return fn


def case_sphere(face_idx, faces, antialias, parts=(1, 1, 1)):
    """-> fn(verts, cams, face_uv, tex, lights, w1, w2, w3) -> (image, normal, lighting, depth, grad_verts) of the loss
    sum(w1 image) + sum(w2 normal) + sum(w3 depth), image = the shaded (colour * lighting, mask) render."""
    S = SPHERE_SIDE

    def fn(verts, cams, face_uv, tex, lights, w1, w2, w3):
        verts = verts.requires_grad_()
        img, normal, lighting, depth = shaded_chain(verts, faces, cams, face_idx, face_uv, tex, lights, S, S, antialias)
        used = [(o, w) for o, w, on in zip((img, normal, depth), (w1, w2, w3), parts) if on]
        (gv,) = RG._grads([o for o, _ in used], [w for _, w in used], [verts])
        return img.detach(), normal.detach(), lighting.detach(), depth.detach(), gv
    return fn


def sphere_winners(verts, faces, cams):
    fxy, fz = RG.prepare(verts, faces, cams)
    return RG.oracle_face_idx(fxy, fz, SPHERE_SIDE, SPHERE_SIDE)


def interior_vertices(face_idx, faces, n_verts, n_views=2, keep=None):
    """The vertices away from every silhouette in some view: all their faces win a pixel of that view -> list of ids.
    keep [P] bool: a face with a pixel where it is False counts as not drawn in that view (e.g. a clamped lighting)."""
    faces = faces.long()
    inner = torch.zeros(n_verts, dtype=torch.bool)
    keep = torch.ones_like(face_idx, dtype=torch.bool) if keep is None else keep
    for idx, ok in zip(face_idx.reshape(n_views, -1), keep.reshape(n_views, -1)):
        drawn = torch.zeros(faces.shape[0], dtype=torch.bool)
        drawn[idx[idx >= 0].long()] = True
        drawn[idx[(idx >= 0) & ~ok].long()] = False
        hidden = torch.zeros(n_verts, dtype=torch.bool)
        hidden[faces[~drawn].reshape(-1)] = True
        inner |= ~hidden
    return torch.nonzero(inner).reshape(-1).tolist()


def measured_deviations():
    """{case name: [relative f32-vs-f64 deviation per output]} on the tests' own inputs, winners from the f32 oracle."""
    rows = {}
    for name, (verts, faces) in normal_meshes().items():
        rows["vnormals_" + name] = RG.deviation(case_vnormals(faces), [verts, randn(tuple(verts.shape), 42)])
    for H, W in RG.SIZES:
        s = pixel_scene(H, W)
        for combo in COMBOS:
            key = "shade_%d%d%d_%dx%d" % (*combo, H, W)
            rows[key] = RG.deviation(case_shade(s["idx"], s["faces"], H, W, combo),
                                     [s["vn"], s["bary"], s["fz"], s["lights"], s["gn"], s["gl"], s["gd"]])
    for name, constant, antialias, parts in (("sphere_chain", False, True, (1, 1, 1)), ("sphere_reason", True, False, (1, 0, 0))):
        verts, faces, cams, face_uv, tex, lights = sphere_scene(constant)
        idx = sphere_winners(verts, faces, cams)
        rows[name] = RG.deviation(case_sphere(idx, faces, antialias, parts),
                                  [verts, cams, face_uv, tex, lights, *sphere_weights(tex.shape[0] + 1)])
    return rows


if __name__ == "__main__":
    print("REL = {")
    for name, devs in measured_deviations().items():
        print("    %r: (%s)," % (name, ", ".join("%.3g" % d for d in devs) + ("," if len(devs) == 1 else "")))
    print("}")
