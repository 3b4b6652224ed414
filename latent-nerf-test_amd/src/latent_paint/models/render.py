"""HIP-backed counterpart of src/latent_paint/models/render.py (Renderer :5-69): same constructor, camera
convention (:19-31) and the two render entry points (:34-47, :50-69), with the kaolin calls replaced by the
C-ABI raster kernels (csrc/raster.hip).  `render_views` / `render_views_texture` take B views per call (the fork's
`render.batch_size`); the single-view methods are their B = 1 case, on the one tile-culled rasteriser.
`interpolation_mode="mipmap"` is this project's own: the trilinear mip-mapped lookup of csrc/texmip.hip, for renders much
smaller than their texture; with `mip_coverage` its pyramid is the coverage-weighted one of the same file, which keeps the
texels no face covers out of every level.  Also this project's own: `verts` that require grad receive the image's gradient
(csrc/rastergrad.hip: the transposes of projection, barycentrics, interpolation and the bilinear lookup), and
`antialias_views` makes silhouettes differentiable; with plain vertices every call is what it was.  `shade_views`
(csrc/meshshade.hip) adds what the fork's live trainer renders beside the image: smooth vertex normals interpolated per
pixel, nine-term spherical-harmonic lighting and depth, differentiable w.r.t. the vertices like the image."""
import math

import torch

from ...latent_nerf.raymarching import backend as _b
from ...latent_nerf.raymarching.raymarching import (RasterState, _chk, _p, _stream, mip_build, mip_levels,  # noqa: F401
                                                    mip_texels, mipcov_weights, pyramid_build, pyramid_fold,
                                                    raster_cover, raster_project, rasterize_views, uv_dilate, uv_raster)

_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}   # lnerf_texture_map_*'s point lookups ("mipmap": _TextureMip)


def _texture_shape(tex):
    """(C, R) of the one square [1,C,R,R] texture the lookup kernels read."""
    if tex.dim() != 4 or tex.shape[0] != 1 or tex.shape[2] != tex.shape[3]:
        raise ValueError("texture_map: texture must be [1,C,R,R] (got %s)" % (tuple(tex.shape),))
    return tex.shape[1], tex.shape[2]


class _InterpAttr(torch.autograd.Function):
    """feat = sum_k bary_k attr_k.  The attributes' gradient always; the barycentrics' (lnerf_interpolate_attributes_
    backward_bary) only when they are part of a graph, i.e. the vertices are being learned."""

    @staticmethod
    def forward(ctx, attr, face_idx, bary):
        P, D = face_idx.shape[0], attr.shape[-1]
        attr = attr.contiguous()
        feat = torch.empty(P, D, device=attr.device)
        _b.call("lnerf_interpolate_attributes", _p(face_idx), _p(bary), _chk(attr, "attr"), P, D, _p(feat), _stream())
        ctx.save_for_backward(face_idx, bary, attr if ctx.needs_input_grad[2] else None)
        ctx.shape = attr.shape
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        face_idx, bary, attr = ctx.saved_tensors
        dfeat = dfeat.contiguous()
        P, D = face_idx.shape[0], ctx.shape[-1]
        dattr = dbary = None
        if ctx.needs_input_grad[0]:
            dattr = torch.zeros(ctx.shape, device=dfeat.device)
            _b.call("lnerf_interpolate_attributes_backward", _p(face_idx), _p(bary), _chk(dfeat, "dfeat"), P, D,
                    _p(dattr), _stream())
        if ctx.needs_input_grad[2]:
            dbary = torch.empty(P, 3, device=dfeat.device)
            _b.call("lnerf_interpolate_attributes_backward_bary", _p(face_idx), _p(attr), _chk(dfeat, "dfeat"), P, D,
                    attr.numel() // (3 * D), _p(dbary), _stream())
        return dattr, None, dbary


class _TextureMap(torch.autograd.Function):
    """The point lookups.  The texture's gradient always; the UVs' (lnerf_texture_map_backward_uv, bilinear only) when
    they are part of a graph."""

    @staticmethod
    def forward(ctx, tex, uv, face_idx, mode):
        C, R = _texture_shape(tex)
        P = uv.shape[0]
        tex = tex.contiguous()
        out = torch.empty(P, C, device=tex.device)
        _b.call("lnerf_texture_map_forward", _chk(uv, "uv"), _p(face_idx), _chk(tex, "texture"), P, C, R, mode, _p(out),
                _stream())
        ctx.save_for_backward(uv, face_idx, tex if ctx.needs_input_grad[1] else None)
        ctx.meta = (tex.shape, mode)
        return out

    @staticmethod
    def backward(ctx, dout):
        uv, face_idx, tex = ctx.saved_tensors
        shape, mode = ctx.meta
        dout = dout.contiguous()
        dtex = duv = None
        if ctx.needs_input_grad[0]:
            dtex = torch.zeros(shape, device=dout.device)
            _b.call("lnerf_texture_map_backward", _p(uv), _p(face_idx), _chk(dout, "dout"), uv.shape[0], shape[1],
                    shape[2], mode, _p(dtex), _stream())
        if ctx.needs_input_grad[1]:
            if mode != _MODES["bilinear"]:
                raise ValueError("texture_map: the UV gradient exists for the bilinear lookup only")
            duv = torch.empty_like(uv)
            _b.call("lnerf_texture_map_backward_uv", _p(uv), _p(face_idx), _p(tex), _chk(dout, "dout"), uv.shape[0],
                    shape[1], shape[2], _p(duv), _stream())
        return dtex, duv, None, None


# ---- the geometry half of the backward pass (csrc/rastergrad.hip): vertices -> projected faces -> barycentrics
class _PrepareBatch(torch.autograd.Function):
    """lnerf_raster_prepare_batch with its transpose: verts [V,3] -> (face_z [B,F,3], face_xy [B,F,3,2], face_box)."""

    @staticmethod
    def forward(ctx, verts, faces32, cams, H, W):
        face_z, face_xy, face_box = raster_project(verts, faces32, cams, H, W)
        ctx.save_for_backward(verts, faces32, cams)
        ctx.mark_non_differentiable(face_box)
        return face_z, face_xy, face_box

    @staticmethod
    def backward(ctx, dz, dxy, _dbox):
        verts, faces32, cams = ctx.saved_tensors
        B, F = cams.shape[0], faces32.shape[0]
        dz = torch.zeros(B, F, 3, device=verts.device) if dz is None else dz.contiguous()
        dxy = torch.zeros(B, F, 3, 2, device=verts.device) if dxy is None else dxy.contiguous()
        dverts = torch.empty_like(verts)
        _b.call("lnerf_raster_prepare_batch_backward", _chk(dxy, "grad_face_xy"), _chk(dz, "grad_face_z"), _p(verts),
                verts.shape[0], _p(faces32), F, _p(cams), B, _p(dverts), _stream())
        return dverts, None, None, None, None


class _RasterizeBatch(torch.autograd.Function):
    """lnerf_rasterize_batch; the winners are discrete, the barycentrics carry lnerf_raster_bary_backward."""

    @staticmethod
    def forward(ctx, face_z, face_xy, face_box, H, W):
        face_idx, bary = raster_cover(face_z, face_xy, face_box, H, W)
        ctx.save_for_backward(face_z, face_xy, face_idx)
        ctx.dims = (face_z.shape[0], H, W, face_z.shape[1])
        ctx.mark_non_differentiable(face_idx)
        return face_idx, bary

    @staticmethod
    def backward(ctx, _didx, dbary):
        face_z, face_xy, face_idx = ctx.saved_tensors
        B, H, W, F = ctx.dims
        dz, dxy = torch.zeros_like(face_z), torch.zeros_like(face_xy)
        if dbary is not None:
            _b.call("lnerf_raster_bary_backward", _chk(dbary.contiguous(), "grad_bary"), _p(face_idx), _p(face_xy),
                    _p(face_z), B, H, W, F, _p(dxy), _p(dz), _stream())
        return dz, dxy, None, None, None


class _Antialias(torch.autograd.Function):
    """lnerf_raster_antialias_forward / _backward on image [B,H,W,C]."""

    @staticmethod
    def forward(ctx, image, face_xy, face_idx, bary, face_z, faces32):
        B, H, W, C = image.shape
        F = faces32.shape[0]
        image = image.contiguous()
        out = torch.empty_like(image)
        _b.call("lnerf_raster_antialias_forward", _chk(image, "image"), _chk(face_idx, "face_idx", torch.int32),
                _chk(bary, "bary"), _chk(face_xy, "face_xy"), _chk(face_z, "face_z"),
                _chk(faces32, "faces", torch.int32), B, H, W, C, F, _p(out), _stream())
        ctx.save_for_backward(image, face_xy, face_idx, bary, face_z, faces32)
        return out

    @staticmethod
    def backward(ctx, dout):
        image, face_xy, face_idx, bary, face_z, faces32 = ctx.saved_tensors
        B, H, W, C = image.shape
        dimage = torch.empty_like(image)
        dxy = torch.zeros_like(face_xy)
        _b.call("lnerf_raster_antialias_backward", _chk(dout.contiguous(), "grad_out"), _p(image), _p(face_idx), _p(bary),
                _p(face_xy), _p(face_z), _p(faces32), B, H, W, C, faces32.shape[0], _p(dimage), _p(dxy), _stream())
        return dimage, dxy, None, None, None, None


# ---- shading (csrc/meshshade.hip): vertices -> smooth vertex normals -> per pixel normal, SH lighting and depth
DEFAULT_LIGHTS = (1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)   # the fork's nine SH coefficients: 0.2821 + 0.4886 (n_z - n_x)


def check_lights(lights, what):
    """Nine finite floats -> a tuple of them; anything else raises ValueError naming `what`."""
    try:
        vals = tuple(float(v) for v in lights)
    except (TypeError, ValueError):
        vals = ()
    if len(vals) != 9 or not all(math.isfinite(v) for v in vals):
        raise ValueError("%s must be nine finite floats, the SH coefficients of l = 0, 1, 2 (got %r)" % (what, lights))
    return vals


def corner_table(faces, n_verts):
    """The corners of every vertex -> (corner_start [V+1], corner_list [3F]) int32 on faces' device, the table
    lnerf_vertex_normals_* gather over: corner id c = 3 f + k, vertex i owns corner_list[corner_start[i]:corner_start[i+1]],
    ascending (a stable sort of faces.flatten()).  Corners whose vertex id lies outside [0, n_verts) are in no list; the
    tail of corner_list they leave is -1."""
    flat = faces.reshape(-1).long()
    valid = (flat >= 0) & (flat < n_verts)
    order = torch.sort(flat, stable=True).indices
    order = order[valid[order]]
    start = torch.zeros(n_verts + 1, dtype=torch.int64, device=faces.device)
    start[1:] = torch.cumsum(torch.bincount(flat[valid], minlength=n_verts), 0)
    corners = torch.full((flat.numel(),), -1, dtype=torch.int32, device=faces.device)
    corners[:order.numel()] = order.to(torch.int32)
    return start.to(torch.int32).contiguous(), corners


def vertex_normals(verts, faces32, corner_start, corner_list):
    """lnerf_vertex_normals_forward -> [V,3]: unit sums of the unit normals of every vertex's faces (0 where they cancel)."""
    vn = torch.empty_like(verts)
    _b.call("lnerf_vertex_normals_forward", _chk(verts, "verts"), verts.shape[0], _chk(faces32, "faces", torch.int32),
            faces32.shape[0], _chk(corner_start, "corner_start", torch.int32), _chk(corner_list, "corner_list", torch.int32),
            _p(vn), _stream())
    return vn


def shade_pixels(vnormals, bary, face_z, face_idx, faces32, lights, B, H, W):
    """lnerf_raster_shade_forward -> (normal [B*H*W,3], lighting [B*H*W], depth [B*H*W]), 0 on background."""
    P, dev = B * H * W, vnormals.device
    normal, lighting, depth = torch.empty(P, 3, device=dev), torch.empty(P, device=dev), torch.empty(P, device=dev)
    _b.call("lnerf_raster_shade_forward", _chk(face_idx, "face_idx", torch.int32), _chk(bary, "bary"),
            _chk(face_z, "face_z"), _chk(faces32, "faces", torch.int32), _chk(vnormals, "vnormals"), _chk(lights, "lights"),
            B, H, W, faces32.shape[0], vnormals.shape[0], _p(normal), _p(lighting), _p(depth), _stream())
    return normal, lighting, depth


class _VertexNormals(torch.autograd.Function):
    """lnerf_vertex_normals_forward / _backward over verts [V,3]."""

    @staticmethod
    def forward(ctx, verts, faces32, corner_start, corner_list):
        ctx.save_for_backward(verts, faces32, corner_start, corner_list)
        return vertex_normals(verts, faces32, corner_start, corner_list)

    @staticmethod
    def backward(ctx, dvn):
        verts, faces32, corner_start, corner_list = ctx.saved_tensors
        V, F = verts.shape[0], faces32.shape[0]
        nbytes = _b.get_lib().lnerf_vertex_normals_scratch_bytes(V, F)
        scratch = torch.empty(max(nbytes, 16), device=verts.device, dtype=torch.uint8)
        dverts = torch.empty_like(verts)
        _b.call("lnerf_vertex_normals_backward", _chk(dvn.contiguous(), "grad_vnormals"), _p(verts), V, _p(faces32), F,
                _p(corner_start), _p(corner_list), _p(scratch), nbytes, _p(dverts), _stream())
        return dverts, None, None, None


class _ShadePixels(torch.autograd.Function):
    """lnerf_raster_shade_forward / _backward over (vnormals, bary, face_z): grad_bary goes on to _RasterizeBatch,
    grad_face_z to _PrepareBatch, grad_vnormals to _VertexNormals.  An output no loss uses hands the kernel a NULL."""

    @staticmethod
    def forward(ctx, vnormals, bary, face_z, face_idx, faces32, lights, B, H, W):
        ctx.save_for_backward(vnormals, bary, face_z, face_idx, faces32, lights)
        ctx.dims = (B, H, W)
        ctx.set_materialize_grads(False)
        return shade_pixels(vnormals, bary, face_z, face_idx, faces32, lights, B, H, W)

    @staticmethod
    def backward(ctx, dnormal, dlighting, ddepth):
        vnormals, bary, face_z, face_idx, faces32, lights = ctx.saved_tensors
        if dnormal is None and dlighting is None and ddepth is None:
            return (None,) * 9
        B, H, W = ctx.dims
        grads = [None if g is None else g.contiguous() for g in (dnormal, dlighting, ddepth)]
        dbary = torch.empty_like(bary)
        dvn, dz = torch.zeros_like(vnormals), torch.zeros_like(face_z)
        _b.call("lnerf_raster_shade_backward", *[_chk(g, "grad", allow_none=True) for g in grads], _p(face_idx), _p(bary),
                _p(face_z), _p(faces32), _p(vnormals), _p(lights), B, H, W, faces32.shape[0], vnormals.shape[0],
                _p(dbary), _p(dvn), _p(dz), _stream())
        return (dvn, dbary, dz) + (None,) * 6


class _Umbrella(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, faces32):
        ctx.save_for_backward(faces32)
        return _umbrella(x, faces32, False)

    @staticmethod
    def backward(ctx, dy):
        return _umbrella(dy, ctx.saved_tensors[0], True), None


def _umbrella(x, faces32, transpose):
    x = x.float().contiguous()
    V, F = x.shape[0], faces32.shape[0]
    nbytes = _b.get_lib().lnerf_mesh_umbrella_scratch_bytes(V, F)
    scratch = torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)
    out = torch.empty_like(x)
    _b.call("lnerf_mesh_umbrella", _chk(x, "x"), V, _chk(faces32, "faces", torch.int32), F, int(bool(transpose)),
            _p(scratch), nbytes, _p(out), _stream())
    return out


def mesh_umbrella(x, faces):
    """The face-weighted uniform Laplacian of x [V,3] on the mesh `faces` [F,3] (lnerf_mesh_umbrella):
    (L x)_i = x_i - (1 / (2 n_i)) sum over the faces (i,j,k) of (x_j + x_k), n_i the faces at i; a vertex in no face keeps
    x_i.  Differentiable w.r.t. x: the backward is the same call with the transpose flag.  No dense matrix."""
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError("mesh_umbrella: x must be [V,3] (got %s)" % (tuple(x.shape),))
    return _Umbrella.apply(x, faces.to(x.device).to(torch.int32).contiguous())


def _learns(verts):
    """The vertices are part of a graph that is being recorded: the render then carries their gradient."""
    return torch.is_grad_enabled() and verts.requires_grad


def uv_footprint(face_idx, face_xy, face_z, face_uv, B, H, W):
    """rho [B*H*W]: the longer screen-space UV derivative per one-pixel step, in UV units (lnerf_uv_footprint)."""
    F = face_uv.shape[0]
    rho = torch.empty(B * H * W, device=face_idx.device)
    _b.call("lnerf_uv_footprint", _chk(face_idx, "face_idx", torch.int32), _chk(face_xy, "face_xy"), _chk(face_z, "face_z"),
            _chk(face_uv, "face_uv"), B, H, W, F, _p(rho), _stream())
    return rho


def mip_lookup(tex, pyr, uv, rho, face_idx, L, bias, w0=None, wpyr=None):
    """The trilinear lookup -> [P,C]: lnerf_texture_mip_forward on mip_build's levels, or, given the weights w0 [R,R]
    and wpyr [S], the normalised lnerf_texture_mipcov_forward on mipcov_pull's."""
    C, R, P = tex.shape[0], tex.shape[1], uv.shape[0]
    out = torch.empty(P, C, device=tex.device)
    head = (_chk(uv, "uv"), _chk(rho, "rho"), _p(face_idx), _chk(tex, "texture"), _p(pyr))
    tail = (P, C, R, L, float(bias), _p(out), _stream())
    if w0 is None:
        _b.call("lnerf_texture_mip_forward", *head, *tail)
    else:
        _b.call("lnerf_texture_mipcov_forward", *head, _chk(w0, "w0"), _p(wpyr), *tail)
    return out


def mip_lookup_backward(dout, shape, uv, rho, face_idx, L, bias, w0=None, wpyr=None):
    """dout [P,C] -> the gradient of the [C,R,R] texture: the atomics of lnerf_texture_mip_backward (given the weights,
    lnerf_texture_mipcov_backward) into level 0 and a packed gradient pyramid, which pyramid_fold then folds into level 0."""
    C, R = shape
    dtex = torch.zeros(C, R, R, device=dout.device)
    dpyr = torch.zeros(C, mip_texels(R, L), device=dout.device) if L > 0 else None
    head = (_p(uv), _p(rho), _p(face_idx), _chk(dout, "dout"))
    tail = (uv.shape[0], C, R, L, float(bias), _p(dtex), _p(dpyr), _stream())
    if w0 is None:
        _b.call("lnerf_texture_mip_backward", *head, *tail)
    else:
        _b.call("lnerf_texture_mipcov_backward", *head, _chk(w0, "w0"), _p(wpyr), *tail)
    return pyramid_fold(dpyr, dtex, L, w0, wpyr)


def texture_coverage(verts, faces, face_uv, R, ring=1):
    """The texels of an R x R texture that belong to the surface -> bool [R,R]: the texels whose centre a face covers
    (uv_raster's texel_face >= 0), grown by `ring` rounds of uv_dilate's mask.  A bilinear tap reads one texel beyond a
    chart's edge, so with ring >= 1 those texels count as parameters too.  face_uv [F,3,2]: per-face-vertex UVs."""
    R = int(R)
    if R > _b.UV_MAX_RES:
        raise ValueError("texture_mip_coverage: a texture side of %d is above LNERF_UV_MAX_RES = %d, the largest atlas "
                         "uv_raster covers" % (R, _b.UV_MAX_RES))
    F = face_uv.shape[0]
    ft = torch.arange(3 * F, device=face_uv.device, dtype=torch.int32).reshape(F, 3)
    texel_face, _, _ = uv_raster(verts.float().contiguous(), faces, face_uv.reshape(-1, 2).float().contiguous(), ft, R)
    mask = (texel_face >= 0).to(torch.uint8) * 2
    uv_dilate(torch.zeros(1, R, R, device=mask.device), mask, int(ring))
    return mask > 0


class _TextureMip(torch.autograd.Function):
    """Footprint, pyramid and trilinear lookup of one render call; the backward returns the texture's gradient.  With
    w0 [R,R] f32 and wpyr [S], the weights of the texture's side, the pyramid is the coverage-weighted one."""

    @staticmethod
    def forward(ctx, tex, uv, state, face_uv, L, lod_bias, w0=None, wpyr=None):
        C, R = _texture_shape(tex)
        t = tex[0].contiguous()
        rho = uv_footprint(state.face_idx, state.face_xy, state.face_z, face_uv, state.B, state.H, state.W)
        out = mip_lookup(t, pyramid_build(t, L, w0, wpyr), uv, rho, state.face_idx, L, lod_bias, w0, wpyr)
        ctx.save_for_backward(uv, rho, state.face_idx, w0, wpyr)
        ctx.meta = (C, R, L, lod_bias)
        return out

    @staticmethod
    def backward(ctx, dout):
        uv, rho, face_idx, w0, wpyr = ctx.saved_tensors
        C, R, L, bias = ctx.meta
        dtex = mip_lookup_backward(dout.contiguous(), (C, R), uv, rho, face_idx, L, bias, w0, wpyr)
        return (dtex[None],) + (None,) * 7


class Renderer:
    def __init__(self, device, dim=(224, 224), interpolation_mode="nearest", max_mip_level=-1, lod_bias=0.0,
                 mip_coverage=False, coverage_ring=1, antialias=False, lights=DEFAULT_LIGHTS):
        assert interpolation_mode in ["nearest", "bilinear", "bicubic", "mipmap"], \
            "no interpolation mode %s" % interpolation_mode
        self.lights = check_lights(lights, "Renderer: lights")   # shade_views: nine SH coefficients, every view's default
        self._corners = {}                             # (faces, V) -> corner_table: the topology is fixed
        if not math.isfinite(lod_bias):
            raise ValueError("Renderer: lod_bias must be finite (got %r)" % (lod_bias,))
        if mip_coverage and interpolation_mode != "mipmap":
            raise ValueError("Renderer: mip_coverage needs interpolation_mode mipmap (got %s)" % interpolation_mode)
        if int(coverage_ring) < 0:
            raise ValueError("Renderer: coverage_ring must be >= 0 (got %r)" % (coverage_ring,))
        self.device = device
        self.interpolation_mode = interpolation_mode
        self.max_mip_level = int(max_mip_level)        # "mipmap" only: < 0 = every level the texture's side allows
        self.lod_bias = float(lod_bias)                # "mipmap" only: added to the level log2(footprint in texels)
        self.mip_coverage = bool(mip_coverage)         # "mipmap" only: the coverage-weighted pyramid (csrc/texmip.hip)
        self.coverage_ring = int(coverage_ring)        # ... rounds the covered texels are grown by (the bilinear taps' reach)
        self.antialias = bool(antialias)               # the models antialias their renders' edges (antialias_views)
        self._coverage = {}                            # (side, levels, UV layout) -> (w0 [R,R] f32, wpyr [S])
        self.fov = math.pi / 3                         # kal.render.camera.generate_perspective_projection(np.pi / 3)
        self.dim = dim
        self.background = torch.ones(dim).to(device).float()

    @staticmethod
    def get_camera_from_view(elev, azim, r=3.0, look_at_height=0.0, fov=math.pi / 3):
        """14 floats for the C ABI: rotation rows, eye position, fx, fy."""
        elev, azim = float(elev), float(azim)
        pos = [r * math.sin(elev) * math.sin(azim), r * math.cos(elev), r * math.sin(elev) * math.cos(azim)]
        look = [0.0, look_at_height, 0.0]
        z = [pos[i] - look[i] for i in range(3)]
        n = math.sqrt(sum(c * c for c in z))
        z = [c / n for c in z]
        up = [0.0, 1.0, 0.0]
        x = [up[1] * z[2] - up[2] * z[1], up[2] * z[0] - up[0] * z[2], up[0] * z[1] - up[1] * z[0]]
        n = math.sqrt(sum(c * c for c in x))
        x = [c / n for c in x]
        y = [z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]]
        f = 1.0 / math.tan(fov / 2)
        import ctypes
        return (ctypes.c_float * 14)(*(x + y + z + pos + [f, f]))

    def _cameras(self, elev, azim, radius, look_at_height):
        """[B,14] f32 on the device: row b holds the very floats get_camera_from_view gives for view b."""
        rows = [list(self.get_camera_from_view(e, a, r, look_at_height, self.fov)) for e, a, r in zip(elev, azim, radius)]
        return torch.tensor(rows, dtype=torch.float32).to(self.device)

    def _rasterize_views(self, verts, faces, elev, azim, radius, look_at_height, dims):
        """B views of one mesh through the tile-culled rasteriser -> (face_idx [B*H*W], bary [B*H*W,3], B, H, W)."""
        st = self._rasterize_views_faces(verts, faces, elev, azim, radius, look_at_height, dims)
        return st.face_idx, st.bary, st.B, st.H, st.W

    def _rasterize_views_faces(self, verts, faces, elev, azim, radius, look_at_height, dims):
        """The RasterState of B views: _rasterize_views' result followed by the projected faces it was made from."""
        elev, azim, radius = list(elev), list(azim), list(radius)
        B = len(elev)
        if B < 1 or len(azim) != B or len(radius) != B:
            raise ValueError("render_views: elev, azim and radius must be sequences of one length >= 1 (got %d, %d, %d)"
                             % (B, len(azim), len(radius)))
        H, W = dims[1], dims[0]
        cams = self._cameras(elev, azim, radius, look_at_height)
        verts = verts.to(self.device).float().contiguous()
        faces32 = faces.to(self.device).to(torch.int32).contiguous()
        nodes = (_PrepareBatch.apply, _RasterizeBatch.apply) if _learns(verts) else ()   # the same launches, in the graph
        return rasterize_views(verts, faces32, cams, H, W, *nodes)

    def coverage_weights(self, verts, faces, face_uv, R, L):
        """(w0 [R,R] f32 of 0 / 1, wpyr [S]) of one UV layout at one texture side, computed once: render_test passes the
        decoded texture, whose side is not the trained one."""
        key = (int(R), int(L), face_uv.data_ptr(), tuple(face_uv.shape))
        if key not in self._coverage:
            w0 = texture_coverage(verts.to(self.device), faces.to(self.device), face_uv, R, self.coverage_ring).float()
            self._coverage[key] = (w0.contiguous(), mipcov_weights(w0, L))
        return self._coverage[key]

    def _rasterize(self, verts, faces, elev, azim, radius, look_at_height, dims):
        st = self._rasterize_views_faces(verts, faces, [elev], [azim], [radius], look_at_height, dims)
        return st.face_idx, st.bary, st.H, st.W

    def render_views(self, mesh, face_attributes, elev, azim, radius, look_at_height=0.0):
        """B views in one call: elev, azim, radius are sequences of length B.  face_attributes [1,F,3,D] ->
        (image [B,D,H,W], mask [B,1,H,W]); differentiable w.r.t. the attributes (their gradient sums over the views) and,
        when mesh.vertices require grad, w.r.t. the vertices inside every face (silhouettes: antialias_views)."""
        face_idx, bary, B, H, W = self._rasterize_views(mesh.vertices, mesh.faces, elev, azim, radius, look_at_height,
                                                        self.dim)
        feat = _InterpAttr.apply(face_attributes[0], face_idx, bary)
        mask = (face_idx > -1).float().reshape(B, H, W, 1)
        return feat.reshape(B, H, W, -1).permute(0, 3, 1, 2), mask.permute(0, 3, 1, 2)

    def render_views_texture(self, verts, faces, uv_face_attr, texture_map, elev, azim, radius, look_at_height=0.0,
                             dims=None, white_background=False, return_state=False):
        """B views of the textured mesh in one call -> (image [B,C,H,W], mask [B,1,H,W]).  The batch is B*H*W flat
        pixels through the single-view kernels; the texture is shared, so its gradient sums over the views.
        `verts` that require grad receive the image's gradient through the UVs (bilinear lookup only: any other mode
        raises before a launch); the mask stays hard, so a silhouette moves only under antialias_views.
        return_state: the rasterisation state of _rasterize_views_faces follows as a third result."""
        dims = self.dim if dims is None else dims
        learns = _learns(verts)
        if learns and self.interpolation_mode != "bilinear":
            raise ValueError("render_views_texture: vertex gradients need interpolation_mode bilinear (got %s)"
                             % self.interpolation_mode)
        state = self._rasterize_views_faces(verts, faces, elev, azim, radius, look_at_height, dims)
        face_idx, B, H, W = state.face_idx, state.B, state.H, state.W
        face_uv = uv_face_attr[0].detach().contiguous()
        with torch.set_grad_enabled(learns):           # off: uv_features.detach() in the reference (:61)
            uv = _InterpAttr.apply(face_uv, face_idx, state.bary).contiguous()
        if self.interpolation_mode == "mipmap":
            R = texture_map.shape[-1]
            L = mip_levels(R, self.max_mip_level)      # per call: render_test passes the decoded, larger texture
            weights = self.coverage_weights(verts, faces, face_uv, R, L) if self.mip_coverage else ()
            image = _TextureMip.apply(texture_map, uv, state, face_uv, L, self.lod_bias, *weights)
        else:
            image = _TextureMap.apply(texture_map, uv, face_idx, _MODES[self.interpolation_mode])
        mask = (face_idx > -1).float().reshape(B, H, W, 1)
        image = image.reshape(B, H, W, -1) * mask
        if white_background:
            image = image + 1 * (1 - mask)
        if return_state:
            return image.permute(0, 3, 1, 2), mask.permute(0, 3, 1, 2), state
        return image.permute(0, 3, 1, 2), mask.permute(0, 3, 1, 2)

    def antialias_views(self, image, raster_state, faces):
        """Edge antialiasing of a rendered batch (lnerf_raster_antialias_forward): image [B,C,H,W] -> [B,C,H,W].  Across
        every depth discontinuity between neighbouring pixels the nearer face's edge is located between the two pixel
        centres and the pixel it cuts is blended with its neighbour by the covered fraction, which makes the image a
        differentiable function of the projected edge: the gradient reaches the image and, through raster_state's
        face_xy, the vertices.  raster_state: the RasterState _rasterize_views_faces returned for these views; faces: the
        mesh's [F,3] vertex ids (edges between faces that share both vertices are interior and left alone)."""
        st = RasterState(*raster_state)
        if image.dim() != 4 or image.shape[0] != st.B or tuple(image.shape[2:]) != (st.H, st.W):
            raise ValueError("antialias_views: image must be [%d,C,%d,%d] (got %s)" % (st.B, st.H, st.W, tuple(image.shape)))
        faces32 = faces.to(self.device).to(torch.int32).contiguous()
        out = _Antialias.apply(image.float().permute(0, 2, 3, 1).contiguous(), st.face_xy, st.face_idx, st.bary.detach(),
                               st.face_z.detach(), faces32)
        return out.permute(0, 3, 1, 2)

    def corner_table(self, faces, n_verts):
        """corner_table of one mesh, computed once (keyed like coverage_weights: Latent-Paint never changes its faces)."""
        key = (faces.data_ptr(), tuple(faces.shape), int(n_verts))
        if key not in self._corners:
            self._corners[key] = corner_table(faces.to(self.device), int(n_verts))
        return self._corners[key]

    def _lights(self, lights, B):
        """None (self.lights), nine floats or [B,9] -> [B,9] f32 on the device, one row per view."""
        if torch.is_tensor(lights) and lights.dim() == 2:
            if tuple(lights.shape) != (B, 9) or not bool(torch.isfinite(lights).all()):
                raise ValueError("shade_views: lights must be nine floats or a finite [%d,9] (got %s)"
                                 % (B, tuple(lights.shape)))
            return lights.detach().to(self.device).float().contiguous()
        row = self.lights if lights is None else check_lights(lights, "shade_views: lights")
        return torch.tensor([row] * B, dtype=torch.float32).to(self.device)

    def shade_views(self, verts, faces, raster_state, lights=None):
        """The shading of a rendered batch (csrc/meshshade.hip) -> (normal [B,3,H,W], lighting [B,1,H,W], depth [B,1,H,W]).
        normal: the smooth vertex normals of the mesh (unit sums of unit face normals, world space) interpolated with the
        pixel's barycentrics and normalised; lighting: nine-term SH under `lights` (nine floats or [B,9]; None:
        self.lights), clamped to [1e-8, 1]; depth: the camera-space distance along the view axis, positive.  Background
        pixels hold 0 in all three.  raster_state: the RasterState _rasterize_views_faces returned for these verts.
        With `verts` that require grad all three are differentiable w.r.t. them: through the normals, and through the
        barycentrics and depths of raster_state when that was rendered from the same `verts`.  Otherwise no graph is
        recorded and the two forward kernels are all that is launched."""
        st = RasterState(*raster_state)
        verts = verts.to(self.device).float().contiguous()
        faces32 = faces.to(self.device).to(torch.int32).contiguous()
        corner_start, corner_list = self.corner_table(faces, verts.shape[0])
        lights = self._lights(lights, st.B)
        if _learns(verts):
            vn = _VertexNormals.apply(verts, faces32, corner_start, corner_list)
            normal, lighting, depth = _ShadePixels.apply(vn, st.bary, st.face_z, st.face_idx, faces32, lights,
                                                         st.B, st.H, st.W)
        else:
            with torch.no_grad():
                vn = vertex_normals(verts, faces32, corner_start, corner_list)
                normal, lighting, depth = shade_pixels(vn, st.bary.detach(), st.face_z.detach(), st.face_idx, faces32,
                                                       lights, st.B, st.H, st.W)
        as_image = lambda t, c: t.reshape(st.B, st.H, st.W, c).permute(0, 3, 1, 2)
        return as_image(normal, 3), as_image(lighting, 1), as_image(depth, 1)

    def render_single_view(self, mesh, face_attributes, elev=0, azim=0, radius=2, look_at_height=0.0):
        """face_attributes [1,F,3,D] -> (image [1,D,H,W], mask [1,1,H,W]); differentiable w.r.t. the attributes."""
        return self.render_views(mesh, face_attributes, [elev], [azim], [radius], look_at_height)

    def render_single_view_texture(self, verts, faces, uv_face_attr, texture_map, elev=0, azim=0, radius=2,
                                   look_at_height=0.0, dims=None, white_background=False):
        return self.render_views_texture(verts, faces, uv_face_attr, texture_map, [elev], [azim], [radius],
                                         look_at_height, dims=dims, white_background=white_background)
