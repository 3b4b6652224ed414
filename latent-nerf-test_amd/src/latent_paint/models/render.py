"""HIP-backed counterpart of src/latent_paint/models/render.py (Renderer :5-69): same constructor, camera
convention (:19-31) and the two render entry points (:34-47, :50-69), with the kaolin calls replaced by the
C-ABI raster kernels (csrc/raster.hip).  `render_views` / `render_views_texture` take B views per call (the fork's
`render.batch_size`); the single-view methods are their B = 1 case, on the one tile-culled rasteriser.
`interpolation_mode="mipmap"` is this project's own: the trilinear mip-mapped lookup of csrc/texmip.hip, for renders much
smaller than their texture; with `mip_coverage` its pyramid is the coverage-weighted one of the same file, which keeps the
texels no face covers out of every level."""
import math

import torch

from ...latent_nerf.raymarching import backend as _b
from ...latent_nerf.raymarching.raymarching import (_chk, _p, _stream, mip_build, mip_levels, mip_texels,  # noqa: F401
                                                    mipcov_weights, pyramid_build, pyramid_fold, uv_dilate, uv_raster)

_MODES = {"nearest": 0, "bilinear": 1, "bicubic": 2}   # lnerf_texture_map_*'s point lookups ("mipmap": _TextureMip)


def _texture_shape(tex):
    """(C, R) of the one square [1,C,R,R] texture the lookup kernels read."""
    if tex.dim() != 4 or tex.shape[0] != 1 or tex.shape[2] != tex.shape[3]:
        raise ValueError("texture_map: texture must be [1,C,R,R] (got %s)" % (tuple(tex.shape),))
    return tex.shape[1], tex.shape[2]


class _InterpAttr(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, face_idx, bary):
        P, D = face_idx.shape[0], attr.shape[-1]
        attr = attr.contiguous()
        feat = torch.empty(P, D, device=attr.device)
        _b.call("lnerf_interpolate_attributes", _p(face_idx), _p(bary), _chk(attr, "attr"), P, D, _p(feat), _stream())
        ctx.save_for_backward(face_idx, bary)
        ctx.shape = attr.shape
        return feat

    @staticmethod
    def backward(ctx, dfeat):
        face_idx, bary = ctx.saved_tensors
        dattr = torch.zeros(ctx.shape, device=dfeat.device)
        _b.call("lnerf_interpolate_attributes_backward", _p(face_idx), _p(bary), _chk(dfeat.contiguous(), "dfeat"),
                face_idx.shape[0], ctx.shape[-1], _p(dattr), _stream())
        return dattr, None, None


class _TextureMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv, face_idx, mode):
        C, R = _texture_shape(tex)
        P = uv.shape[0]
        tex = tex.contiguous()
        out = torch.empty(P, C, device=tex.device)
        _b.call("lnerf_texture_map_forward", _chk(uv, "uv"), _p(face_idx), _chk(tex, "texture"), P, C, R, mode, _p(out),
                _stream())
        ctx.save_for_backward(uv, face_idx)
        ctx.meta = (tex.shape, mode)
        return out

    @staticmethod
    def backward(ctx, dout):
        uv, face_idx = ctx.saved_tensors
        shape, mode = ctx.meta
        dtex = torch.zeros(shape, device=dout.device)
        _b.call("lnerf_texture_map_backward", _p(uv), _p(face_idx), _chk(dout.contiguous(), "dout"), uv.shape[0],
                shape[1], shape[2], mode, _p(dtex), _stream())
        return dtex, None, None, None


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
    def forward(ctx, tex, uv, face_idx, face_xy, face_z, face_uv, dims, L, lod_bias, w0=None, wpyr=None):
        C, R = _texture_shape(tex)
        B, H, W = dims
        t = tex[0].contiguous()
        rho = uv_footprint(face_idx, face_xy, face_z, face_uv, B, H, W)
        out = mip_lookup(t, pyramid_build(t, L, w0, wpyr), uv, rho, face_idx, L, lod_bias, w0, wpyr)
        ctx.save_for_backward(uv, rho, face_idx, w0, wpyr)
        ctx.meta = (C, R, L, lod_bias)
        return out

    @staticmethod
    def backward(ctx, dout):
        uv, rho, face_idx, w0, wpyr = ctx.saved_tensors
        C, R, L, bias = ctx.meta
        dtex = mip_lookup_backward(dout.contiguous(), (C, R), uv, rho, face_idx, L, bias, w0, wpyr)
        return (dtex[None],) + (None,) * 10


class Renderer:
    def __init__(self, device, dim=(224, 224), interpolation_mode="nearest", max_mip_level=-1, lod_bias=0.0,
                 mip_coverage=False, coverage_ring=1):
        assert interpolation_mode in ["nearest", "bilinear", "bicubic", "mipmap"], \
            "no interpolation mode %s" % interpolation_mode
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
        return self._rasterize_views_faces(verts, faces, elev, azim, radius, look_at_height, dims)[:5]

    def _rasterize_views_faces(self, verts, faces, elev, azim, radius, look_at_height, dims):
        """_rasterize_views' result followed by the projected faces it was made from: face_xy [B,F,3,2], face_z [B,F,3]."""
        elev, azim, radius = list(elev), list(azim), list(radius)
        B = len(elev)
        if B < 1 or len(azim) != B or len(radius) != B:
            raise ValueError("render_views: elev, azim and radius must be sequences of one length >= 1 (got %d, %d, %d)"
                             % (B, len(azim), len(radius)))
        H, W = dims[1], dims[0]
        cams = self._cameras(elev, azim, radius, look_at_height)
        verts = verts.to(self.device).float().contiguous()
        faces32 = faces.to(self.device).to(torch.int32).contiguous()
        F = faces32.shape[0]
        face_z = torch.empty(B, F, 3, device=self.device)
        face_xy = torch.empty(B, F, 3, 2, device=self.device)
        face_box = torch.empty(B, F, 4, device=self.device, dtype=torch.int16)
        _b.call("lnerf_raster_prepare_batch", _chk(verts, "verts"), verts.shape[0], _chk(faces32, "faces", torch.int32),
                F, _chk(cams, "cams"), B, H, W, _p(face_z), _p(face_xy), _p(face_box), _stream())
        face_idx = torch.empty(B * H * W, device=self.device, dtype=torch.int32)
        bary = torch.empty(B * H * W, 3, device=self.device)
        _b.call("lnerf_rasterize_batch", B, H, W, _p(face_z), _p(face_xy), _p(face_box), F, _p(face_idx), _p(bary),
                _stream())
        return face_idx, bary, B, H, W, face_xy, face_z

    def coverage_weights(self, verts, faces, face_uv, R, L):
        """(w0 [R,R] f32 of 0 / 1, wpyr [S]) of one UV layout at one texture side, computed once: render_test passes the
        decoded texture, whose side is not the trained one."""
        key = (int(R), int(L), face_uv.data_ptr(), tuple(face_uv.shape))
        if key not in self._coverage:
            w0 = texture_coverage(verts.to(self.device), faces.to(self.device), face_uv, R, self.coverage_ring).float()
            self._coverage[key] = (w0.contiguous(), mipcov_weights(w0, L))
        return self._coverage[key]

    def _rasterize(self, verts, faces, elev, azim, radius, look_at_height, dims):
        face_idx, bary, _, H, W = self._rasterize_views(verts, faces, [elev], [azim], [radius], look_at_height, dims)
        return face_idx, bary, H, W

    def render_views(self, mesh, face_attributes, elev, azim, radius, look_at_height=0.0):
        """B views in one call: elev, azim, radius are sequences of length B.  face_attributes [1,F,3,D] ->
        (image [B,D,H,W], mask [B,1,H,W]); differentiable w.r.t. the attributes (their gradient sums over the views)."""
        face_idx, bary, B, H, W = self._rasterize_views(mesh.vertices, mesh.faces, elev, azim, radius, look_at_height,
                                                        self.dim)
        feat = _InterpAttr.apply(face_attributes[0], face_idx, bary)
        mask = (face_idx > -1).float().reshape(B, H, W, 1)
        return feat.reshape(B, H, W, -1).permute(0, 3, 1, 2), mask.permute(0, 3, 1, 2)

    def render_views_texture(self, verts, faces, uv_face_attr, texture_map, elev, azim, radius, look_at_height=0.0,
                             dims=None, white_background=False):
        """B views of the textured mesh in one call -> (image [B,C,H,W], mask [B,1,H,W]).  The batch is B*H*W flat
        pixels through the single-view kernels; the texture is shared, so its gradient sums over the views."""
        dims = self.dim if dims is None else dims
        face_idx, bary, B, H, W, face_xy, face_z = self._rasterize_views_faces(verts, faces, elev, azim, radius,
                                                                               look_at_height, dims)
        face_uv = uv_face_attr[0].detach().contiguous()
        with torch.no_grad():                          # uv_features.detach() in the reference (:61)
            uv = _InterpAttr.apply(face_uv, face_idx, bary).contiguous()
        if self.interpolation_mode == "mipmap":
            R = texture_map.shape[-1]
            L = mip_levels(R, self.max_mip_level)      # per call: render_test passes the decoded, larger texture
            weights = self.coverage_weights(verts, faces, face_uv, R, L) if self.mip_coverage else ()
            image = _TextureMip.apply(texture_map, uv, face_idx, face_xy, face_z, face_uv, (B, H, W), L, self.lod_bias,
                                      *weights)
        else:
            image = _TextureMap.apply(texture_map, uv, face_idx, _MODES[self.interpolation_mode])
        mask = (face_idx > -1).float().reshape(B, H, W, 1)
        image = image.reshape(B, H, W, -1) * mask
        if white_background:
            image = image + 1 * (1 - mask)
        return image.permute(0, 3, 1, 2), mask.permute(0, 3, 1, 2)

    def render_single_view(self, mesh, face_attributes, elev=0, azim=0, radius=2, look_at_height=0.0):
        """face_attributes [1,F,3,D] -> (image [1,D,H,W], mask [1,1,H,W]); differentiable w.r.t. the attributes."""
        return self.render_views(mesh, face_attributes, [elev], [azim], [radius], look_at_height)

    def render_single_view_texture(self, verts, faces, uv_face_attr, texture_map, elev=0, azim=0, radius=2,
                                   look_at_height=0.0, dims=None, white_background=False):
        return self.render_views_texture(verts, faces, uv_face_attr, texture_map, [elev], [azim], [radius],
                                         look_at_height, dims=dims, white_background=white_background)
