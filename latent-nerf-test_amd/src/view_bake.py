"""View-projected textures, shared by the two export paths: NeRFRenderer.export_mesh(bake_views=K) and Latent-Paint's
TexturedMeshModel.export_mesh(bake_views=K) both render K views of their model, decode them AS IMAGES, and project the
decoded pixels back into the mesh's UV atlas here ("View-projected albedo")."""
import torch

from .latent_nerf.raymarching import raymarching as rm

TEXTURE_FILLS = ("dilate", "pullpush")   # what an exported texture holds outside its charts
BAKE_UNSEEN = ("fallback", "inpaint")    # what a view bake gives the covered texels no view sees
BAKE_BLENDS = ("mean", "bands")          # how a view bake combines the views that see a texel
EXPOSURE_PRIOR = 1.5e-3                  # exposure_gains' default: (sigma_N / sigma_g)^2 = ((1 / 255) / 0.1)^2


def check_choice(value, choices, name):
    if value not in choices:
        raise ValueError("%s must be one of %s, not %r" % (name, " | ".join(choices), value))
    return value


def fill_atlas(texture, mask, fill):
    """The last step of every bake, after the gutter rounds.  "dilate": nothing more -- the gutter is all there is.
    "pullpush": every texel the gutter left empty is filled from the non-empty ones (raymarching.pull_push_fill with
    weight 1 where mask > 0), so that no mip level built from the image averages the empty colour in; texels with
    mask > 0 keep their bits, the filled ones get mask code 3.  texture [C,R,R], mask [R,R] uint8 -> (texture, mask)."""
    check_choice(fill, TEXTURE_FILLS, "fill")
    if fill == "dilate":
        return texture, mask
    texture, filled = rm.pull_push_fill(texture, (mask > 0).float())
    mask[filled > 0] = 3
    return texture, mask


def face_normals(verts, faces):
    """Unit winding normals [F,3] of a mesh, (b - a) x (c - a) normalised (0 for a degenerate face)."""
    tri = verts.float()[faces.long()]
    n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    return n / n.norm(dim=-1, keepdim=True).clamp_min(1e-30)


def view_cameras(poses, radius, fovy_deg, H, W, device, target=(0.0, 0.0, 0.0)):
    """[K,14] camera records on `device` for the (theta, phi) of bake_view_poses, through the NeRF camera: the pose of
    pose_from_angles at `radius` around `target` and the intrinsics of intrinsics_from_fov.
    -> (cams [K,14], c2w [K,4,4] on the host, intrinsics (fx, fy, cx, cy))."""
    from .latent_nerf.models.nerf_utils import intrinsics_from_fov, pose_from_angles
    intr = intrinsics_from_fov(fovy_deg, H, W)
    c2w = torch.stack([pose_from_angles(max(t, 1e-3), p, radius, target) for t, p in poses])
    rows = [rm.nerf_camera_record(m, *intr, H, W) for m in c2w]
    return torch.tensor(rows, dtype=torch.float32).to(device), c2w, intr


def exposure_gains(N, S, prior=EXPOSURE_PRIOR):
    """One gain per view and channel from the overlap statistics of raymarching.view_overlap_stats (Brown & Lowe's gain
    compensation), on the host in float64.  N [K,K] int64: points views i and j both accept; S [K,K,C] int64: the sums
    of round(2^24 x what view i shows there), so M_ij = S_ij / (2^24 N_ij) is view i's mean colour on the overlap (0
    where N_ij = 0).  Per channel the gains minimise
        sum_{i<j} N_ij (g_i M_ij - g_j M_ji)^2  +  prior * sum_i n_i (g_i - 1)^2,      n_i = sum_{j != i} N_ij,
    i.e. solve A g = b with A_ii = sum_j N_ij (M_ij^2 + prior), A_ij = -N_ij M_ij M_ji, b_i = prior * n_i; a view with
    n_i = 0 (it overlaps no other) gets exactly 1.  `prior` (> 0) is (sigma_N / sigma_g)^2 of the paper's error model:
    how far a gain may drift from 1 against how well two views must agree.  The default takes the paper's sigma_g =
    0.1 and sigma_N = 1 / 255, one 8-bit step, because the views are noise-free renders and not photographs; the
    paper's sigma_N = 10 / 255 leaves about a quarter of a gain error uncorrected on mid-grey images.  The default was
    derived, not tuned.  -> gains [K,C] float64 (a CPU tensor)."""
    prior = float(prior)
    if not prior > 0.0:
        raise ValueError("exposure_gains: prior must be > 0 (got %r)" % (prior,))
    N = torch.as_tensor(N).detach().cpu()
    S = torch.as_tensor(S).detach().cpu()
    if N.dim() != 2 or N.shape[0] != N.shape[1] or S.dim() != 3 or tuple(S.shape[:2]) != tuple(N.shape):
        raise ValueError("exposure_gains: N must be [K,K] and S [K,K,C], not %s and %s" % (tuple(N.shape), tuple(S.shape)))
    K, C = N.shape[0], S.shape[2]
    off = ~torch.eye(K, dtype=torch.bool)
    n = torch.where(off, N, torch.zeros_like(N)).double()                      # the diagonal is not a pair
    M = torch.where(n[..., None] > 0, S.double() / (16777216.0 * n.clamp_min(1.0))[..., None], torch.zeros(()).double())
    alone = n.sum(1) == 0
    gains = torch.ones(K, C, dtype=torch.float64)
    for c in range(C):
        m = M[..., c]
        A = -n * m * m.T
        A[range(K), range(K)] = (n * (m * m + prior)).sum(1)
        b = prior * n.sum(1)
        A[alone, alone] = 1.0
        b[alone] = 1.0
        gains[:, c] = torch.linalg.solve(A, b)
    gains[alone] = 1.0
    return gains


def bake_views(verts, faces, vt, ft, images, cams, resolution, gutter=4, fallback=None, erode=0, cos_min=0.2, power=4.0,
               slack=2.0, fill="dilate", unseen="fallback", blend="mean", exposure=False, band_sigma=0.0):
    """Project K images of a UV-mapped mesh into its R x R atlas.  images [K,C,H,W] (C <= 4) as seen by the cameras
    cams [K,14] (the rasteriser's records).  The texels and their surface points come from raymarching.uv_raster, a
    texel's normal is the winding normal of the face that covers it, visibility from raymarching.view_zbuffer at the
    images' size (`erode` pixels taken off every silhouette), the colours from raymarching.project_views.  A covered
    texel that no view sees takes `fallback` ([C,R,R]; zeros if None) or, with unseen="inpaint", is filled from the seen
    texels (raymarching.pull_push_fill with weight 1 on the seen covered texels; with no seen texel at all the fallback
    stays); then `gutter` dilation rounds, as the point bake, and `fill` (fill_atlas) for the rest of the atlas.
    blend = "mean": the weighted mean of the views (project_views).  blend = "bands": two-band blending
    (project_views_bands) -- the views are low-passed with a Gaussian of `band_sigma` pixels (view_lowpass; 0 = 1 pixel
    here: the exporters pass max(1, decoded side / render side), one pixel of the render, the finest scale at which
    independently decoded views agree); a texel's low band is the weighted mean of the views' low bands and everything
    finer comes from its best view alone, so nothing above the band limit is averaged.  exposure = True: one gain per
    view and channel (exposure_gains, from view_overlap_stats of the low-passed views; K <= 64) multiplies the views
    before they are combined.  With "mean" and exposure = False the path and every output are the plain bake's.
    -> dict(rgb [C,R,R], view_weight [R,R], view_count [R,R] int32, mask [R,R] uint8 (2 covered, 1 gutter, 3 filled by
    "pullpush", 0 empty); with exposure: view_gains [K,C]; with "bands": view_best [R,R] int32, the best view of a seen
    texel, -1 elsewhere)."""
    check_choice(fill, TEXTURE_FILLS, "bake_views: fill")
    check_choice(unseen, BAKE_UNSEEN, "bake_views: unseen")
    check_choice(blend, BAKE_BLENDS, "bake_views: blend")
    band_sigma = float(band_sigma)
    if not 0.0 <= band_sigma <= rm.LOWPASS_MAX_R / 3.0:
        raise ValueError("bake_views: band_sigma must be in [0, %g] (got %r)" % (rm.LOWPASS_MAX_R / 3.0, band_sigma))
    R = int(resolution)
    verts = verts.to(torch.float32).contiguous()
    dev = verts.device
    images = images.to(dev).float().contiguous()
    K, C, H, W = images.shape
    texel_face, texel_idx, pos = rm.uv_raster(verts, faces, vt, ft, R)
    idx = texel_idx.long()
    nrm = face_normals(verts, faces.to(dev))[texel_face.reshape(-1)[idx].long()].contiguous()
    zbuf = rm.view_zbuffer(verts, faces, cams, H, W, erode=erode)
    extra = {}
    if blend == "mean" and not exposure:
        out, weight, count = rm.project_views(pos, nrm, cams, zbuf, images, cos_min=cos_min, power=power, slack=slack)
    else:
        low = rm.view_lowpass(images, zbuf, band_sigma if band_sigma > 0 else 1.0)
        gains = None
        if exposure:
            if K > rm.STATS_MAX_K:
                raise ValueError("bake_views: exposure matching takes at most %d views (got %d)" % (rm.STATS_MAX_K, K))
            N, S = rm.view_overlap_stats(pos, nrm, cams, zbuf, low, cos_min=cos_min, slack=slack)
            gains = exposure_gains(N, S).to(device=dev, dtype=torch.float32)
            extra["view_gains"] = gains
        if blend == "bands":
            out, weight, count, best = rm.project_views_bands(pos, nrm, cams, zbuf, images, low, gains, cos_min=cos_min,
                                                              power=power, slack=slack)
            view_best = torch.full((R * R,), -1, device=dev, dtype=torch.int32)
            view_best[texel_idx.long()] = best
            extra["view_best"] = view_best.view(R, R)
        else:
            out, weight, count = rm.project_views(pos, nrm, cams, zbuf, images * gains[:, :, None, None], cos_min=cos_min,
                                                  power=power, slack=slack)
    if fallback is None:
        texture = torch.zeros(C, R * R, device=dev)
    else:
        if tuple(fallback.shape) != (C, R, R):
            raise ValueError("bake_views: fallback must be [%d,%d,%d], not %s" % (C, R, R, tuple(fallback.shape)))
        texture = fallback.to(dev).float().reshape(C, R * R).clone()
    seen = count > 0
    texture[:, idx[seen]] = out[seen].T
    if unseen == "inpaint" and bool(seen.any()) and not bool(seen.all()):
        known = torch.zeros(R * R, device=dev)
        known[idx[seen]] = 1.0
        inpainted, _ = rm.pull_push_fill(texture.view(C, R, R), known.view(R, R))
        hole = idx[~seen]
        texture[:, hole] = inpainted.reshape(C, R * R)[:, hole]
    view_weight = torch.zeros(R * R, device=dev)
    view_count = torch.zeros(R * R, device=dev, dtype=torch.int32)
    view_weight[idx] = weight
    view_count[idx] = count
    mask = (texel_face.reshape(-1) >= 0).to(torch.uint8) * 2
    texture, mask = texture.view(C, R, R).contiguous(), mask.view(R, R)
    if fallback is not None:
        # the fallback's own gutter is not part of this bake: the covered texels alone seed the dilation
        texture = texture * (mask > 0)[None]
    rm.uv_dilate(texture, mask, gutter)
    texture, mask = fill_atlas(texture, mask, fill)
    return {"rgb": texture, "view_weight": view_weight.view(R, R), "view_count": view_count.view(R, R), "mask": mask,
            **extra}


def to_uint8(rgb):
    """[3,R,R] in [0, 1] -> uint8 [R,R,3], rounded: what albedo.png holds."""
    return (rgb.clamp(0, 1).permute(1, 2, 0).cpu().numpy() * 255).round().astype("uint8")
