"""View-projected textures, shared by the two export paths: NeRFRenderer.export_mesh(bake_views=K) and Latent-Paint's
TexturedMeshModel.export_mesh(bake_views=K) both render K views of their model, decode them AS IMAGES, and project the
decoded pixels back into the mesh's UV atlas here ("View-projected albedo")."""
import torch

from .latent_nerf.raymarching import raymarching as rm

TEXTURE_FILLS = ("dilate", "pullpush")   # what an exported texture holds outside its charts
BAKE_UNSEEN = ("fallback", "inpaint")    # what a view bake gives the covered texels no view sees


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


def bake_views(verts, faces, vt, ft, images, cams, resolution, gutter=4, fallback=None, erode=0, cos_min=0.2, power=4.0,
               slack=2.0, fill="dilate", unseen="fallback"):
    """Project K images of a UV-mapped mesh into its R x R atlas.  images [K,C,H,W] (C <= 4) as seen by the cameras
    cams [K,14] (the rasteriser's records).  The texels and their surface points come from raymarching.uv_raster, a
    texel's normal is the winding normal of the face that covers it, visibility from raymarching.view_zbuffer at the
    images' size (`erode` pixels taken off every silhouette), the colours from raymarching.project_views.  A covered
    texel that no view sees takes `fallback` ([C,R,R]; zeros if None) or, with unseen="inpaint", is filled from the seen
    texels (raymarching.pull_push_fill with weight 1 on the seen covered texels; with no seen texel at all the fallback
    stays); then `gutter` dilation rounds, as the point bake, and `fill` (fill_atlas) for the rest of the atlas.
    -> dict(rgb [C,R,R], view_weight [R,R], view_count [R,R] int32, mask [R,R] uint8 (2 covered, 1 gutter, 3 filled by
    "pullpush", 0 empty))."""
    check_choice(fill, TEXTURE_FILLS, "bake_views: fill")
    check_choice(unseen, BAKE_UNSEEN, "bake_views: unseen")
    R = int(resolution)
    verts = verts.to(torch.float32).contiguous()
    dev = verts.device
    images = images.to(dev).float().contiguous()
    K, C, H, W = images.shape
    texel_face, texel_idx, pos = rm.uv_raster(verts, faces, vt, ft, R)
    idx = texel_idx.long()
    nrm = face_normals(verts, faces.to(dev))[texel_face.reshape(-1)[idx].long()].contiguous()
    zbuf = rm.view_zbuffer(verts, faces, cams, H, W, erode=erode)
    out, weight, count = rm.project_views(pos, nrm, cams, zbuf, images, cos_min=cos_min, power=power, slack=slack)
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
    return {"rgb": texture, "view_weight": view_weight.view(R, R), "view_count": view_count.view(R, R), "mask": mask}


def to_uint8(rgb):
    """[3,R,R] in [0, 1] -> uint8 [R,R,3], rounded: what albedo.png holds."""
    return (rgb.clamp(0, 1).permute(1, 2, 0).cpu().numpy() * 255).round().astype("uint8")
