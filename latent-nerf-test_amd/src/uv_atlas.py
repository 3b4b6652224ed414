"""UV atlas shared by the two paths: Latent-Paint paints a mesh through it when the mesh has no UVs of its own, and
NeRFRenderer.export_mesh bakes the field into it when asked for a textured mesh."""
import numpy as np
import torch

MIN_TEXELS_PER_CELL = 4   # below this a chart covers too few texel centres to carry a texture


def atlas_cells(n_faces):
    """Side n of the n x n cell grid per_triangle_atlas lays `n_faces` out on (two faces per cell)."""
    return int(np.ceil(np.sqrt((int(n_faces) + 1) // 2)))


def atlas_min_resolution(n_faces, texels_per_cell=MIN_TEXELS_PER_CELL):
    """Smallest texture side that gives every cell of the per-triangle atlas `texels_per_cell` texels across."""
    return max(1, atlas_cells(n_faces)) * int(texels_per_cell)


def per_triangle_atlas(n_faces, device):
    """UV atlas that needs no unwrapping library: the unit square is cut into n x n cells, two triangles per cell
    (lower-left and upper-right half, with a margin so neighbouring charts do not bleed).  Every face gets three
    texture vertices of its own: vt [3F,2], ft [F,3]."""
    n = atlas_cells(n_faces)
    k = torch.arange(n_faces, device=device)
    cell, upper = k // 2, (k % 2).float()[:, None]
    org = torch.stack([(cell % n).float(), (cell // n).float()], -1)
    lo, hi, m = 0.08, 0.92, 0.06
    lower_tri = torch.tensor([[lo, lo], [hi - m, lo], [lo, hi - m]], device=device)
    upper_tri = torch.tensor([[hi, hi], [lo + m, hi], [hi, lo + m]], device=device)
    corners = lower_tri[None] * (1 - upper[..., None]) + upper_tri[None] * upper[..., None]   # [F,3,2]
    vt = ((org[:, None, :] + corners) / n).reshape(-1, 2)
    ft = torch.arange(3 * n_faces, device=device).reshape(n_faces, 3)
    return vt.float(), ft.long()


# ------------------------------------------------------------------------------ chart atlas (include/lnerf_hip.h)
ATLAS_SHRINK = 0.95      # s_k = s_0 * ATLAS_SHRINK^k
ATLAS_MAX_SHRINKS = 200  # the scale search gives up past this k
ATLAS_CHOICES = ("triangle", "charts")


def check_atlas_choice(value, name):
    """`value` if it names an atlas, else a ValueError that names the setting."""
    if value not in ATLAS_CHOICES:
        raise ValueError("%s must be one of %s, not %r" % (name, " | ".join(ATLAS_CHOICES), value))
    return value


def atlas_scale(ext_p, ext_q, R, pad, k):
    """s_k of the scale search, rounded to f32 (returned as a Python float): the largest chart spans the side at k = 0."""
    m = max(float(np.max(ext_p, initial=0.0)), float(np.max(ext_q, initial=0.0)))
    s0 = (R - 2 * pad - 2) / m if m > 0 else 1.0
    return float(np.float32(s0 * ATLAS_SHRINK ** k))


def chart_rect_sizes(ext_p, ext_q, s, pad):
    """(w, h) int64 of the charts' rectangles at scale s: the content, a texel of rounding room and the pad each side."""
    w = 2 * pad + 2 + np.floor(np.asarray(ext_p, np.float64) * s).astype(np.int64)
    h = 2 * pad + 2 + np.floor(np.asarray(ext_q, np.float64) * s).astype(np.int64)
    return w, h


def shelf_pack(w, h, R, state=(0, 0, 0)):
    """Shelf-pack rectangles into R x R in the order (h desc, w desc, index asc), continuing from `state` = (x, y, height
    of the open shelf).  -> (ox, oy [n] int64 in the callers' order, state) or None when they do not fit."""
    w, h = np.asarray(w, np.int64), np.asarray(h, np.int64)
    order = np.lexsort((np.arange(len(w)), -w, -h))
    ox, oy = np.zeros(len(w), np.int64), np.zeros(len(w), np.int64)
    x, y, sh = state
    for c in order.tolist():
        wc, hc = int(w[c]), int(h[c])
        if wc > R:
            return None
        if x + wc > R:
            x, y, sh = 0, y + sh, 0
        if y + hc > R:
            return None
        ox[c], oy[c] = x, y
        x, sh = x + wc, max(sh, hc)
    return ox, oy, (x, y, sh)


def atlas_pack_error(R, n_charts, pad):
    side = int(np.ceil(np.sqrt(n_charts))) * (2 * pad + 2)
    return ValueError("chart_atlas: %d charts do not fit a %d x %d texture at any of %d scales; that many %d x %d "
                      "rectangles need resolution >= %d" % (n_charts, R, R, ATLAS_MAX_SHRINKS + 1, 2 * pad + 2,
                                                            2 * pad + 2, side))


def pack_charts(chart_box, R, pad, k0=0):
    """The scale search: the first k >= k0 at which the charts' rectangles shelf-pack into R x R.
    chart_box [C,4] f32 (p_lo, p_hi, q_lo, q_hi) -> (k, s, rect [C,4] int64 (ox, oy, w, h), shelf state)."""
    box = np.asarray(chart_box, np.float32).reshape(-1, 4).astype(np.float64)
    ext_p, ext_q = box[:, 1] - box[:, 0], box[:, 3] - box[:, 2]
    for k in range(k0, ATLAS_MAX_SHRINKS + 1):
        s = atlas_scale(ext_p, ext_q, R, pad, k)
        w, h = chart_rect_sizes(ext_p, ext_q, s, pad)
        placed = shelf_pack(w, h, R)
        if placed is not None:
            return k, s, np.stack([placed[0], placed[1], w, h], 1), placed[2]
    raise atlas_pack_error(R, len(box), pad)


def chart_atlas_with_info(verts, faces, resolution, pad=2):
    """chart_atlas plus the dict of raymarching.chart_atlas (face_chart, chart_rect, chart_axis, scale, k, ...)."""
    from .latent_nerf.raymarching import chart_atlas as op
    return op(verts, faces, resolution, pad)


def chart_atlas(verts, faces, resolution, pad=2):
    """UV atlas of connected patches: faces are grouped by the axis their normal is closest to, connected same-axis
    patches are projected along it and packed into the square at one texel density per world unit
    (raymarching.chart_atlas, on the GPU).  -> vt [n_vt,2] f32, ft [F,3] long, like per_triangle_atlas; neighbouring
    faces of a chart share their texture vertices."""
    vt, ft, _ = chart_atlas_with_info(verts, faces, resolution, pad)
    return vt, ft
