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


