"""References for the batched, tile-culled rasteriser (lnerf_raster_prepare_batch / lnerf_rasterize_batch).

* `face_boxes`: the box rule of include/lnerf_hip.h in numpy f32, one rounding per operation, in the header's order.
* `restricted_rasterize`: oracle/raster_oracle.rasterize with the (pixel, face) pairs outside the boxes masked out --
  the contract of lnerf_rasterize_batch.  The oracle has no hook for a mask, so its expressions are restated here;
  tests/test_raster_batch_cpu.py pins the restatement to the oracle (whole-image boxes give RO.rasterize, torch.equal).
* the scenes and views the CPU and GPU tests share."""
import math
import os

import numpy as np
import torch

from oracle import raster_oracle as RO

SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")
EMPTY = (0, -1, 0, -1)
_F = np.float32


def face_boxes(H, W, face_z, face_xy):
    """face_z [F,3], face_xy [F,3,2] (torch or numpy, f32) -> int16 [F,4] = (j_lo, j_hi, i_lo, i_hi)."""
    z = np.asarray(face_z, dtype=np.float32)
    xy = np.asarray(face_xy, dtype=np.float32)
    x, y = xy[..., 0], xy[..., 1]
    one, half, Wf, Hf = _F(1.0), _F(0.5), _F(W), _F(H)
    with np.errstate(all="ignore"):
        rejected = ~((z[:, 0] < 0) & (z[:, 1] < 0) & (z[:, 2] < 0))
        area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
        rejected |= area == 0
        finite = np.isfinite(xy).all(axis=(1, 2))
        xmin, xmax, ymin, ymax = x.min(1), x.max(1), y.min(1), y.max(1)
        j_lo = np.maximum(np.floor(((xmin + one) * Wf - one) * half) - one, _F(0))
        j_hi = np.minimum(np.ceil(((xmax + one) * Wf - one) * half) + one, Wf - one)
        i_lo = np.maximum(np.floor(((one - ymax) * Hf - one) * half) - one, _F(0))
        i_hi = np.minimum(np.ceil(((one - ymin) * Hf - one) * half) + one, Hf - one)
    for a in (area, j_lo, j_hi, i_lo, i_hi):
        assert a.dtype == np.float32
    off = (j_lo > j_hi) | (i_lo > i_hi)
    box = np.zeros((z.shape[0], 4), dtype=np.int16)
    ok = finite & ~rejected & ~off
    for k, a in enumerate((j_lo, j_hi, i_lo, i_hi)):
        box[ok, k] = a[ok].astype(np.int16)
    box[~finite] = (0, W - 1, 0, H - 1)
    box[rejected | (finite & off)] = EMPTY           # the rejection comes first: it also covers a NaN depth
    return box


def whole_image_boxes(H, W, F):
    return np.tile(np.array([0, W - 1, 0, H - 1], dtype=np.int16), (F, 1))


def pair_mask(H, W, boxes):
    """bool [H*W, F]: pixel p = i*W + j lies in the box of face f."""
    b = torch.as_tensor(np.asarray(boxes, dtype=np.int64))
    j = torch.arange(W)[None, :].expand(H, W).reshape(-1, 1)
    i = torch.arange(H)[:, None].expand(H, W).reshape(-1, 1)
    return (j >= b[None, :, 0]) & (j <= b[None, :, 1]) & (i >= b[None, :, 2]) & (i <= b[None, :, 3])


def restricted_rasterize(H, W, face_z, face_xy, boxes):
    """RO.rasterize (same expressions, same order, f32) over the pairs inside the boxes only."""
    j = torch.arange(W, dtype=torch.float32)
    i = torch.arange(H, dtype=torch.float32)
    px = ((2 * j + 1) / W - 1)[None, :].expand(H, W).reshape(-1)
    py = (1 - (2 * i + 1) / H)[:, None].expand(H, W).reshape(-1)
    x0, y0 = face_xy[:, 0, 0][None], face_xy[:, 0, 1][None]
    x1, y1 = face_xy[:, 1, 0][None], face_xy[:, 1, 1][None]
    x2, y2 = face_xy[:, 2, 0][None], face_xy[:, 2, 1][None]
    PX, PY = px[:, None], py[:, None]
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    e0 = (x1 - PX) * (y2 - PY) - (x2 - PX) * (y1 - PY)
    e1 = (x2 - PX) * (y0 - PY) - (x0 - PX) * (y2 - PY)
    inv = 1.0 / area
    w0 = e0 * inv
    w1 = e1 * inv
    w2 = 1 - w0 - w1
    z0, z1, z2 = face_z[:, 0][None], face_z[:, 1][None], face_z[:, 2][None]
    ok = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (area != 0) & (z0 < 0) & (z1 < 0) & (z2 < 0)
    ok = ok & pair_mask(H, W, boxes)
    q0, q1, q2 = w0 / z0, w1 / z1, w2 / z2
    z = 1.0 / (q0 + q1 + q2)
    z = torch.where(ok, z, torch.full_like(z, -3.0e38))
    best_z = z.max(dim=1).values
    best_f = (z == best_z[:, None]).to(torch.uint8).argmax(dim=1)
    hit = best_z > -1.0e38
    idx = torch.where(hit, best_f, torch.full_like(best_f, -1))
    g = best_f[:, None]
    b = torch.stack([torch.gather(q0 * z, 1, g)[:, 0], torch.gather(q1 * z, 1, g)[:, 0],
                     torch.gather(q2 * z, 1, g)[:, 0]], -1)
    b = torch.where(hit[:, None], b, torch.zeros_like(b))
    return idx, b


def accepted_pairs(H, W, face_z, face_xy):
    """bool [H*W, F]: the pairs RO.rasterize's per-face test accepts (its `ok`, with a depth that can win)."""
    j = torch.arange(W, dtype=torch.float32)
    i = torch.arange(H, dtype=torch.float32)
    PX = ((2 * j + 1) / W - 1)[None, :].expand(H, W).reshape(-1, 1)
    PY = (1 - (2 * i + 1) / H)[:, None].expand(H, W).reshape(-1, 1)
    x0, y0 = face_xy[:, 0, 0][None], face_xy[:, 0, 1][None]
    x1, y1 = face_xy[:, 1, 0][None], face_xy[:, 1, 1][None]
    x2, y2 = face_xy[:, 2, 0][None], face_xy[:, 2, 1][None]
    area = (x1 - x0) * (y2 - y0) - (x2 - x0) * (y1 - y0)
    e0 = (x1 - PX) * (y2 - PY) - (x2 - PX) * (y1 - PY)
    e1 = (x2 - PX) * (y0 - PY) - (x0 - PX) * (y2 - PY)
    inv = 1.0 / area
    w0 = e0 * inv
    w1 = e1 * inv
    w2 = 1 - w0 - w1
    z0, z1, z2 = face_z[:, 0][None], face_z[:, 1][None], face_z[:, 2][None]
    return (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (area != 0) & (z0 < 0) & (z1 < 0) & (z2 < 0)


# ------------------------------------------------------------------------------------------------ shared scenes
def load_shape(name, normalise=True):
    """(verts f32 [V,3], faces long [F,3]) of tests/golden/shapes/<name>.obj; normalised to 0.6 and lifted by 0.25 as
    TexturedMeshModel does with the mesh it paints."""
    from src.latent_paint.models.mesh import Mesh
    m = Mesh(os.path.join(SHAPES, name + ".obj"))
    if normalise:
        m.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    return m.vertices.float().contiguous(), m.faces.long().contiguous()


def training_views(n, seed):
    """n seeded training poses (theta, phi, radius) from the trainer's own sampler."""
    from src.latent_paint.configs.train_config import TrainConfig
    from src.latent_paint.training.views_dataset import rand_poses
    cfg = TrainConfig().render
    g = torch.Generator().manual_seed(seed)
    views = []
    for _ in range(n):
        _, t, p, r = rand_poses(1, "cpu", radius_range=cfg.radius_range, angle_overhead=cfg.angle_overhead,
                                angle_front=cfg.angle_front, generator=g)
        views.append((t, p, r))
    return views


def oracle_prepare(verts, faces, view, dy=0.25):
    rot, pos = RO.camera_from_view(view[0], view[1], view[2], dy)
    return RO.prepare_vertices(verts, faces, rot, pos, math.pi / 3)
