"""Sketch-shape guidance (BASELINE config 3): a mesh given by `guide.shape_path`
(e.g. shapes/teddy.obj, scaled by `guide.mesh_scale`) biases the NeRF occupancy.  The reference's
README describes the knobs (`guide.proximal_surface`, `optim.lambda_shape`, README.md:140-142) and names igl
for the winding number (README.md:119-122); the code is absent from the checkout.

Here the generalised winding number and the unsigned distance are evaluated ONCE on a dense grid with
HIP kernels (csrc/mesh.hip); per-sample values are trilinear reads of those grids."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ..raymarching import backend as _b
from ..raymarching import raymarching as rm
from ..raymarching.raymarching import _chk, _p, _stream


def load_obj(path):
    """Plain-text OBJ reader (no kaolin): `v x y z` and `f i[/j[/k]] ...` records, negative indices,
    polygons as triangle fans.  Returns (vertices float32 [V,3], faces int64 [F,3])."""
    verts, faces = [], []
    with open(path) as f:
        for line in f:
            if line.startswith("v "):
                verts.append([float(x) for x in line.split()[1:4]])
            elif line.startswith("f "):
                idx = []
                for tok in line.split()[1:]:
                    i = int(tok.split("/")[0])
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[k], idx[k + 1]])
    if not verts or not faces:
        raise ValueError("%s: no geometry found" % path)
    return torch.tensor(verts, dtype=torch.float32), torch.tensor(faces, dtype=torch.int64)


def normalize_mesh(verts, target_scale=1.0, dy=0.0):
    """Centre on the vertex mean, scale the farthest vertex to `target_scale`, lift by dy
    (src/latent_paint/models/mesh.py:37-48)."""
    v = verts - verts.mean(dim=0)
    v = v / torch.max(torch.norm(v, p=2, dim=1))
    v = v * target_scale
    v[:, 1] += dy
    return v


def make_icosphere(subdiv=2, radius=1.0):
    t = (1.0 + math.sqrt(5.0)) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        cache, nf = {}, []

        def mid(a, b):
            key = (min(a, b), max(a, b))
            if key not in cache:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                cache[key] = len(v) - 1
            return cache[key]

        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return torch.tensor(np.array(v) * radius, dtype=torch.float32), torch.tensor(f, dtype=torch.int64)


def mesh_winding_number(points, triangles):
    points = points.contiguous()
    out = torch.empty(points.shape[0], device=points.device)
    _b.call("lnerf_mesh_winding_number", _chk(points, "points"), points.shape[0], _chk(triangles, "triangles"),
            triangles.shape[0], _p(out), _stream())
    return out


def mesh_distance(points, triangles):
    points = points.contiguous()
    out = torch.empty(points.shape[0], device=points.device)
    _b.call("lnerf_mesh_distance", _chk(points, "points"), points.shape[0], _chk(triangles, "triangles"),
            triangles.shape[0], _p(out), _stream())
    return out


class MeshOccupancy:
    """Dense winding-number and distance grids of a mesh over [-bound, bound]^3 (R^3 voxels, values at voxel
    centres), built once on the GPU."""

    def __init__(self, verts, faces, device, bound=1.0, resolution=128):
        self.bound, self.R = float(bound), int(resolution)
        self.triangles = verts.to(device)[faces.to(device)].contiguous().float()  # [F,3,3]
        R = self.R
        lin = ((torch.arange(R, device=device, dtype=torch.float32) + 0.5) / R * 2.0 - 1.0) * self.bound
        zz, yy, xx = torch.meshgrid(lin, lin, lin, indexing="ij")
        pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).contiguous()
        self.winding = mesh_winding_number(pts, self.triangles).reshape(1, 1, R, R, R)
        self.dist = mesh_distance(pts, self.triangles).reshape(1, 1, R, R, R)

    def _sample(self, vol, xyzs):
        g = (xyzs / self.bound).reshape(1, 1, 1, -1, 3)  # grid_sample wants (x, y, z) in [-1, 1]
        return F.grid_sample(vol, g, mode="bilinear", padding_mode="border", align_corners=False).reshape(-1)

    def winding_at(self, xyzs):
        return self._sample(self.winding, xyzs)

    def distance_at(self, xyzs):
        return self._sample(self.dist, xyzs)

    def init_density_grid(self, renderer, inside_value=None):
        """Seed the renderer's occupancy grid from the mesh: cells whose centre is inside (winding > 0.5)
        get `inside_value` (default 2 x density_thresh), the rest 0; then repack the bitfield.
        (BASELINE config 3: 'mesh winding-number occupancy in march'.)"""
        G = renderer.grid_size
        dev = renderer.density_grid.device
        val = 2.0 * renderer.density_thresh if inside_value is None else float(inside_value)
        for cas in range(renderer.cascade):
            xyz = torch.empty(G ** 3, 3, device=dev)
            _b.call("lnerf_occ_cell_points", None, G ** 3, cas, G, renderer.bound, None, _p(xyz), _stream())
            w = mesh_winding_number(xyz, self.triangles)
            renderer.density_grid[cas] = torch.where(w > 0.5, torch.full_like(w, val), torch.zeros_like(w))
        renderer.mean_density_dev.fill_(float(renderer.density_grid.clamp(min=0).mean()))
        rm.packbits(renderer.density_grid, renderer.density_thresh, renderer.density_bitfield, renderer.mean_density_dev)
        return renderer.density_bitfield


class ShapeLoss:
    """Shape prior on the NeRF occupancy.  PARITY UNPINNED: the reference ships no shape loss (src/latent_nerf is absent,
    README.md:140-142 only documents the knobs `guide.proximal_surface` and `optim.lambda_shape`); the form below is the
    upstream one as recalled in SURVEY.md Appendix A, chosen deliberately so that the advertised default
    `lambda_shape = 5e-6` (demo_configs/latent_nerf/lego_man.yaml) has the effect it was tuned for:

        nerf_occ  = clamp(1 - exp(-delta sigma), 0, 1.1),  delta = 0.2
        indicator = [winding number > 0.5]
        CE(p = nerf_occ, q = indicator)  = -(p log clamp(q) + (1 - p) log clamp(1 - q)),  clamp to [0.01, 0.99]
        loss = SUM over the samples of  CE x (1 - exp(-d^2 / (2 proximal_surface^2)))

    i.e. the cross-entropy takes the NeRF occupancy as its FIRST argument (linear in nerf_occ: a constant pull
    of log(0.99/0.01) per sample towards the indicator, the indicator itself is not optimised), it is SUMMED over the
    M ~ 1e5..4e5 samples of the view (not averaged), and samples near the surface are down-weighted by their
    distance d to the mesh."""

    def __init__(self, occ: MeshOccupancy, proximal_surface=0.3, delta=0.2):
        self.occ, self.proximal_surface, self.delta = occ, proximal_surface, delta

    def __call__(self, xyzs, sigmas, counter=None):
        """xyzs [cap,3], sigmas [cap] (capacity-sized), counter: device int32 whose [0] is the valid count."""
        n = xyzs.shape[0]
        valid = torch.ones(n, dtype=torch.bool, device=xyzs.device) if counter is None else \
            torch.arange(n, device=xyzs.device) < counter[0]
        x = torch.where(valid[:, None], xyzs, torch.zeros_like(xyzs))
        inside = (self.occ.winding_at(x) > 0.5).float()
        sig = torch.where(valid, sigmas, torch.zeros_like(sigmas))  # never read the uninitialised tail
        nerf_occ = (1.0 - torch.exp(-self.delta * sig)).clamp(0.0, 1.1)
        ce = -(nerf_occ * torch.log(inside.clamp(0.01, 0.99)) + (1.0 - nerf_occ) * torch.log((1.0 - inside).clamp(0.01, 0.99)))
        if self.proximal_surface > 0:
            d = self.occ.distance_at(x)
            # -expm1, not 1 - exp: near the surface the weight is ~d^2 and 1 - exp leaves it an absolute error of 2^-24
            ce = ce * -torch.expm1(-(d * d) / (2.0 * self.proximal_surface ** 2))
        return torch.where(valid, ce, torch.zeros_like(ce)).sum()
