"""numpy restatement of lnerf_marching_cubes (include/lnerf_hip.h): same tables, same vertex / triangle order, the same
f32 arithmetic in the same order, so vertices and faces compare bit for bit with the HIP op."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_generator():
    spec = importlib.util.spec_from_file_location("gen_mc_tables", os.path.join(ROOT, "tools", "gen_mc_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_TABLES = None


def tables():
    """(tri_count [256] int, tris [256, MAXT, 3] int (-1 padded), edge_corners [12, 2])."""
    global _TABLES
    if _TABLES is None:
        g = load_generator()
        tabs = g.tables()
        maxt = max(len(t) for t in tabs)
        tris = -np.ones((256, maxt, 3), np.int64)
        for c, t in enumerate(tabs):
            if t:
                tris[c, :len(t)] = np.array(t)
        _TABLES = (np.array([len(t) for t in tabs]), tris, np.array(g.EDGES))
    return _TABLES


def _coords(lo, hi, n):
    lo, hi = np.float32(lo), np.float32(hi)
    i = np.arange(n, dtype=np.float32)
    return lo + ((hi - lo) * i) / np.float32(n - 1)


def _gradient(vol, cs):
    """Per-axis differences at every lattice point: central inside, one-sided at the border, over world spacing."""
    g = []
    for a in range(3):
        n = vol.shape[a]
        i = np.arange(n)
        lo_i, hi_i = np.maximum(i - 1, 0), np.minimum(i + 1, n - 1)
        dv = np.take(vol, hi_i, axis=a) - np.take(vol, lo_i, axis=a)
        dc = cs[a][hi_i] - cs[a][lo_i]
        shape = [1, 1, 1]
        shape[a] = n
        g.append(dv / dc.reshape(shape))
    return np.stack(g, -1).astype(np.float32)


def marching_cubes(vol, iso, lo, hi, close_boundary=True):
    """vol [nx, ny, nz] (z fastest) -> (verts [V,3] f32, faces [F,3] i32, normals [V,3] f32)."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    iso = np.float32(iso)
    n = vol.shape
    assert all(k >= 2 for k in n)
    cs = [_coords(lo[a], hi[a], n[a]) for a in range(3)]
    grad = _gradient(vol, cs)
    p = 1 if close_boundary else 0
    # working lattice: the volume, with one layer of outside (NaN) points around it under close_boundary
    W = tuple(k + 2 * p for k in n)
    wv = np.full(W, np.nan, np.float32)
    wv[p:p + n[0], p:p + n[1], p:p + n[2]] = vol
    wg = np.zeros(W + (3,), np.float32)
    wg[p:p + n[0], p:p + n[1], p:p + n[2]] = grad
    wc = []
    for a in range(3):   # coordinates of the working indices (outside points are never used: vertices snap)
        c = np.zeros(W[a], np.float32)
        c[p:p + n[a]] = cs[a]
        wc.append(c)
    inside = wv > iso
    # ---- vertices: crossed +x/+y/+z edges of every working point, in (point, axis) order
    crossed = np.zeros(W + (3,), bool)
    for a in range(3):
        sl0 = [slice(None)] * 3
        sl1 = [slice(None)] * 3
        sl0[a] = slice(0, W[a] - 1)
        sl1[a] = slice(1, W[a])
        sl0, sl1 = tuple(sl0), tuple(sl1)
        crossed[sl0 + (a,)] = inside[sl0] != inside[sl1]
    flat = crossed.reshape(-1)
    vid = np.cumsum(flat) - 1
    idx = np.nonzero(flat)[0]
    pt, axis = idx // 3, idx % 3
    I, J, K = np.unravel_index(pt, W)
    P0 = np.stack([I, J, K], -1)
    P1 = P0.copy()
    P1[np.arange(len(axis)), axis] += 1
    v0 = wv[P0[:, 0], P0[:, 1], P0[:, 2]]
    v1 = wv[P1[:, 0], P1[:, 1], P1[:, 2]]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t = (iso - v0) / (v1 - v0)
        ok = (t >= 0) & (t <= 1)
        in0 = v0 > iso
        t = np.where(ok, t, np.where(in0, np.float32(0), np.float32(1))).astype(np.float32)
        verts = np.empty((len(idx), 3), np.float32)
        for a in range(3):
            x0 = wc[a][P0[:, a]]
            on = axis == a
            x1 = wc[a][np.minimum(P1[:, a], W[a] - 1)]
            interp = x0 + t * (x1 - x0)
            snapped = np.where(in0, x0, x1)
            verts[:, a] = np.where(on, np.where(ok, interp, snapped), x0)
        g0 = wg[P0[:, 0], P0[:, 1], P0[:, 2]]
        g1 = wg[P1[:, 0], P1[:, 1], P1[:, 2]]
        nrm = g0 + t[:, None] * (g1 - g0)
        nrm = np.where(ok[:, None], nrm, np.where(in0[:, None], g0, g1))
        l2 = nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2]
        inv = np.where(l2 > 0, np.float32(1) / np.sqrt(l2), np.float32(0)).astype(np.float32)
        normals = (-nrm * inv[:, None]).astype(np.float32)
    # ---- triangles: cells in order of their corner 0, table order within a cell
    count, tris, ecorners = tables()
    C = tuple(k - 1 for k in W)
    case = np.zeros(C, np.int64)
    for c in range(8):
        x, y, z = c & 1, (c >> 1) & 1, (c >> 2) & 1
        case |= inside[x:x + C[0], y:y + C[1], z:z + C[2]].astype(np.int64) << c
    case = case.reshape(-1)
    nt = count[case]
    cells = np.repeat(np.arange(case.size), nt)
    rank = np.arange(cells.size) - np.repeat(np.cumsum(nt) - nt, nt)
    edges = tris[case[cells], rank]                        # [F, 3]
    ci, cj, ck = np.unravel_index(cells, C)
    vid3 = vid.reshape(W + (3,))
    faces = np.empty(edges.shape, np.int64)
    for j in range(3):
        e = edges[:, j]
        c0 = ecorners[e, 0]
        faces[:, j] = vid3[ci + (c0 & 1), cj + ((c0 >> 1) & 1), ck + ((c0 >> 2) & 1), e // 4]
    return verts, faces.astype(np.int32), normals


# ---------------------------------------------------------------- mesh checks used by the tests
def directed_edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def is_closed_oriented_manifold(faces):
    """Every directed edge appears exactly once and its reverse exactly once."""
    d = directed_edges(faces)
    if len(d) == 0:
        return True
    key = d[:, 0] * (1 << 32) + d[:, 1]
    rkey = d[:, 1] * (1 << 32) + d[:, 0]
    if len(np.unique(key)) != len(key):
        return False
    return bool(np.isin(rkey, key).all())


def euler_characteristic(verts, faces):
    d = directed_edges(faces)
    und = np.unique(np.sort(d, axis=1), axis=0)
    used = np.unique(np.asarray(faces).reshape(-1))
    return len(used) - len(und) + len(faces)


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)
