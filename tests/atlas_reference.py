"""numpy restatement of the chart atlas (include/lnerf_hip.h "chart atlas", raymarching.chart_atlas): buckets, links,
labels, boxes, the scale search and shelf packing, UVs and the strict-coverage eviction, with the same f32 operations
in the same order, so vt, ft, face_chart, chart_rect, chart_axis, scale, k and the evicted set compare bit for bit
with the op.  Also the test meshes both atlas test files share."""
import functools

import numpy as np

from tests import uv_reference as U

f32 = np.float32
SHRINK, MAX_SHRINKS = 0.95, 200
AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
PLANE = ((1, 2), (2, 1), (2, 0), (0, 2), (0, 1), (1, 0))      # coordinate indices of (p, q) per bucket


# ------------------------------------------------------------------------------ stages
def buckets(verts, faces):
    """bucket [F] (first maximum of (m_x, -m_x, m_y, -m_y, m_z, -m_z); 0 for m = 0 or NaN)."""
    P = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    with np.errstate(all="ignore"):
        mx = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]
        my = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]
        mz = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    score = [mx, -mx, my, -my, mz, -mz]
    bk, best = np.zeros(len(P), np.int32), score[0].copy()
    for k in range(1, 6):
        better = score[k] > best
        best = np.where(better, score[k], best)
        bk = np.where(better, k, bk).astype(np.int32)
    return bk


def twins(faces):
    """twin [3F]: the opposite half-edge where the undirected edge has exactly two half-edges, one each way; else -1."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    groups = {}
    for e, (a, b) in enumerate(zip(faces.reshape(-1).tolist(), faces[:, [1, 2, 0]].reshape(-1).tolist())):
        groups.setdefault((min(a, b), max(a, b)), []).append((e, a < b))
    twin = np.full(3 * len(faces), -1, np.int32)
    for (lo, hi), g in groups.items():
        if len(g) == 2 and lo != hi and g[0][1] != g[1][1]:
            twin[g[0][0]], twin[g[1][0]] = g[1][0], g[0][0]
    return twin


def labels(bucket, twin):
    """label [F]: the smallest face index of the face's component (linked and same bucket)."""
    F = len(bucket)
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for e in np.flatnonzero(twin >= 0).tolist():
        f, g = e // 3, int(twin[e]) // 3
        if bucket[f] == bucket[g]:
            a, b = find(f), find(g)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(f) for f in range(F)], np.int32)


def _encode(v):
    u = np.asarray(v, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _decode(e):
    e = np.asarray(e, np.uint32)
    return np.where(e & np.uint32(0x80000000), e & np.uint32(0x7FFFFFFF), ~e).astype(np.uint32).view(np.float32)


def plane_coords(verts, faces, bucket):
    """(p, q) [F,3] f32 of every face corner in its face's bucket."""
    P = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]          # [F,3,3]
    pi = np.array([PLANE[b][0] for b in bucket], np.int64)
    qi = np.array([PLANE[b][1] for b in bucket], np.int64)
    rows = np.arange(len(P))[:, None]
    return P[rows, np.arange(3)[None], pi[:, None]], P[rows, np.arange(3)[None], qi[:, None]]


def boxes(p, q, face_chart, C):
    """[C,4] f32 (p_lo, p_hi, q_lo, q_hi) through the order-preserving integer encoding (so -0 < +0)."""
    enc = np.stack([np.full(C, 0xFFFFFFFF, np.uint32), np.zeros(C, np.uint32)] * 2)
    fc = np.repeat(np.asarray(face_chart, np.int64), 3)
    ep, eq = _encode(p).reshape(-1), _encode(q).reshape(-1)
    np.minimum.at(enc[0], fc, ep)
    np.maximum.at(enc[1], fc, ep)
    np.minimum.at(enc[2], fc, eq)
    np.maximum.at(enc[3], fc, eq)
    return np.stack([_decode(e) for e in enc], 1)


def scale_at(ext_p, ext_q, R, pad, k):
    m = max([0.0] + [float(x) for x in ext_p] + [float(x) for x in ext_q])
    s0 = (R - 2 * pad - 2) / m if m > 0 else 1.0
    return float(f32(s0 * SHRINK ** k))


def rect_sizes(box, s, pad):
    box = np.asarray(box, np.float32).reshape(-1, 4).astype(np.float64)
    w = 2 * pad + 2 + np.floor((box[:, 1] - box[:, 0]) * s).astype(np.int64)
    h = 2 * pad + 2 + np.floor((box[:, 3] - box[:, 2]) * s).astype(np.int64)
    return w, h


def shelf_pack(w, h, R, state=(0, 0, 0)):
    """Rectangles in the order (h desc, w desc, index asc) onto shelves -> (ox, oy, state) or None."""
    order = sorted(range(len(w)), key=lambda c: (-int(h[c]), -int(w[c]), c))
    ox, oy = np.zeros(len(w), np.int64), np.zeros(len(w), np.int64)
    x, y, sh = state
    for c in order:
        if w[c] > R:
            return None
        if x + w[c] > R:
            x, y, sh = 0, y + sh, 0
        if y + h[c] > R:
            return None
        ox[c], oy[c] = x, y
        x, sh = x + int(w[c]), max(sh, int(h[c]))
    return ox, oy, (x, y, sh)


def pack(box, R, pad, k0=0):
    """First k >= k0 that packs -> (k, s, rect [C,4], state); ValueError past MAX_SHRINKS."""
    b = np.asarray(box, np.float32).reshape(-1, 4).astype(np.float64)
    ext_p, ext_q = b[:, 1] - b[:, 0], b[:, 3] - b[:, 2]
    for k in range(k0, MAX_SHRINKS + 1):
        s = scale_at(ext_p, ext_q, R, pad, k)
        w, h = rect_sizes(box, s, pad)
        placed = shelf_pack(w, h, R)
        if placed is not None:
            return k, s, np.stack([placed[0], placed[1], w, h], 1), placed[2]
    raise ValueError("no scale packs %d charts into %d" % (len(b), R))


def emit(p, q, faces, face_chart, rect, box, s, R, pad, V):
    """vt [n_vt,2] f32, ft [F,3]: one texture vertex per distinct (chart, vertex) pair, ascending."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    fc = np.asarray(face_chart, np.int64)
    key = (fc[:, None] * max(V, 1) + faces).reshape(-1)
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    c = np.repeat(fc, 3)[first]
    pp, qq = p.reshape(-1)[first], q.reshape(-1)[first]
    box = np.asarray(box, np.float32).reshape(-1, 4)
    s, Rf = f32(s), f32(R)
    x0 = (rect[c, 0] + pad).astype(np.float32) + f32(0.5)
    y0 = (rect[c, 1] + pad).astype(np.float32) + f32(0.5)
    X = x0 + (pp - box[c, 0]) * s
    Y = y0 + (box[c, 3] - qq) * s
    vt = np.stack([X / Rf, f32(1.0) - Y / Rf], 1).astype(np.float32)
    return vt, inv.reshape(-1, 3).astype(np.int64)


def _strict_items(vt, ft, R):
    """Every (face, candidate texel) with strict coverage: f, linear texel index."""
    ft = np.asarray(ft, np.int64).reshape(-1, 3)
    X, Y, area, box, _ = U.face_setup(np.zeros((1, 3), np.float32), np.zeros_like(ft), vt, ft, R)
    j0, i0, w, h = box
    items = w * h
    f = np.repeat(np.arange(len(items)), items)
    local = np.arange(int(items.sum()), dtype=np.int64) - (np.cumsum(items) - items)[f]
    di = local // np.maximum(w[f], 1)
    i, j = i0[f] + di, j0[f] + (local - di * w[f])
    _, e = U._covered(X[:, f], Y[:, f], area[f], i, j)
    strict = np.where(area[f] > 0, (e[0] > 0) & (e[1] > 0) & (e[2] > 0), (e[0] < 0) & (e[1] < 0) & (e[2] < 0))
    return f[strict], (i * R + j)[strict]


def strict_coverage_count(vt, ft, R):
    """[R,R]: how many faces strictly contain each texel centre."""
    _, t = _strict_items(vt, ft, R)
    return np.bincount(t, minlength=R * R).reshape(R, R)


def evicted_faces(vt, ft, R):
    """Faces that strictly cover a texel centre which a face with a larger index strictly covers too (ascending)."""
    f, t = _strict_items(vt, ft, R)
    owner = np.full(R * R, -1, np.int64)
    np.maximum.at(owner, t, f)
    return np.unique(f[owner[t] != f])


def chart_atlas(verts, faces, R, pad=2, fold_check=True):
    """The whole pipeline -> dict(vt, ft, face_chart, chart_rect, chart_axis, scale, k, evicted (face indices), n_base)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = len(verts), len(faces)
    if ((faces < 0) | (faces >= V)).any():
        raise ValueError("%d faces index outside verts" % int(((faces < 0) | (faces >= V)).any(1).sum()))
    bk = buckets(verts, faces)
    lab = labels(bk, twins(faces))
    roots = np.flatnonzero(lab == np.arange(F))
    face_chart = np.searchsorted(roots, lab).astype(np.int32)
    axis = bk[roots].astype(np.int32)
    C = len(roots)
    p, q = plane_coords(verts, faces, bk)
    box = boxes(p, q, face_chart, C)
    k = 0
    while True:
        k, s, rect, state = pack(box, R, pad, k)
        vt, ft = emit(p, q, faces, face_chart, rect, box, s, R, pad, V)
        ev = evicted_faces(vt, ft, R) if fold_check else np.zeros(0, np.int64)
        fc, ax, bx = face_chart, axis, box
        if len(ev):
            ebox = boxes(p[ev], q[ev], np.arange(len(ev)), len(ev))
            w, h = rect_sizes(ebox, s, pad)
            placed = shelf_pack(w, h, R, state)
            if placed is None:
                k += 1
                if k > MAX_SHRINKS:
                    raise ValueError("no scale packs %d charts into %d" % (C + len(ev), R))
                continue
            rect = np.concatenate([rect, np.stack([placed[0], placed[1], w, h], 1)], 0)
            fc = face_chart.copy()
            fc[ev] = C + np.arange(len(ev))
            ax, bx = np.concatenate([axis, bk[ev]]).astype(np.int32), np.concatenate([box, ebox])
            vt, ft = emit(p, q, faces, fc, rect, bx, s, R, pad, V)
        return dict(vt=vt, ft=ft, face_chart=fc, chart_rect=rect.astype(np.int32), chart_axis=ax, scale=s, k=k,
                    evicted=ev, n_base=C, chart_box=bx, bucket=bk)


def bilinear(texture, uv):
    """texture [C,R,R] at uv [N,2] -> [N,C]: grid_sample(bilinear, align_corners=False, zero padding) on (u, 1 - v),
    the texel convention of lnerf_uv_raster and lnerf_texture_map_forward, in f64."""
    tex = np.asarray(texture, np.float64)
    C, R, _ = tex.shape
    x = np.asarray(uv, np.float64)[:, 0] * R - 0.5
    y = (1.0 - np.asarray(uv, np.float64)[:, 1]) * R - 0.5
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    out = np.zeros((len(x), C))
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = x0 + dx, y0 + dy
            wgt = (1 - np.abs(x - xi)) * (1 - np.abs(y - yi))
            ok = (xi >= 0) & (xi < R) & (yi >= 0) & (yi < R)
            out += np.where(ok, wgt, 0.0)[:, None] * tex[:, np.clip(yi, 0, R - 1), np.clip(xi, 0, R - 1)].T
    return out


# ------------------------------------------------------------------------------ properties
def uv_area(vt, ft):
    t = np.asarray(vt, np.float64)[np.asarray(ft, np.int64)]
    a, b = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    return 0.5 * (a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


def world_area(verts, faces):
    P = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)


def check_properties(verts, faces, res, R, pad=2):
    """The properties every atlas must have (asserts); `res`: chart_atlas's dict, or the op's with numpy values."""
    vt, ft, fc, rect, s = res["vt"], np.asarray(res["ft"], np.int64), np.asarray(res["face_chart"], np.int64), \
        np.asarray(res["chart_rect"], np.int64), res["scale"]
    V = len(verts)
    a3, a2 = world_area(verts, faces), uv_area(vt, ft) * R * R        # a2 in texels^2
    # A pixel coordinate X = x0 + (p - p_lo) * s, u = X / R and back carries at most 8 f32 roundings of numbers <= R:
    # |dX| <= d = 8 R 2^-24 texels.  Moving every corner by d changes a triangle's area by at most d * perimeter.
    t = np.asarray(vt, np.float64)[ft] * R
    per = sum(np.linalg.norm(t[:, k] - t[:, (k + 1) % 3], axis=1) for k in range(3))
    tol = 8 * R * 2.0 ** -24 * (per + 1)
    exact = a3 * s * s                                                  # the face's own area at the atlas scale
    solid = exact / np.sqrt(3) > tol                                    # faces whose sign rounding cannot turn
    assert (a2[solid] > 0).all()
    assert (a2 <= exact + tol).all(), float((a2 - exact - tol).max())
    assert (a2 >= exact / np.sqrt(3) - tol).all(), float((exact / np.sqrt(3) - tol - a2).max())
    ratio = a2[solid] / exact[solid]
    assert strict_coverage_count(vt, ft, R).max() <= 1
    assert (rect[:, :2] >= 0).all() and (rect[:, 0] + rect[:, 2] <= R).all() and (rect[:, 1] + rect[:, 3] <= R).all()
    occ = np.zeros((R, R), np.int32)
    for ox, oy, w, h in rect.tolist():
        occ[oy:oy + h, ox:ox + w] += 1
    assert occ.max() <= 1                                             # rectangles of different charts are disjoint
    X, Y = vt[:, 0].astype(np.float64) * R, (1 - vt[:, 1].astype(np.float64)) * R
    c = np.zeros(len(vt), np.int64)
    c[ft.reshape(-1)] = np.repeat(fc, 3)
    assert (np.repeat(fc, 3) == c[ft.reshape(-1)]).all()              # ft indexes only vt rows of its own chart
    eps = 1e-3
    assert (X >= rect[c, 0] + pad - eps).all() and (X <= rect[c, 0] + rect[c, 2] - pad + eps).all()
    assert (Y >= rect[c, 1] + pad - eps).all() and (Y <= rect[c, 1] + rect[c, 3] - pad + eps).all()
    pairs = np.unique(np.repeat(fc, 3) * max(V, 1) + np.asarray(faces, np.int64).reshape(-1))
    assert len(vt) == len(pairs) and len(np.unique(ft)) == len(vt)
    return ratio


# ------------------------------------------------------------------------------ meshes
def _lattice(n):
    ax = f32(-1) + (f32(2) * np.arange(n, dtype=np.float32)) / f32(n - 1)
    return np.meshgrid(ax, ax, ax, indexing="ij")


def field(name, n):
    """The marching-cubes test volumes: sphere, torus, bumpy blob on [-1, 1]^3 at n^3."""
    X, Y, Z = _lattice(n)
    if name == "sphere":
        return (0.55 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    if name == "torus":
        return (0.2 - np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)).astype(np.float32)
    if name == "blob":
        return (0.6 - np.sqrt(X * X + Y * Y + Z * Z) + 0.04 * np.sin(9 * X) * np.sin(9 * Y) * np.sin(9 * Z)).astype(np.float32)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mc_mesh(name, n):
    from tests import mc_reference as M
    v, f, _ = M.marching_cubes(field(name, n), 0.0, (-1, -1, -1), (1, 1, 1))
    return v, f.astype(np.int32)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)      # index 4x + 2y + z
    q = [(4, 6, 7, 5), (0, 1, 3, 2), (2, 3, 7, 6), (0, 4, 5, 1), (1, 5, 7, 3), (0, 2, 6, 4)]   # +x -x +y -y +z -z
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int32)


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, np.int32)


def helicoid(n_r=4, n_t=48, r0=0.3, r1=0.8, turns=2.5, rise=1.0):
    """A ramp winding 2.5 times about +y, normals up: one +y chart that covers itself up to three times."""
    r = np.linspace(r0, r1, n_r + 1)
    t = np.linspace(0.0, 2 * np.pi * turns, n_t + 1)
    rr, tt = np.meshgrid(r, t, indexing="ij")
    v = np.stack([rr * np.cos(tt), rise * tt / (2 * np.pi * turns) - 0.5, rr * np.sin(tt)], -1).reshape(-1, 3)
    idx = lambda i, j: i * (n_t + 1) + j
    f = []
    for i in range(n_r):
        for j in range(n_t):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            f += [(a, c, b), (a, d, c)]
    return v.astype(np.float32), np.array(f, np.int32)


def topology_zoo():
    """Stacked squares, a three-face fan on one edge, an open strip, a zero-area face and a face repeated reversed."""
    v, f = [], []

    def add(pts, tris):
        o = len(v)
        v.extend(pts)
        f.extend([tuple(o + i for i in t) for t in tris])

    sq = [(0, 0), (1, 0), (1, 1), (0, 1)]
    add([(x, y, 0.0) for x, y in sq], [(0, 1, 2), (0, 2, 3)])                       # two stacked squares facing +z
    add([(x, y, 0.5) for x, y in sq], [(0, 1, 2), (0, 2, 3)])
    add([(3, 0, 0), (3, 1, 0), (4, 0.5, 0.2), (2, 0.5, 0.2), (3, 0.5, 1)],          # three faces on the edge 0-1
        [(0, 1, 2), (1, 0, 3), (0, 1, 4)])
    add([(x, y, 2.0 + 0.1 * x) for x in range(5) for y in (0, 1)],                  # an open strip of 4 quads
        [t for i in range(4) for t in ((2 * i, 2 * i + 2, 2 * i + 3), (2 * i, 2 * i + 3, 2 * i + 1))])
    add([(6, 0, 0), (7, 0, 0), (8, 0, 0)], [(0, 1, 2)])                             # zero area
    add([(6, 2, 0), (7, 2, 0), (6, 3, 0.3)], [(0, 1, 2), (0, 2, 1)])                # one face twice, reversed
    return np.array(v, np.float32), np.array(f, np.int32)
