"""numpy restatement of the mesh-cleaning contract (include/lnerf_hip.h, "mesh cleaning"): connected components with the
library's numbering, boxes and counts, clean_mesh's keep rule in f64, the stable filter, Taubin smoothing with the
contract's order of summation, and the normals.  Written from the header's text, not from the kernels."""
import numpy as np

SMOOTH_LAMBDA, SMOOTH_MU = 0.5, -0.53


def _faces(faces, V):
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if len(f) and (f.min() < 0 or f.max() >= V):
        raise ValueError("face index outside [0, %d)" % V)
    return f


def _encode(x):
    """f32 -> u32 with the same order (-0 < +0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _decode(e):
    e = np.asarray(e, dtype=np.uint32)
    return np.where(e & np.uint32(0x80000000), e & np.uint32(0x7FFFFFFF), ~e).astype(np.uint32).view(np.float32)


def components(verts, faces):
    """-> dict(vert_comp [V] i32, face_comp [F] i32, comp_faces [C] i32, comp_box [C,6] f32, components, referenced)."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(verts)
    f = _faces(faces, V)
    parent = list(range(V))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union(a, b):
        a, b = find(a), find(b)
        if a != b:                    # the smaller index stays the root, so a root is its component's smallest vertex
            if a < b:
                parent[b] = a
            else:
                parent[a] = b

    for a, b, c in f.tolist():
        union(a, b)
        union(b, c)
    root = np.array([find(v) for v in range(V)], dtype=np.int64).reshape(-1)
    referenced = np.zeros(V, bool)
    referenced[f.reshape(-1)] = True
    roots = np.nonzero(referenced & (root == np.arange(V)))[0]          # ascending
    rank = np.full(V, -1, np.int64)
    rank[roots] = np.arange(len(roots))
    vert_comp = np.where(referenced, rank[root], -1).astype(np.int32)
    face_comp = vert_comp[f[:, 0]].astype(np.int32) if len(f) else np.zeros(0, np.int32)
    C = len(roots)
    comp_faces = np.bincount(face_comp, minlength=C).astype(np.int32) if C else np.zeros(0, np.int32)
    lo = np.full((C, 3), 0xFFFFFFFF, np.uint32)
    hi = np.zeros((C, 3), np.uint32)
    m = vert_comp >= 0
    enc = _encode(verts)
    for a in range(3):
        np.minimum.at(lo[:, a], vert_comp[m], enc[m, a])
        np.maximum.at(hi[:, a], vert_comp[m], enc[m, a])
    comp_box = np.concatenate([_decode(lo), _decode(hi)], 1).astype(np.float32).reshape(C, 6)
    return dict(vert_comp=vert_comp, face_comp=face_comp, comp_faces=comp_faces, comp_box=comp_box, components=C,
                referenced=int(referenced.sum()))


def keep_rule(comp_faces, comp_box, min_faces=0, min_diameter=0.0, keep_largest=0):
    """bool [C]: the components that stay."""
    n = [int(x) for x in comp_faces]
    box = np.asarray(comp_box, dtype=np.float32).reshape(-1, 6).astype(np.float64)
    C = len(n)
    if C == 0:
        return np.zeros(0, bool)

    def diag2(b):
        dx, dy, dz = b[3] - b[0], b[4] - b[1], b[5] - b[2]
        return (dx * dx + dy * dy) + dz * dz

    mesh = diag2(np.concatenate([box[:, :3].min(0), box[:, 3:].max(0)]))
    md = float(min_diameter)
    passing = [c for c in range(C) if n[c] >= min_faces and diag2(box[c]) >= (md * md) * mesh]
    if keep_largest > 0:
        passing = sorted(passing, key=lambda c: (-n[c], c))[:keep_largest]
    ok = np.zeros(C, bool)
    ok[passing] = True
    return ok


def mesh_filter(verts, faces, face_keep):
    """-> (verts [V',3] f32, faces [F',3] i32 re-indexed, vert_src [V'] i64), both in their old order."""
    verts = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(verts)
    f = _faces(faces, V)
    kept = f[np.asarray(face_keep).astype(bool)]
    used = np.zeros(V, bool)
    used[kept.reshape(-1)] = True
    vert_src = np.nonzero(used)[0]
    new = np.full(V, -1, np.int64)
    new[vert_src] = np.arange(len(vert_src))
    return verts[vert_src], new[kept].astype(np.int32).reshape(-1, 3), vert_src


def clean(verts, faces, min_faces=0, min_diameter=0.0, keep_largest=0):
    """-> (verts, faces, vert_src, info dict(components, kept, faces_before, faces_after))."""
    comp = components(verts, faces)
    ok = keep_rule(comp["comp_faces"], comp["comp_box"], min_faces, min_diameter, keep_largest)
    keep = ok[comp["face_comp"]] if len(comp["face_comp"]) else np.zeros(0, bool)
    v, f, src = mesh_filter(verts, faces, keep)
    return v, f, src, dict(components=comp["components"], kept=int(ok.sum()), faces_before=len(comp["face_comp"]),
                           faces_after=len(f))


def incidences(faces, V):
    """(inc [V, D] i64 = the values 3 f + k with faces[f][k] == v, ascending, -1 padded; deg [V]); faces that repeat an
    index are in no list."""
    f = _faces(faces, V)
    good = (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0]) if len(f) else np.zeros(0, bool)
    e = (3 * np.arange(len(f))[:, None] + np.arange(3)[None, :])[good].reshape(-1)
    v = f[good].reshape(-1)
    order = np.lexsort((e, v))
    e, v = e[order], v[order]
    deg = np.bincount(v, minlength=V).astype(np.int64) if V else np.zeros(0, np.int64)
    start = np.cumsum(deg) - deg
    D = int(deg.max()) if V and len(v) else 0
    inc = np.full((V, D), -1, np.int64)
    inc[v, np.arange(len(v)) - start[v]] = e
    return inc, deg


def _step(p, f, inc, deg, w):
    S = np.zeros(p.shape, np.float64)
    for r in range(inc.shape[1]):
        m = deg > r
        e = inc[m, r]
        ff, k = e // 3, e % 3
        S[m] = S[m] + p[f[ff, (k + 1) % 3]].astype(np.float64)
        S[m] = S[m] + p[f[ff, (k + 2) % 3]].astype(np.float64)
    out = p.copy()
    m = deg > 0
    mean = S[m] / (2 * deg[m]).astype(np.float64)[:, None]
    p64 = p[m].astype(np.float64)
    out[m] = (p64 + float(np.float32(w)) * (mean - p64)).astype(np.float32)
    return out


def normals(verts, faces, inc=None, deg=None):
    """lnerf_decimate's vertex normals over the incidence lists."""
    p = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
    V = len(p)
    f = _faces(faces, V)
    if inc is None:
        inc, deg = incidences(f, V)
    acc = np.zeros((V, 3), np.float32)
    if len(f):
        a, b = p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], -1).astype(np.float32)
        for r in range(inc.shape[1]):
            m = deg > r
            acc[m] = acc[m] + n[inc[m, r] // 3]
    l2 = acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2]
    with np.errstate(divide="ignore"):
        inv = np.where(l2 > 0, np.float32(1) / np.sqrt(l2), np.float32(0)).astype(np.float32)
    return (acc * inv[:, None]).astype(np.float32)


def smooth(verts, faces, iterations, lam=SMOOTH_LAMBDA, mu=SMOOTH_MU):
    """-> (verts [V,3] f32, normals [V,3] f32)."""
    if not (0 <= iterations <= 1000 and 0 < lam <= 1 and -1.5 <= mu <= 0):
        raise ValueError("smooth: arguments out of range")
    p = np.array(verts, dtype=np.float32).reshape(-1, 3)
    V = len(p)
    f = _faces(faces, V)
    inc, deg = incidences(f, V)
    for _ in range(iterations):
        for w in (lam, mu):
            if np.float32(w) != 0:
                p = _step(p, f, inc, deg, w)
    return p, normals(p, f, inc, deg)


# ---------------------------------------------------------------- the suites' meshes
BLOBS = (((0, 0, 0), 0.5), ((.8, .8, .8), .12), ((-.8, .7, -.6), .07), ((.75, -.8, .1), .2), ((-.85, -.85, -.85), .03),
         ((0, .85, 0), .09))


def _lattice(n):
    x = np.linspace(-1, 1, n, dtype=np.float32)
    return np.meshgrid(x, x, x, indexing="ij")


def floaters_volume(n=40):
    """max over BLOBS of r - |x - c| on the n^3 lattice over [-1, 1]^3 (iso 0): a body and five floaters."""
    X, Y, Z = _lattice(n)
    vol = np.full(X.shape, -np.inf, np.float32)
    for c, r in BLOBS:
        d = np.sqrt((X - np.float32(c[0])) ** 2 + (Y - np.float32(c[1])) ** 2 + (Z - np.float32(c[2])) ** 2)
        vol = np.maximum(vol, (np.float32(r) - d).astype(np.float32))
    return vol


def staircase_volume(n=40):
    """(|x| < 0.6) as 0 / 1 (iso 0.5): a sphere made of lattice steps."""
    X, Y, Z = _lattice(n)
    return (np.sqrt(X * X + Y * Y + Z * Z) < 0.6).astype(np.float32)
