"""numpy restatement of lnerf_decimate (include/lnerf_hip.h): rounds of independent quadric-error edge collapses with the
same quadrics, candidate keys, validity checks, selection and compaction as the HIP op, the same f64 / f32 arithmetic in
the same order, so vertices, faces and normals compare bit for bit with it."""
import numpy as np

SINGULAR_REL = 1e-10      # LNERF_DECIMATE_SINGULAR_REL: solve iff |det| > SINGULAR_REL * tr^3
KEY_NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
DEFAULT_MAX_ROUNDS = 128  # LNERF_DECIMATE_DEFAULT_ROUNDS


def edge_tag(e):
    """The key's low word: a fixed bijection of the 32-bit edge id (multiply by odd constants, xor-shift), so that equal
    costs (every cost of a flat region is 0) do not order themselves along the lattice."""
    x = np.asarray(e).astype(np.uint32)
    x = x * np.uint32(0x9E3779B1)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    return x


def _fan(faces, V):
    """Vertex -> incident faces, ascending: (fan [V, D] int64, -1 padded; deg [V])."""
    F = len(faces)
    w = faces.reshape(-1)
    f = np.repeat(np.arange(F), 3)
    order = np.lexsort((f, w))
    w, f = w[order], f[order]
    deg = np.bincount(w, minlength=V)
    D = max(int(deg.max()) if V else 0, 1)
    start = np.concatenate([[0], np.cumsum(deg)[:-1]])
    slot = np.arange(len(w)) - start[w]
    fan = -np.ones((V, D), np.int64)
    fan[w, slot] = f
    return fan, deg


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def face_quadrics(pos, faces):
    """[F, 10] f64: area * (n0n0, n0n1, n0n2, n1n1, n1n2, n2n2, n0d, n1d, n2d, dd) of each face's plane n.x + d = 0."""
    p = pos[faces].astype(np.float64)
    n = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.sqrt(_dot(n, n))
    zero = ln == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        u = n / ln[:, None]
        d = -_dot(u, p[:, 0])
        w = ln * 0.5
        q = np.stack([w * (u[:, 0] * u[:, 0]), w * (u[:, 0] * u[:, 1]), w * (u[:, 0] * u[:, 2]),
                      w * (u[:, 1] * u[:, 1]), w * (u[:, 1] * u[:, 2]), w * (u[:, 2] * u[:, 2]),
                      w * (u[:, 0] * d), w * (u[:, 1] * d), w * (u[:, 2] * d), w * (d * d)], -1)
    q[zero] = 0.0
    return q


def vertex_quadrics(pos, faces):
    V = len(pos)
    fan, deg = _fan(faces, V)
    qf = face_quadrics(pos, faces)
    Q = np.zeros((V, 10), np.float64)
    for k in range(fan.shape[1]):
        m = deg > k
        Q[m] = Q[m] + qf[fan[m, k]]
    return Q


def cost(Q, x):
    """x^T A x + 2 b.x + c at f64 points x [..., 3], in the pinned order."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2, c = (Q[..., i] for i in range(10))
    x0, x1, x2 = x[..., 0], x[..., 1], x[..., 2]
    t0 = a00 * x0 + a01 * x1 + a02 * x2 + b0
    t1 = a01 * x0 + a11 * x1 + a12 * x2 + b1
    t2 = a02 * x0 + a12 * x1 + a22 * x2 + b2
    return (t0 * x0 + t1 * x1 + t2 * x2) + (b0 * x0 + b1 * x1 + b2 * x2) + c


def optimal_point(Q, pu, pv):
    """(v* [E,3] f32, cost [E] f64): the solve of A x = -b by cofactors where |det| > SINGULAR_REL * tr^3 and the result
    is finite, else the cheapest of u, v, the midpoint (first wins a tie)."""
    a00, a01, a02, a11, a12, a22, b0, b1, b2, _ = (Q[:, i] for i in range(10))
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = a00 * c00 + a01 * c01 + a02 * c02
    tr = a00 + a11 + a22
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x = np.stack([-(c00 * b0 + c01 * b1 + c02 * b2) / det,
                      -(c01 * b0 + c11 * b1 + c12 * b2) / det,
                      -(c02 * b0 + c12 * b1 + c22 * b2) / det], -1).astype(np.float32)
        solved = (np.abs(det) > SINGULAR_REL * (tr * tr * tr)) & np.isfinite(x).all(1)
        mid = (pu + pv) * np.float32(0.5)
        cands = [pu, pv, mid]
        cs = [cost(Q, p.astype(np.float64)) for p in cands]
        best, bc = pu.copy(), cs[0]
        for p, cc in zip(cands[1:], cs[1:]):
            b = cc < bc
            best[b], bc = p[b], np.where(b, cc, bc)
        out = np.where(solved[:, None], x, best)
        return out, np.where(solved, cost(Q, x.astype(np.float64)), bc)


def vertex_status(faces, fan, deg):
    """(locked [V] bool, nxt [V, D]): nxt = the vertex after w in each fan face (-1 padded).  Locked: no faces, an edge
    at w that is not in exactly one face each way round, or faces that do not make one closed fan."""
    V, D = fan.shape
    valid = fan >= 0
    fv = faces[np.maximum(fan, 0)]                                   # [V, D, 3]
    w = np.arange(V)[:, None]
    c = np.argmax(fv == w[:, :, None], axis=2)
    nxt = np.take_along_axis(fv, ((c + 1) % 3)[:, :, None], 2)[:, :, 0]
    prv = np.take_along_axis(fv, ((c + 2) % 3)[:, :, None], 2)[:, :, 0]
    nxt = np.where(valid, nxt, -1)
    prv = np.where(valid, prv, -2)
    eq_np = (nxt[:, :, None] == prv[:, None, :])                    # [V, k, j]: nxt[k] == prv[j]
    ok = ((nxt[:, :, None] == nxt[:, None, :]).sum(2) == 1) & (eq_np.sum(2) == 1)
    ok &= ((prv[:, :, None] == prv[:, None, :]).sum(2) == 1) & (eq_np.sum(1) == 1)
    locked = (deg == 0) | ~np.where(valid, ok, True).all(1)
    # one cycle: from the first face, the next face is the one whose prv is this one's nxt
    succ = np.argmax(eq_np, axis=2)
    cur = np.zeros(V, np.int64)
    length = np.zeros(V, np.int64)
    for s in range(1, D + 1):
        cur = succ[np.arange(V), cur]
        length = np.where((length == 0) & (cur == 0), s, length)
    locked |= length != deg
    return locked, nxt


def evaluate(pos, faces, Q, fan, deg, locked, nxt, max_error):
    """Key [3F] u64 = cost bits << 32 | edge_tag(e) (KEY_NONE: no valid candidate) and v* [3F, 3] f32 of every
    half-edge e = 3 f + k."""
    F = len(faces)
    u = faces.reshape(-1)
    v = np.roll(faces, -1, axis=1).reshape(-1)
    keys = np.full(3 * F, KEY_NONE, np.uint64)
    vstar = np.zeros((3 * F, 3), np.float32)
    cand = (u < v) & ~locked[u] & ~locked[v] & ~((deg[u] == 3) & (deg[v] == 3))
    e = np.nonzero(cand)[0]
    if len(e) == 0:
        return keys, vstar
    u, v = u[e], v[e]
    # link condition: exactly the two opposite vertices are common neighbours
    Nu, Nv = nxt[u], nxt[v]
    common = ((Nu[:, :, None] == Nv[:, None, :]) & (Nu[:, :, None] >= 0)).sum((1, 2))
    Qe = Q[u] + Q[v]
    x, c = optimal_point(Qe, pos[u], pos[v])
    ok = (common == 2) & np.isfinite(c)
    c = np.where(c > 0, c, 0.0)                                      # (-0.0 and below -> +0.0)
    cf = c.astype(np.float32)
    ok &= ~(cf > np.float32(max_error))
    # no face around u or v (other than the edge's two) may flip: new normal . old normal > 0; a face of zero area may
    # not gain area (its plane is in no quadric, so the move would be free)
    fs = np.concatenate([fan[u], fan[v]], 1)                          # [E, 2D]
    fv = faces[np.maximum(fs, 0)]                                     # [E, 2D, 3]
    hu, hv = (fv == u[:, None, None]), (fv == v[:, None, None])
    consider = (fs >= 0) & ~(hu.any(2) & hv.any(2))
    P = pos[fv].astype(np.float64)                                    # [E, 2D, 3, 3]
    Pn = np.where((hu | hv)[..., None], x.astype(np.float64)[:, None, None, :], P)
    n0 = _cross(P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0])
    n1 = _cross(Pn[:, :, 1] - Pn[:, :, 0], Pn[:, :, 2] - Pn[:, :, 0])
    nz0, nz1 = (n0 != 0).any(2), (n1 != 0).any(2)
    flips = consider & np.where(nz0, ~(_dot(n0, n1) > 0), nz1)
    ok &= ~flips.any(1)
    k = (cf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | edge_tag(e).astype(np.uint64)
    keys[e[ok]] = k[ok]
    vstar[e] = x
    return keys, vstar


def normals(pos, faces):
    """Normalised sum of the incident faces' f32 cross products, ascending face order (0 for a zero sum)."""
    V = len(pos)
    p = pos[faces]
    n = _cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]).astype(np.float32)
    fan, deg = _fan(faces, V) if len(faces) else (np.zeros((V, 0), np.int64), np.zeros(V, np.int64))
    acc = np.zeros((V, 3), np.float32)
    for k in range(fan.shape[1]):
        m = deg > k
        acc[m] = acc[m] + n[fan[m, k]]
    l2 = acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1] + acc[:, 2] * acc[:, 2]
    with np.errstate(divide="ignore"):
        inv = np.where(l2 > 0, np.float32(1) / np.sqrt(l2), np.float32(0)).astype(np.float32)
    return (acc * inv[:, None]).astype(np.float32)


def decimate(verts, faces, target_faces, max_error=np.inf, max_rounds=DEFAULT_MAX_ROUNDS, trace=None):
    """-> (verts [V',3] f32, faces [F',3] int32, normals [V',3] f32, info dict(rounds, collapses)).  `trace` (a list)
    receives (F, S, m) of every round begun: the faces it started from, the edges selected, the collapses applied."""
    pos = np.array(verts, dtype=np.float32).reshape(-1, 3)
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    V = len(pos)
    if len(faces) and (faces.min() < 0 or faces.max() >= V):
        raise ValueError("decimate: face index outside [0, %d)" % V)
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
    Q = vertex_quadrics(pos, faces) if len(faces) else np.zeros((V, 10))
    rounds = collapses = 0
    while rounds < max_rounds and len(faces) > target_faces:
        F = len(faces)
        fan, deg = _fan(faces, V)
        locked, nxt = vertex_status(faces, fan, deg)
        keys, vstar = evaluate(pos, faces, Q, fan, deg, locked, nxt, max_error)
        u = faces.reshape(-1)
        v = np.roll(faces, -1, axis=1).reshape(-1)
        valid = keys != KEY_NONE
        K1 = np.full(V, KEY_NONE, np.uint64)
        np.minimum.at(K1, u[valid], keys[valid])
        np.minimum.at(K1, v[valid], keys[valid])
        FK = K1[faces].min(1)
        K2 = np.where(fan >= 0, FK[np.maximum(fan, 0)], KEY_NONE).min(1)
        sel = np.nonzero(valid & (K2[u] == keys) & (K2[v] == keys))[0]
        S = len(sel)
        if S == 0:
            if trace is not None:
                trace.append((F, 0, 0))
            break
        if F - 2 * S < target_faces:
            m = (F - target_faces + 1) // 2
            sel = np.sort(sel[np.argsort(keys[sel])[:m]])
        if trace is not None:
            trace.append((F, S, len(sel)))
        su, sv = u[sel], v[sel]
        pos[su] = vstar[sel]
        Q[su] = Q[su] + Q[sv]
        remap = np.arange(V)
        remap[sv] = su
        faces = remap[faces]
        faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
        assert len(faces) == F - 2 * len(sel)
        rounds += 1
        collapses += len(sel)
    used = np.zeros(V, bool)
    used[faces.reshape(-1)] = True
    new = np.cumsum(used) - 1
    out_v = pos[used]
    out_f = new[faces].astype(np.int32)
    return out_v, out_f, normals(out_v, out_f), {"rounds": rounds, "collapses": collapses}
