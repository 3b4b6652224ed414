"""numpy restatement of lnerf_uv_raster and lnerf_uv_dilate (include/lnerf_hip.h): the same candidate boxes, the same
f32 arithmetic in the same order and the same max-index rule, so texel_face, texel_idx, pos and the dilated texture
compare bit for bit with the HIP ops."""
import numpy as np

f32 = np.float32

# neighbour order of a gutter round (row, column offsets)
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))


def _edge(X, Y, a, b, px, py):
    return (X[b] - X[a]) * (py - Y[a]) - (Y[b] - Y[a]) * (px - X[a])


def face_setup(verts, faces, vt, ft, R):
    """Per face: pixel-space corners X, Y [3,F], area [F], box (j0, i0, w, h) [F] each, and the bad-index mask."""
    vt = np.asarray(vt, np.float32).reshape(-1, 2)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ft = np.asarray(ft, np.int64).reshape(-1, 3)
    V, T = len(np.asarray(verts).reshape(-1, 3)), len(vt)
    bad = ((faces < 0) | (faces >= V) | (ft < 0) | (ft >= T)).any(1)
    q = np.where(bad[:, None], 0, ft).T                                    # [3,F]
    Rf = f32(R)
    with np.errstate(all="ignore"):
        if T:
            X = vt[q, 0] * Rf
            Y = (f32(1.0) - vt[q, 1]) * Rf
        else:
            X = Y = np.zeros_like(q, dtype=np.float32)
        area = (X[1] - X[0]) * (Y[2] - Y[0]) - (Y[1] - Y[0]) * (X[2] - X[0])
        ok = ~bad & np.isfinite(area) & (area != 0)
        top = Rf - f32(1.0)
        xl = np.floor(np.fmin(np.fmin(X[0], X[1]), X[2])) - f32(1.0)
        xh = np.floor(np.fmax(np.fmax(X[0], X[1]), X[2])) + f32(1.0)
        yl = np.floor(np.fmin(np.fmin(Y[0], Y[1]), Y[2])) - f32(1.0)
        yh = np.floor(np.fmax(np.fmax(Y[0], Y[1]), Y[2])) + f32(1.0)
        ok &= ~((xh < 0) | (yh < 0) | (xl > top) | (yl > top))
        j0 = np.where(ok, np.fmax(xl, f32(0)), 0).astype(np.int64)
        i0 = np.where(ok, np.fmax(yl, f32(0)), 0).astype(np.int64)
        w = np.where(ok, np.where(ok, np.fmin(xh, top), 0).astype(np.int64) - j0 + 1, 0)
        h = np.where(ok, np.where(ok, np.fmin(yh, top), 0).astype(np.int64) - i0 + 1, 0)
    return X, Y, area, (j0, i0, w, h), bad


def _candidates(X, Y, area, box):
    """Every (face, texel) candidate with its coverage: f, i, j, covered [N]."""
    j0, i0, w, h = box
    items = w * h
    f = np.repeat(np.arange(len(items)), items)
    start = np.cumsum(items) - items
    local = np.arange(int(items.sum()), dtype=np.int64) - start[f]
    di = local // w[f]
    i, j = i0[f] + di, j0[f] + (local - di * w[f])
    cov = _covered(X[:, f], Y[:, f], area[f], i, j)[0]
    return f, i, j, cov


def _covered(X, Y, area, i, j):
    px = j.astype(np.float32) + f32(0.5)
    py = i.astype(np.float32) + f32(0.5)
    with np.errstate(all="ignore"):
        e = [_edge(X, Y, 1, 2, px, py), _edge(X, Y, 2, 0, px, py), _edge(X, Y, 0, 1, px, py)]
    pos_side = (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
    neg_side = (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)
    return np.where(area > 0, pos_side, neg_side), e


def uv_raster(verts, faces, vt, ft, R):
    """-> texel_face [R,R] int32, texel_idx [P] int32, pos [P,3] f32, n_items, n_bad (the op's counts)."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    X, Y, area, box, bad = face_setup(verts, faces, vt, ft, R)
    f, i, j, cov = _candidates(X, Y, area, box)
    tf = np.full(R * R, -1, np.int64)
    np.maximum.at(tf, (i * R + j)[cov], f[cov])
    texel_idx = np.flatnonzero(tf >= 0)
    g = tf[texel_idx]
    _, e = _covered(X[:, g], Y[:, g], area[g], texel_idx // R, texel_idx % R)
    a = area[g]
    b0, b1, b2 = e[0] / a, e[1] / a, e[2] / a
    P = verts[faces[g]]                                                    # [P,3,3]
    pos = b0[:, None] * P[:, 0] + b1[:, None] * P[:, 1] + b2[:, None] * P[:, 2]
    n_items = int((box[2] * box[3]).sum())
    return (tf.reshape(R, R).astype(np.int32), texel_idx.astype(np.int32), pos.astype(np.float32), n_items,
            int(bad.sum()))


def coverage_count(verts, faces, vt, ft, R):
    """How many faces cover each texel centre [R,R] (every covering face, not only the winner)."""
    X, Y, area, box, _ = face_setup(verts, faces, vt, ft, R)
    f, i, j, cov = _candidates(X, Y, area, box)
    n = np.zeros(R * R, np.int64)
    np.add.at(n, (i * R + j)[cov], 1)
    return n.reshape(R, R), np.bincount(f[cov], minlength=len(area))


def barycentrics(verts, faces, vt, ft, R, texel_idx, texel_face):
    """(b0, b1, b2) [P] f32 of the winning face at each covered texel."""
    X, Y, area, _, _ = face_setup(verts, faces, vt, ft, R)
    g = np.asarray(texel_face).reshape(-1)[texel_idx]
    _, e = _covered(X[:, g], Y[:, g], area[g], texel_idx // R, texel_idx % R)
    return tuple(x / area[g] for x in e)


def uv_dilate(texture, mask, passes):
    """`passes` gutter rounds over texture [C,R,R] f32, mask [R,R] uint8 (2 covered, 1 filled, 0 empty)."""
    tex = np.array(texture, np.float32, copy=True)
    mask = np.array(mask, np.uint8, copy=True)
    C, R, _ = tex.shape
    for _ in range(passes):
        full = mask != 0
        pm = np.pad(full, 1)
        pt = np.pad(tex, ((0, 0), (1, 1), (1, 1)))
        s = np.zeros_like(tex)
        cnt = np.zeros((R, R), np.int64)
        for di, dj in NEIGHBOURS:
            m = pm[1 + di:1 + di + R, 1 + dj:1 + dj + R]
            v = pt[:, 1 + di:1 + di + R, 1 + dj:1 + dj + R]
            s = np.where(m[None], s + v, s)
            cnt += m
        fill = ~full & (cnt > 0)
        with np.errstate(all="ignore"):
            mean = s / np.maximum(cnt, 1).astype(np.float32)[None]
        tex = np.where(fill[None], mean, tex).astype(np.float32)
        mask = np.where(fill, np.uint8(1), mask).astype(np.uint8)
    return tex, mask
