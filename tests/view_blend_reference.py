"""Float64 numpy restatement of the three rules of csrc/viewblend.hip (include/lnerf_hip.h: lnerf_view_lowpass,
lnerf_view_overlap_stats, lnerf_uv_project_views_bands) and of view_bake.exposure_gains, on top of the restatement of
the acceptance rule in tests/test_gpu_view_bake.py (ref_steps).  Nothing here touches the GPU."""
import math

import numpy as np

from tests.test_gpu_view_bake import COS_MIN, POWER, SLACK, ref_steps

FIXED = 16777216.0          # 2^24: the fixed point of the overlap sums


def ref_taps(sigma):
    """exp(-t^2 / (2 sigma^2)), t = -r .. r, r = ceil(3 sigma), normalised in float64, then rounded to f32."""
    r = int(math.ceil(3.0 * sigma))
    t = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-t * t / (2.0 * sigma * sigma)) if sigma > 0 else np.ones(1)
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def ref_lowpass(images, zbuf, sigma):
    """images [K,C,H,W], zbuf [K,H,W] -> low [K,C,H,W] float64.  Unusable pixels are selected out, not multiplied."""
    images, zbuf = np.asarray(images), np.asarray(zbuf)
    g = ref_taps(sigma)
    r = len(g) // 2
    K, C, H, W = images.shape
    usable = zbuf < 0
    clean = np.where(usable[:, None], images, 0.0).astype(np.float64)
    num, den = np.zeros((K, C, H, W)), np.zeros((K, H, W))
    for t in range(-r, r + 1):                       # rows: out column j reads column j + t
        j0, j1 = max(0, -t), min(W, W - t)
        if j0 >= j1:
            continue
        u = usable[:, :, j0 + t:j1 + t]
        den[:, :, j0:j1] += g[t + r] * u
        num[:, :, :, j0:j1] += g[t + r] * clean[:, :, :, j0 + t:j1 + t]
    num2, den2 = np.zeros_like(num), np.zeros_like(den)
    for t in range(-r, r + 1):                       # columns: out row i reads row i + t
        i0, i1 = max(0, -t), min(H, H - t)
        if i0 >= i1:
            continue
        den2[:, i0:i1] += g[t + r] * den[:, i0 + t:i1 + t]
        num2[:, :, i0:i1] += g[t + r] * num[:, :, i0 + t:i1 + t]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den2[:, None] > 0, num2 / den2[:, None], 0.0)


def ref_bilinear(stack, s):
    """The bilinear samples of stack [K,C,H,W] at the taps of ref_steps' result s -> [P,K,C] (garbage where rejected)."""
    K = stack.shape[0]
    k, i, j, tu, tv = np.arange(K)[None], s["i0"], s["j0"], s["tu"][..., None], s["tv"][..., None]
    tap = lambda di, dj: stack[k, :, i + di, j + dj]
    return (1 - tu) * (1 - tv) * tap(0, 0) + tu * (1 - tv) * tap(0, 1) + (1 - tu) * tv * tap(1, 0) + tu * tv * tap(1, 1)


def ref_stats(pos, nrm, cams, zbuf, low, cos_min=COS_MIN, slack=SLACK, keep=None):
    """-> (N [K,K] int64, M [K,K,C] float64 = view i's mean low colour over the points i and j both accept (0 where
    N = 0), ok [P,K]).  keep [P] bool: the points that count (default all)."""
    pos, nrm, cams, zbuf, low = (np.asarray(a, np.float64) for a in (pos, nrm, cams, zbuf, low))
    s = ref_steps(pos, nrm, cams, zbuf, cos_min, slack)
    ok = s["step"] == 0
    if keep is not None:
        ok = ok & keep[:, None]
    L = np.where(ok[..., None], ref_bilinear(low, s), 0.0)
    pair = ok[:, :, None] & ok[:, None, :]
    K = ok.shape[1]
    pair[:, np.arange(K), np.arange(K)] = False
    N = pair.sum(0).astype(np.int64)
    S = np.einsum("pij,pic->ijc", pair.astype(np.float64), L)
    return N, np.where(N[..., None] > 0, S / np.maximum(N, 1)[..., None], 0.0), ok


def ref_gains(N, M, prior):
    """The minimiser of sum_{i<j} N_ij (g_i M_ij - g_j M_ji)^2 + prior sum_i n_i (g_i - 1)^2 per channel, as a least
    squares problem over its residuals (not through the normal equations view_bake.exposure_gains solves).
    A view with n_i = 0 gets 1.  -> [K,C] float64."""
    N = np.asarray(N, np.float64)
    K, C = M.shape[0], M.shape[2]
    n = N.sum(1) - np.diag(N)
    gains = np.ones((K, C))
    for c in range(C):
        rows, rhs = [], []
        for i in range(K):
            for j in range(i + 1, K):
                if N[i, j] > 0:
                    row = np.zeros(K)
                    row[i], row[j] = math.sqrt(N[i, j]) * M[i, j, c], -math.sqrt(N[i, j]) * M[j, i, c]
                    rows.append(row)
                    rhs.append(0.0)
        for i in range(K):
            row = np.zeros(K)
            row[i] = math.sqrt(prior * n[i]) if n[i] > 0 else 1.0
            rows.append(row)
            rhs.append(row[i])
        gains[:, c] = np.linalg.lstsq(np.array(rows), np.array(rhs), rcond=None)[0]
    gains[n == 0] = 1.0
    return gains


def ref_bands(pos, nrm, cams, zbuf, images, low, gains=None, cos_min=COS_MIN, power=POWER, slack=SLACK):
    """The two-band rule in float64 -> dict(out [P,C], weight [P], count [P], best [P] (-1: none), margin [P]: the
    relative gap between the two largest weights of a point (inf with fewer than two views), ok [P,K])."""
    pos, nrm, cams, zbuf, images, low = (np.asarray(a, np.float64) for a in (pos, nrm, cams, zbuf, images, low))
    s = ref_steps(pos, nrm, cams, zbuf, cos_min, slack)
    ok = s["step"] == 0
    P, K = ok.shape
    g = np.ones((K, images.shape[1])) if gains is None else np.asarray(gains, np.float64)
    I = ref_bilinear(images, s) * g[None]
    L = ref_bilinear(low, s) * g[None]
    w = np.where(ok, np.where(ok, s["c"], 1.0) ** power, 0.0)
    weight, count = w.sum(1), ok.sum(1)
    seen = count > 0
    lowmean = (w[..., None] * np.where(ok[..., None], L, 0.0)).sum(1) / np.where(seen, weight, 1.0)[:, None]
    wk = np.where(ok, w, -1.0)
    best = np.where(seen, wk.argmax(1), -1)                    # argmax takes the first of equal maxima: the lowest k
    top = np.sort(wk, 1)[:, ::-1]
    second = top[:, 1] if K > 1 else np.full(P, -1.0)
    margin = np.where(second >= 0, (top[:, 0] - second) / np.where(top[:, 0] > 0, top[:, 0], 1.0), np.inf)
    b = np.maximum(best, 0)
    pick = lambda a: a[np.arange(P), b]
    out = np.where(seen[:, None], pick(I) + (lowmean - pick(L)), 0.0)
    return dict(out=out, weight=weight, count=count, best=best, margin=margin, ok=ok)


def surface_images(cams, zbuf, fn):
    """Images of a surface coloured by fn(world position [N,3]) -> [N,C], rendered consistently: every usable pixel
    (zbuf < 0) is back-projected through its camera record to the surface point it shows.  cams [K,14], zbuf [K,H,W]
    -> images [K,C,H,W] float64, 0 on unusable pixels."""
    cams, zbuf = np.asarray(cams, np.float64), np.asarray(zbuf, np.float64)
    K, H, W = zbuf.shape
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    X, Y = (2 * j + 1) / W - 1, 1 - (2 * i + 1) / H
    out = []
    for k in range(K):
        rot, eye, fx, fy = cams[k, :9].reshape(3, 3), cams[k, 9:12], cams[k, 12], cams[k, 13]
        z = np.where(zbuf[k] < 0, zbuf[k], -1.0)
        p = np.stack([X * -z / fx, Y * -z / fy, z], -1).reshape(-1, 3)
        col = fn(p @ rot + eye).reshape(H, W, -1)
        out.append(np.where((zbuf[k] < 0)[..., None], col, 0.0).transpose(2, 0, 1))
    return np.stack(out)


def view_spread(samples, ok):
    """Mean over the points with at least two views of the standard deviation, across their views, of samples [P,K,C]
    (averaged over the channels)."""
    n = ok.sum(1)
    many = n >= 2
    w = ok[many][..., None].astype(np.float64)
    x = np.where(ok[many][..., None], samples[many], 0.0)
    cnt = n[many][:, None].astype(np.float64)
    mean = (w * x).sum(1) / cnt
    var = (w * (x - mean[:, None]) ** 2).sum(1) / cnt
    return float(np.sqrt(var).mean())
