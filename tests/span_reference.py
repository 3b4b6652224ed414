"""What the references of the one-wavefront-per-ray ops share (csrc/span_walk.h is the kernels' side of it): the rows of the
rays' spans, the compositing weight in float64, one chunk's exclusive sum as the kernels take it, and the finite-difference
normal with its backward.  Used by tests/distortion_reference.py, tests/normal_image_reference.py and
tests/orient_reference.py; each is written ONCE here, in the kernels' op order, for any dtype."""
import numpy as np

CHUNK = 64
FLOOR = np.float32(1e-20)


def span_rows(rays):
    """rays [N,3] -> (rows int64 [m], ids int64 [m]) of every span row, ray after ray."""
    rows, ids = [], []
    for rid, off, cnt in np.asarray(rays).tolist():
        rows.append(np.arange(off, off + cnt, dtype=np.int64))
        ids.append(np.full(cnt, rid, dtype=np.int64))
    if not rows:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(rows), np.concatenate(ids)


def per_ray_max(values, rays, n_ids):
    """values [m] or [m, k] in span-row order -> per ray id the largest |value| of its span (0 for an empty span / absent id)."""
    out, at = np.zeros(int(n_ids)), 0
    for rid, _, cnt in np.asarray(rays).tolist():
        if cnt:
            out[rid] = float(np.abs(values[at:at + cnt]).max())
        at += cnt
    return out


def weights(sigmas, deltas, rays, T_thresh, density_scale=1.0):
    """float64 compositing weights of every span row (ray order) on sigma' = density_scale * sigma:  tau = sigma' dt,
    T = exp(-sum of the taus in front), w = T >= T_thresh ? (1 - exp(-tau)) T : 0.  -> (w, T, tau)."""
    sig = np.asarray(sigmas, dtype=np.float32).astype(np.float64)
    dt = np.asarray(deltas, dtype=np.float32).astype(np.float64)[:, 0]
    w, T, tau = [], [], []
    for _, off, cnt in np.asarray(rays).tolist():
        t = (float(density_scale) * sig[off:off + cnt]) * dt[off:off + cnt]
        excl = np.concatenate([[0.0], np.cumsum(t)[:-1]]) if cnt else np.zeros(0)
        Tr = np.exp(-excl)
        w.append(np.where(Tr >= float(T_thresh), (1.0 - np.exp(-t)) * Tr, 0.0))
        T.append(Tr)
        tau.append(t)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0)
    return cat(w), cat(T), cat(tau)


def chunk_excl(x, carry, dtype):
    """One chunk: the inclusive sum, the exclusive one (previous lane's inclusive, lane 0: 0, plus the carry), the carry after."""
    inc = np.cumsum(x, dtype=dtype)
    prev = np.concatenate([np.zeros(1, dtype), inc[:-1]]).astype(dtype)
    return inc, (prev + carry).astype(dtype), dtype(carry + inc[-1])


def fd_normal(sg, inv_2eps, dtype):
    """sg [m,7] -> (n [m,3], s2 [m], r [m]) in `dtype`, the order of lnerf_shade_fd_forward (a NaN component becomes 0)."""
    sg = np.asarray(sg, dtype=np.float32).astype(dtype)
    k = dtype(np.float32(inv_2eps))
    with np.errstate(all="ignore"):
        g = [((sg[:, 1 + 2 * a] - sg[:, 2 + 2 * a]) * k).astype(dtype) for a in range(3)]
        s2 = ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]).astype(dtype)
        r = (dtype(1) / np.sqrt(np.fmax(s2, dtype(FLOOR)))).astype(dtype)      # (fmax: a NaN s2 gives the floor)
        n = np.stack([-(g[a] * r) for a in range(3)], -1).astype(dtype)
        n = np.where(np.isnan(n), dtype(0), n).astype(dtype)
    return n, s2, r


def normal_backward(n, s2, r, dn, inv_2eps, dtype):
    """dn [m,3] -> the six stencil rows [m,6] (+x, -x, +y, -y, +z, -z), the order of lnerf_shade_fd_backward."""
    k = dtype(np.float32(inv_2eps))
    with np.errstate(all="ignore"):
        q = ((n[:, 0] * dn[:, 0] + n[:, 1] * dn[:, 1]) + n[:, 2] * dn[:, 2]).astype(dtype)
        project = s2 > dtype(FLOOR)                                            # (False for a NaN s2)
        out = np.zeros((n.shape[0], 6), dtype)
        for a in range(3):
            t = np.where(project, dn[:, a] - n[:, a] * q, dn[:, a]).astype(dtype)
            v = ((-(r * t)) * k).astype(dtype)
            out[:, 2 * a], out[:, 2 * a + 1] = v, -v
    return out


# ------------------------------------------------------------------ the case of tests/test_gpu_span_weights.py
# One input on which four ops must produce THE SAME weights: every normal is exactly (-1, 0, 0) and every view direction too,
# so the orientation term and the normal image reduce to plain sums of w, bit for bit (r = 1 / sqrt(1) = 1, q = 1).
W_COUNTS = (0, 1, 2, 63, 64, 65, 128, 130, 200)    # the chunk edges, two and three chunks
W_IDS = (4, 7, 0, 8, 2, 5, 1, 3, 6)                # ray r -> id, a permutation
W_REGIMES = ("thin", "opaque", "mixed")
W_T_THRESHES = (1e-4, 0.0)
W_EPS = 0.5                                        # inv_2eps = 1
# opaque: thin samples (sigma dt = 0.02) up to this position of each ray, sigma in [1e3, 1e4] from there on -- the cut
# (T_thresh = 1e-4) falls inside the first chunk, on the chunk edge (65: the first dead sample is lane 0 of the second
# chunk), inside the second and inside the third chunk
W_OPAQUE_FROM = (0, 0, 1, 30, 63, 63, 20, 100, 150)


def weights_case(regime, seed=0):
    """-> dict(rays int32 [9,3] whose spans tile [0, M) exactly (M = 653), deltas f32 [M,2] (dt > 0, t increasing along a
    span), sig f32 [M] finite and >= 0, sig7 f32 [7 M] with row 7 i = sig, row 7 i + 1 = 1 and the others 0, rays_d f32
    [9,3] = (-1, 0, 0), shade f32 [1,5], N, M)."""
    rng = np.random.default_rng(100 + seed + 10 * W_REGIMES.index(regime))
    cnts = np.array(W_COUNTS)
    N, M = len(cnts), int(cnts.sum())
    offs = np.concatenate([[0], np.cumsum(cnts)[:-1]])
    rays = np.stack([np.array(W_IDS), offs, cnts], -1).astype(np.int32)
    dt = rng.uniform(0.005, 0.02, M)
    t = np.zeros(M)
    tau = np.exp(rng.uniform(np.log(1e-3), np.log(1e-1), M))                 # thin: sigma dt in [1e-3, 1e-1]
    for r, (off, cnt) in enumerate(zip(offs, cnts)):
        s = slice(off, off + cnt)
        gap = np.where(rng.random(cnt) < 0.2, rng.uniform(0.0, 0.05, cnt), 0.0)
        t[s] = 0.3 + np.cumsum(np.concatenate([[0.0], (dt[s] + gap)[:-1]])) if cnt else 0.0
        if regime == "opaque":
            tau[s] = 0.02
            p = W_OPAQUE_FROM[r]
            tau[off + p:off + cnt] = rng.uniform(1e3, 1e4, cnt - p) * dt[off + p:off + cnt]
        elif regime == "mixed":
            tau[s] = np.exp(rng.uniform(np.log(1e-3), np.log(1.0), cnt))
            at = 0
            while at < cnt:                                                 # runs of sigma = 0 between runs of matter
                run = int(rng.integers(1, 12))
                if rng.random() < 0.4:
                    tau[off + at:off + min(at + run, cnt)] = 0.0
                at += run
    sig = (tau / dt).astype(np.float32)
    sig7 = np.zeros((M, 7), np.float32)
    sig7[:, 0], sig7[:, 1] = sig, 1.0
    rays_d = np.tile(np.array([-1.0, 0.0, 0.0], np.float32), (N, 1))
    shade = np.array([[0.6, 0.0, 0.8, 0.1, 0.0]], np.float32)
    return dict(rays=rays, deltas=np.stack([dt, t], -1).astype(np.float32), sig=sig, sig7=sig7.reshape(-1), rays_d=rays_d,
                shade=shade, N=N, M=M)
