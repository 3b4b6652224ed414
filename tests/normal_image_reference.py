"""References of the composited normal image and the 2D smoothness stencil (csrc/normal_image.hip; contract in
include/lnerf_hip.h, "composited normal image"):  normal_image[ray] = sum_i w_i n_i,  loss[p] = (sum_c (right - own)^2,
sum_c (below - own)^2).

  fd_normal()           the finite-difference normal of lnerf_shade_fd_forward for any dtype (tests/span_reference.py, which
                        also holds its backward, span_rows(), per_ray_max() and the chunk's exclusive sum)
  truth()               float64, no chunks, nothing of the kernels' algebra: the weights by a plain cumulative sum, the
                        forward as a plain sum, the backward with the suffix sums sum_{j>i} g_j w_j written out -- NOT the
                        identity sum_i g_i w_i = N . dN the kernel's one sweep rests on
  restate()             the header's arithmetic, operation by operation, for any dtype: chunks of 64 with scalar carries,
                        the exclusive sum taken from the previous lane, G_tot from the forward's output.  (Inside a chunk
                        numpy's cumsum adds left to right where the kernel's scan adds as a tree, and numpy's exp is not
                        expf: the restatement measures the arithmetic's own error, it is no bit model.)
  central_difference()  float64 central differences of sum(normal_image * dN) w.r.t. chosen entries of sigmas7: validates
                        truth()'s backward on the CPU
  f32_errors()          the float32 restatement's error against truth(), per ray: the yardstick of the GPU tests
  smooth_forward() / smooth_backward()   the stencil, operation for operation, for any dtype (no transcendental: float32 is
                        a bit model of the kernels); smooth_truth_backward() the float64 gradient by scattering
  op_case() / check_case()   the op-level input of tests/test_gpu_normal_image.py and its preconditions"""
import numpy as np

from tests import span_reference as S
from tests.span_reference import CHUNK, FLOOR, fd_normal, per_ray_max, span_rows    # (the tests reach them through this module)

T_THRESH = 1e-4


def _inputs(sigmas7, deltas, dtype):
    sg = np.asarray(sigmas7, dtype=np.float32).astype(dtype).reshape(-1, 7)
    d = np.asarray(deltas, dtype=np.float32).astype(dtype)
    return sg, d


def truth(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, T_thresh=T_THRESH, dN=None):
    """float64 -> dict(image [n_ids,3], w [m], T [m], live [m], n [m,3], r [m] in span-row order, and with dN [n_ids,3]:
    grad [m,7], the seven dsigmas7 rows of every span row)."""
    sg, d = _inputs(sigmas7, deltas, np.float64)
    ds, thr = float(np.float32(density_scale)), float(np.float32(T_thresh))
    image = np.zeros((int(n_ids), 3))
    ws, Ts, lives, ns, rs, grads = [], [], [], [], [], []
    for rid, off, cnt in np.asarray(rays).tolist():
        s = slice(off, off + cnt)
        n, s2, r = fd_normal(sg[s], inv_2eps, np.float64)
        dt = d[s, 0]
        tau = (ds * sg[s, 0]) * dt
        excl = np.concatenate([[0.0], np.cumsum(tau)[:-1]]) if cnt else np.zeros(0)
        T, e = np.exp(-excl), np.exp(-tau)
        live = T >= thr
        w = np.where(live, (1.0 - e) * T, 0.0)
        image[rid] = (w[:, None] * n).sum(0)
        ws.append(w); Ts.append(T); lives.append(live); ns.append(n); rs.append(r)
        if dN is not None:
            go = np.asarray(dN, dtype=np.float32).astype(np.float64)[rid]
            g = n @ go
            gw = g * w
            after = np.concatenate([np.cumsum(gw[::-1])[::-1][1:], [0.0]]) if cnt else np.zeros(0)   # sum_{j>i} g_j w_j
            dtau = np.where(live, g * T * e - after, 0.0)
            rows = np.zeros((cnt, 7))
            rows[:, 0] = ds * dt * dtau
            rows[:, 1:] = S.normal_backward(n, s2, r, w[:, None] * go[None, :], inv_2eps, np.float64)
            grads.append(rows)
    cat = lambda v, shape: np.concatenate(v) if v else np.zeros(shape)
    out = dict(image=image, w=cat(ws, 0), T=cat(Ts, 0), live=cat(lives, 0).astype(bool), n=cat(ns, (0, 3)), r=cat(rs, 0))
    if dN is not None:
        out["grad"] = cat(grads, (0, 7))
    return out


def restate(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, T_thresh=T_THRESH, dN=None, dtype=np.float32):
    """The header's order of operations in `dtype` -> dict(image [n_ids,3], w [m], live [m], and with dN: grad [m,7])."""
    sg, d = _inputs(sigmas7, deltas, dtype)
    ds, thr = dtype(np.float32(density_scale)), dtype(np.float32(T_thresh))
    image = np.zeros((int(n_ids), 3), dtype)
    ws, lives, grads = [], [], []
    go_all = None if dN is None else np.asarray(dN, dtype=np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        for rid, off, cnt in np.asarray(rays).tolist():
            carry, acc, rec = dtype(0), np.zeros(3, dtype), []
            for base in range(0, cnt, CHUNK):
                s = slice(off + base, off + min(base + CHUNK, cnt))
                n, s2, r = fd_normal(sg[s], inv_2eps, dtype)
                dt = d[s, 0]
                tau = ((ds * sg[s, 0]).astype(dtype) * dt).astype(dtype)
                _, excl, carry = S.chunk_excl(tau, carry, dtype)
                T = np.exp(-excl).astype(dtype)
                e = np.exp(-tau).astype(dtype)
                alpha = dtype(1) - e
                live = T >= thr
                w = np.where(live, alpha * T, dtype(0)).astype(dtype)
                acc = (acc + (w[:, None] * n).astype(dtype).sum(0, dtype=dtype)).astype(dtype)
                rec.append((n, s2, r, dt, w, (T * e).astype(dtype), live))
            image[rid] = acc
            for n, s2, r, dt, w, Te, live in rec:
                ws.append(w); lives.append(live)
            if go_all is not None:
                go = go_all[rid]
                total = dtype((acc[0] * go[0] + acc[1] * go[1]) + acc[2] * go[2])
                c_g = dtype(0)
                for n, s2, r, dt, w, Te, live in rec:
                    g = ((n[:, 0] * go[0] + n[:, 1] * go[1]) + n[:, 2] * go[2]).astype(dtype)
                    P = (np.cumsum((g * w).astype(dtype), dtype=dtype) + c_g).astype(dtype)
                    c_g = P[-1]
                    dtau = np.where(live, g * Te - (total - P), dtype(0)).astype(dtype)
                    rows = np.zeros((len(w), 7), dtype)
                    rows[:, 0] = (ds * dt).astype(dtype) * dtau
                    rows[:, 1:] = S.normal_backward(n, s2, r, (w[:, None] * go[None, :]).astype(dtype), inv_2eps, dtype)
                    grads.append(rows)
    cat = lambda v, t, shape: np.concatenate(v).astype(t) if v else np.zeros(shape, t)
    out = dict(image=image, w=cat(ws, dtype, 0), live=cat(lives, bool, 0))
    if go_all is not None:
        out["grad"] = cat(grads, dtype, (0, 7))
    return out


def central_difference(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, dN, entries, h=1e-6, T_thresh=T_THRESH):
    """d sum(image * dN) / d sigmas7[e] for e in `entries` (flat indices into sigmas7), by float64 central differences of
    truth()'s forward with a step of h * max(1, |value|)."""
    base = np.asarray(sigmas7, dtype=np.float32).astype(np.float64)
    go = np.asarray(dN, dtype=np.float32).astype(np.float64)

    def value(sig):
        sg, d = sig.reshape(-1, 7), np.asarray(deltas, dtype=np.float32).astype(np.float64)
        ds, thr, tot = float(np.float32(density_scale)), float(np.float32(T_thresh)), 0.0
        for rid, off, cnt in np.asarray(rays).tolist():
            s = slice(off, off + cnt)
            n, _, _ = fd_normal_f64(sg[s], inv_2eps)
            tau = (ds * sg[s, 0]) * d[s, 0]
            excl = np.concatenate([[0.0], np.cumsum(tau)[:-1]]) if cnt else np.zeros(0)
            T = np.exp(-excl)
            w = np.where(T >= thr, (1.0 - np.exp(-tau)) * T, 0.0)
            tot += float(((w[:, None] * n).sum(0) * go[rid]).sum())
        return tot

    out = np.zeros(len(entries))
    for k, e in enumerate(entries):
        step = h * max(1.0, abs(base[e]))
        up, dn = base.copy(), base.copy()
        up[e] += step
        dn[e] -= step
        out[k] = (value(up) - value(dn)) / (2.0 * step)
    return out


def fd_normal_f64(sg, inv_2eps):
    """fd_normal on float64 VALUES (no rounding of the input to float32: the central differences move it by 1e-6)."""
    k = float(np.float32(inv_2eps))
    with np.errstate(all="ignore"):
        g = np.stack([(sg[:, 1 + 2 * a] - sg[:, 2 + 2 * a]) * k for a in range(3)], -1)
        s2 = (g * g).sum(-1)
        r = 1.0 / np.sqrt(np.fmax(s2, float(FLOOR)))
        n = -(g * r[:, None])
    return np.where(np.isnan(n), 0.0, n), s2, r


def f32_errors(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, dN, T_thresh=T_THRESH):
    """The float32 restatement against truth(), per ray id -> dict(fwd [n_ids] = max_a |image32 - image64|, centre [n_ids]
    = max_s |row 0|, stencil [n_ids] = max_s max over rows 1..6, t64 = truth()'s dict, r32 = the restatement's)."""
    r32 = restate(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, T_thresh, dN, np.float32)
    t64 = truth(sigmas7, deltas, rays, n_ids, inv_2eps, density_scale, T_thresh, dN)
    diff = np.abs(r32["grad"].astype(np.float64) - t64["grad"])
    return dict(fwd=np.abs(r32["image"].astype(np.float64) - t64["image"]).max(-1),
                centre=per_ray_max(diff[:, 0], rays, n_ids), stencil=per_ray_max(diff[:, 1:], rays, n_ids), t64=t64, r32=r32)


# ------------------------------------------------------------------------------------------ the 2D smoothness stencil
def smooth_forward(img, dtype=np.float32):
    """img [B,H,W,C] -> loss [B,H,W,2] in `dtype`, sums from c = 0 upward."""
    x = np.asarray(img, dtype=np.float32).astype(dtype)
    B, H, W, C = x.shape
    loss = np.zeros((B, H, W, 2), dtype)
    for ch, (a, b) in enumerate(((x[:, :, 1:], x[:, :, :-1]), (x[:, 1:], x[:, :-1]))):
        d = (a - b).astype(dtype)
        acc = (d[..., 0] * d[..., 0]).astype(dtype)
        for c in range(1, C):
            acc = (acc + (d[..., c] * d[..., c]).astype(dtype)).astype(dtype)
        if ch == 0:
            loss[:, :, :-1, 0] = acc
        else:
            loss[:, :-1, :, 1] = acc
    return loss


def smooth_backward(img, d_loss, dtype=np.float32):
    """Gather form in the header's order (own-h, own-v, left, up) -> d_img [B,H,W,C] in `dtype`."""
    x = np.asarray(img, dtype=np.float32).astype(dtype)
    dl = np.asarray(d_loss, dtype=np.float32).astype(dtype)
    two = dtype(2)
    acc = np.zeros_like(x)
    kh, kv = (two * dl[..., 0]).astype(dtype)[..., None], (two * dl[..., 1]).astype(dtype)[..., None]
    acc[:, :, :-1] = (acc[:, :, :-1] - (kh[:, :, :-1] * (x[:, :, 1:] - x[:, :, :-1]).astype(dtype)).astype(dtype)).astype(dtype)
    acc[:, :-1] = (acc[:, :-1] - (kv[:, :-1] * (x[:, 1:] - x[:, :-1]).astype(dtype)).astype(dtype)).astype(dtype)
    acc[:, :, 1:] = (acc[:, :, 1:] + (kh[:, :, :-1] * (x[:, :, 1:] - x[:, :, :-1]).astype(dtype)).astype(dtype)).astype(dtype)
    acc[:, 1:] = (acc[:, 1:] + (kv[:, :-1] * (x[:, 1:] - x[:, :-1]).astype(dtype)).astype(dtype)).astype(dtype)
    return acc


def smooth_truth_backward(img, d_loss):
    """float64, scatter form: every pair hands +-2 d_loss (a - b) to its two pixels."""
    x = np.asarray(img, dtype=np.float32).astype(np.float64)
    dl = np.asarray(d_loss, dtype=np.float32).astype(np.float64)
    B, H, W, C = x.shape
    out = np.zeros_like(x)
    for b in range(B):
        for y in range(H):
            for xx in range(W):
                if xx + 1 < W:
                    t = 2.0 * dl[b, y, xx, 0] * (x[b, y, xx + 1] - x[b, y, xx])
                    out[b, y, xx + 1] += t
                    out[b, y, xx] -= t
                if y + 1 < H:
                    t = 2.0 * dl[b, y, xx, 1] * (x[b, y + 1, xx] - x[b, y, xx])
                    out[b, y + 1, xx] += t
                    out[b, y, xx] -= t
    return out


SMOOTH_SHAPES = ((1, 1, 1, 3), (1, 1, 5, 3), (1, 5, 1, 3), (2, 3, 4, 3), (1, 4, 4, 1))


def smooth_case(shape, seed=0):
    """(img [B,H,W,C], d_loss [B,H,W,2]) f32, normal deviates."""
    rng = np.random.default_rng(1000 + seed)
    return (rng.standard_normal(shape).astype(np.float32),
            rng.standard_normal(tuple(shape[:3]) + (2,)).astype(np.float32))


# ------------------------------------------------------------------------------------------ the op-level case of the tests
COUNTS = (0, 1, 3, 63, 64, 65, 130)             # both sides of the chunk edge, two carries on the last ray
IDS = (5, 2, 7, 0, 3, 6, 1)                     # permuted; id 4 of N_IDS is carried by no ray
N_IDS, SENTINEL_ROWS = 8, 5                     # rows behind the last span that nobody may write
R_EMPTY, R_DEGENERATE, R_NAN, R_KILL = 0, 3, 4, 6
I_DEGENERATE, I_NAN = 10, 5                     # sample of ray R_DEGENERATE with six equal offsets; of R_NAN with a NaN offset
EPS = 1e-2
INV_2EPS = float(np.float32(1.0 / (2.0 * EPS)))
DENSITY_SCALES = (1.0, 0.5)
SEED = 0


def op_case(seed=SEED):
    """7 rays with permuted ids among 8.  dt in [0.005, 0.02], t increasing with gaps as the occupancy skips produce;
    sigma dt is about 0.03 on average, 0.25 on the last ray (130 samples), which goes opaque mid-span at density_scale 1 (in
    its first chunk) and 0.5 (in its second).  The six offset densities are the centre's plus a smooth gradient and noise.
    One sample has six equal offsets (s2 = 0 <= 1e-20: n = -0, the projection is skipped).  One sample has a NaN in its +x
    offset and equal y and z pairs: s2 is NaN, r is the floor's 1e10, all three components of n are 0 (the x one by the NaN
    rule) -- with unequal y / z pairs they would be g 1e10, outside |n| <= 1, which the forward's scale of 1 rests on.
    -> dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    N, cnts = len(COUNTS), np.array(COUNTS)
    offs = np.concatenate([[0], np.cumsum(cnts)[:-1]])
    M = int(cnts.sum())
    cap = M + SENTINEL_ROWS
    rays = np.stack([np.array(IDS), offs, cnts], -1).astype(np.int32)
    deltas = np.zeros((cap, 2), np.float32)
    sig7 = np.zeros((cap, 7), np.float32)
    for r, (off, cnt) in enumerate(zip(offs, cnts)):
        dt = rng.uniform(0.005, 0.02, cnt)
        gap = np.where(rng.random(cnt) < 0.2, rng.uniform(0.0, 0.05, cnt), 0.0)
        t = 0.3 + np.cumsum(np.concatenate([[0.0], (dt + gap)[:-1]])) if cnt else np.zeros(0)
        tau = rng.uniform(0.0, 2.0, cnt) * (0.25 if r == R_KILL else 0.03)
        centre = tau / dt
        grad = rng.standard_normal((cnt, 3)) * (0.5 * centre[:, None] + 0.2)       # per unit length; eps = 0.01
        for a in range(3):
            noise = rng.standard_normal((cnt, 2)) * 0.01
            sig7[off:off + cnt, 1 + 2 * a] = centre + EPS * grad[:, a] + noise[:, 0]
            sig7[off:off + cnt, 2 + 2 * a] = centre - EPS * grad[:, a] + noise[:, 1]
        sig7[off:off + cnt, 0] = centre
        deltas[off:off + cnt, 0], deltas[off:off + cnt, 1] = dt, t
    s = offs[R_DEGENERATE] + I_DEGENERATE
    sig7[s, 0] = 0.05 / deltas[s, 0]                     # (sigma dt = 0.05: a weight that counts)
    sig7[s, 1:] = sig7[s, 0] + np.float32(0.125)
    s = offs[R_NAN] + I_NAN
    sig7[s, 0] = 0.05 / deltas[s, 0]
    sig7[s, 1] = np.nan
    sig7[s, 4], sig7[s, 6] = sig7[s, 3], sig7[s, 5]
    sig7[M:], deltas[M:] = 7.0, 3.0                      # rows outside every span: finite, read by nobody
    dN = rng.standard_normal((N_IDS, 3)).astype(np.float32)
    return dict(sig7=sig7.reshape(-1), deltas=deltas, rays=rays, dN=dN, N=N, M=M, cap=cap, n_ids=N_IDS,
                ids=np.array(IDS), offs=offs)


def check_case(k):
    """The preconditions of the comparison, for every density scale: every reference T at least 1e-3 (relative) away from
    T_thresh (float32 and float64 agree on which samples are live), the last ray goes opaque mid-span with at least ten
    samples on either side, no other ray does, the degenerate and the NaN sample are what the docstring says and are LIVE
    with a weight that counts.  -> {density_scale: truth()'s dict}."""
    out = {}
    for ds in DENSITY_SCALES:
        t = truth(k["sig7"], k["deltas"], k["rays"], k["n_ids"], INV_2EPS, ds, T_THRESH, k["dN"])
        assert float((np.abs(t["T"] - T_THRESH) / T_THRESH).min()) >= 1e-3
        at = np.concatenate([[0], np.cumsum(k["rays"][:, 2])])
        dead = ~t["live"]
        kill = dead[at[R_KILL]:at[R_KILL + 1]]
        assert 10 <= int(kill.sum()) <= COUNTS[R_KILL] - 10 and not dead[:at[R_KILL]].any()
        assert (int((~kill).sum()) < CHUNK) == (ds == 1.0)            # the cut falls in the first / the second chunk
        sg = k["sig7"].reshape(-1, 7)
        for ray, i in ((R_DEGENERATE, I_DEGENERATE), (R_NAN, I_NAN)):
            assert t["w"][at[ray] + i] > 1e-3 and t["r"][at[ray] + i] == 1.0 / np.sqrt(float(FLOOR))
            assert not t["n"][at[ray] + i].any()
        assert np.isnan(sg[k["offs"][R_NAN] + I_NAN]).sum() == 1 and np.isnan(sg).sum() == 1
        assert len(set(sg[k["offs"][R_DEGENERATE] + I_DEGENERATE, 1:].tolist())) == 1
        assert np.isfinite(t["image"]).all() and np.isfinite(t["grad"]).all()
        out[ds] = t
    return out
