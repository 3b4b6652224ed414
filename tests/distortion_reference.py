"""References of the distortion loss of the training renders (csrc/distortion.hip; contract in include/lnerf_hip.h,
"distortion loss"):  loss[ray] = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i.

  weights()             w, T, tau per span row (float64), the kernel's kill rule T >= T_thresh (tests/span_reference.py,
                        which also holds span_rows(), per_ray_max() and the chunk's exclusive sum)
  double_sum()          the DEFINITION in float64: the O(k^2) double sum over the unshifted mid-points m = t + dt / 2 --
                        no prefix sums, no shift by t_0, nothing of the kernels' algebra
  double_sum_torch()    the same double sum in torch (float64 in the tests), weights NOT detached: its autograd gives the
                        reference gradient
  restate()             the header's arithmetic, operation by operation, for any dtype: chunks of 64 with scalar
                        carries, the exclusive sums taken from the previous lane, A_tot / B_tot / 2 L in the backward.
                        (Inside a chunk numpy's cumsum adds left to right where the kernel's scan adds as a tree, and
                        numpy's exp is not expf: the restatement measures the arithmetic's own error, it is no bit model.)
  f32_errors()          the float32 restatement's error against float64, per ray: the yardstick of the GPU tests
  op_case()             the op-level input of tests/test_gpu_distortion.py and check_case(), its preconditions"""
import numpy as np
import torch

from tests import span_reference as S
from tests.span_reference import CHUNK, per_ray_max, span_rows    # (the tests reach them through this module)

T_THRESH = 1e-4


def weights(sigmas, deltas, rays, T_thresh=T_THRESH):
    """float64 compositing weights of every span row (ray order) -> (w, T, tau): span_reference.weights."""
    return S.weights(sigmas, deltas, rays, T_thresh)



def double_sum(sigmas, deltas, rays, n_ids, T_thresh=T_THRESH):
    """The definition, float64 -> loss [n_ids] (0 for an empty span / an id of no ray)."""
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64)
    w, _, _ = weights(sigmas, deltas, rays, T_thresh)
    out, at = np.zeros(int(n_ids)), 0
    for rid, off, cnt in np.asarray(rays).tolist():
        wr, dt, t = w[at:at + cnt], d[off:off + cnt, 0], d[off:off + cnt, 1]
        m = t + 0.5 * dt
        out[rid] = float((wr[:, None] * wr[None, :] * np.abs(m[:, None] - m[None, :])).sum() + (wr * wr * dt).sum() / 3.0)
        at += cnt
    return out


def double_sum_torch(sigma_rows, deltas, rays, n_ids, T_thresh=T_THRESH):
    """sigma_rows [m] in SPAN-ROW order (differentiable), deltas numpy [cap,2], rays [N,3] -> loss [n_ids]; the weights
    are part of the graph (the kill mask alone is a constant)."""
    d = torch.from_numpy(np.asarray(deltas, dtype=np.float32)).to(sigma_rows.dtype)
    out, at = [], 0
    ids = []
    for rid, off, cnt in np.asarray(rays).tolist():
        sg, dt, t = sigma_rows[at:at + cnt], d[off:off + cnt, 0], d[off:off + cnt, 1]
        tau = sg * dt
        excl = torch.cat([tau.new_zeros(1), torch.cumsum(tau, 0)[:-1]]) if cnt else tau
        T = torch.exp(-excl)
        w = torch.where(T >= T_thresh, (1.0 - torch.exp(-tau)) * T, torch.zeros_like(T))
        m = t + 0.5 * dt
        out.append((w[:, None] * w[None, :] * (m[:, None] - m[None, :]).abs()).sum() + (w * w * dt).sum() / 3.0)
        ids.append(rid)
        at += cnt
    loss = sigma_rows.new_zeros(int(n_ids))
    if out:
        loss = loss.index_add(0, torch.tensor(ids, dtype=torch.long), torch.stack(out))
    return loss


def restate(sigmas, deltas, rays, n_ids, T_thresh=T_THRESH, d_loss=None, dtype=np.float32):
    """The header's order of operations in `dtype` -> dict(loss [n_ids], sums [n_ids,2], w [m], live [m], m [m] in ray
    order, and with d_loss [n_ids]: dsigmas [m], the gradient rows of every span)."""
    sig = np.asarray(sigmas, dtype=np.float32).astype(dtype)
    d = np.asarray(deltas, dtype=np.float32).astype(dtype)
    thr = dtype(np.float32(T_thresh))
    third, two_thirds = dtype(1.0) / dtype(3.0), dtype(2.0) / dtype(3.0)
    loss, sums = np.zeros(int(n_ids), dtype), np.zeros((int(n_ids), 2), dtype)
    ws, lives, ms, grads = [], [], [], []
    go_all = None if d_loss is None else np.asarray(d_loss, dtype=np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        for rid, off, cnt in np.asarray(rays).tolist():
            t0 = d[off, 1] if cnt else dtype(0)
            c_tau = c_A = c_B = dtype(0)
            acc = dtype(0)
            rec = []
            for base in range(0, cnt, CHUNK):
                s = slice(off + base, off + min(base + CHUNK, cnt))
                dt, t = d[s, 0], d[s, 1]
                tau = sig[s] * dt
                _, excl, c_tau = S.chunk_excl(tau, c_tau, dtype)
                T = np.exp(-excl).astype(dtype)
                e = np.exp(-tau).astype(dtype)
                alpha = dtype(1) - e
                live = T >= thr
                w = np.where(live, alpha * T, dtype(0)).astype(dtype)
                m = (t - t0) + dtype(0.5) * dt
                _, A, c_A = S.chunk_excl(w, c_A, dtype)
                _, B, c_B = S.chunk_excl(w * m, c_B, dtype)
                u = m * A - B
                acc = dtype(acc + (w * (dtype(2) * u + third * (w * dt))).sum(dtype=dtype))
                rec.append((dt, w, m, u, T * e, live))
            loss[rid], sums[rid] = acc, (c_A, c_B)
            for dt, w, m, u, Te, live in rec:
                ws.append(w); lives.append(live); ms.append(m)
            if go_all is not None:
                go, total, c_g = go_all[rid], dtype(acc + acc), dtype(0)
                for dt, w, m, u, Te, live in rec:
                    g = dtype(2) * ((u + u) + (c_B - m * c_A)) + two_thirds * (w * dt)
                    inc = np.cumsum(g * w, dtype=dtype)
                    P = (inc + c_g).astype(dtype)
                    c_g = P[-1]
                    dtau = np.where(live, g * Te - (total - P), dtype(0))
                    grads.append(((go * dt) * dtau).astype(dtype))
    cat = lambda v, t: np.concatenate(v).astype(t) if v else np.zeros(0, t)
    out = dict(loss=loss, sums=sums, w=cat(ws, dtype), live=cat(lives, bool), m=cat(ms, dtype))
    if go_all is not None:
        out["dsigmas"] = cat(grads, dtype)
    return out


def reference_gradient(sigmas, deltas, rays, n_ids, d_loss, T_thresh=T_THRESH):
    """float64 autograd of sum(double_sum_torch * d_loss) -> (loss [n_ids], dsigmas [m] in span-row order), numpy."""
    rows, _ = span_rows(rays)
    sg = torch.from_numpy(np.asarray(sigmas, dtype=np.float32)[rows]).double().requires_grad_()
    loss = double_sum_torch(sg, deltas, rays, n_ids, float(T_thresh))
    (loss * torch.from_numpy(np.asarray(d_loss, dtype=np.float32)).double()).sum().backward()
    grad = sg.grad if sg.grad is not None else torch.zeros_like(sg)
    return loss.detach().numpy(), grad.numpy()


def f32_errors(sigmas, deltas, rays, n_ids, d_loss, T_thresh=T_THRESH):
    """The float32 restatement against float64 (the double sum, and its autograd gradient), per ray id ->
    dict(fwd [n_ids] = |loss32 - loss64|, bwd [n_ids] = max_s |dsigma32 - dsigma64|, loss64, grad64 [m], r32)."""
    r32 = restate(sigmas, deltas, rays, n_ids, T_thresh, d_loss, np.float32)
    loss64, grad64 = reference_gradient(sigmas, deltas, rays, n_ids, d_loss, T_thresh)
    fwd = np.abs(r32["loss"].astype(np.float64) - loss64)
    bwd = per_ray_max(r32["dsigmas"].astype(np.float64) - grad64, rays, n_ids)
    return dict(fwd=fwd, bwd=bwd, loss64=loss64, grad64=grad64, r32=r32)


# ------------------------------------------------------------------------------------------ the op-level case of the tests
COUNTS = (0, 1, 2, 63, 64, 65, 128, 129, 200, 130, 40, 64, 3, 127, 65, 192)   # both sides of every chunk edge, two carries
N_IDS, SENTINEL_ROWS = 20, 17                   # more ids than rays; rows behind the last span that nobody may write
R_EMPTY, R_KILL, R_HUGE = 0, 8, 9               # the empty ray; the ray that goes opaque mid-span (200); the huge-tau ray (130)
I_HUGE, TAU_HUGE = 70, 80.0                     # the huge sample sits in the second chunk of R_HUGE
SEED = 3          # (chosen on the CPU: check_case holds with no sample left out)


def op_case(seed=SEED):
    """16 rays with shuffled ids among 20.  t increases along every span, with gaps between samples as the occupancy
    skips produce; sigma dt is about 0.025 on average, 0.1 on the ray that goes opaque; one sample of one ray has
    sigma dt = 80.  -> dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    N, cnts = len(COUNTS), np.array(COUNTS)
    offs = np.concatenate([[0], np.cumsum(cnts)[:-1]])
    ids = rng.permutation(N_IDS)[:N]
    rays = np.stack([ids, offs, cnts], -1).astype(np.int32)
    M = int(cnts.sum())
    cap = M + SENTINEL_ROWS
    sig = rng.uniform(0.0, 4.0, cap)
    dt = rng.uniform(0.005, 0.02, cap)
    o, c = int(offs[R_KILL]), int(cnts[R_KILL])
    dt[o:o + c] = 0.05                                    # tau ~ 0.1: T falls below 1e-4 near sample 90
    gap = np.where(rng.uniform(size=cap) < 0.3, rng.uniform(0.0, 0.05, cap), 0.0)
    t = np.zeros(cap)
    for r in range(N):
        o, c = int(offs[r]), int(cnts[r])
        if c:
            start = rng.uniform(0.1, 1.0)
            t[o:o + c] = start + np.concatenate([[0.0], np.cumsum((dt + gap)[o:o + c])[:-1]])
    t[M:] = rng.uniform(0.1, 3.0, cap - M)
    deltas = np.stack([dt, t], -1).astype(np.float32)
    sig = sig.astype(np.float32)
    s = int(offs[R_HUGE]) + I_HUGE
    sig[s] = np.float32(TAU_HUGE / float(deltas[s, 0]))
    return dict(rays=rays, ids=ids, N=N, n_ids=N_IDS, M=M, cap=cap, sig=sig, deltas=deltas,
                d_loss=rng.normal(size=N_IDS).astype(np.float32))


def check_case(case):
    """The preconditions of the op-level comparisons, on the float64 reference (AssertionError otherwise)."""
    k = case
    rays = k["rays"]
    w, T, tau = weights(k["sig"], k["deltas"], rays)
    at = np.concatenate([[0], np.cumsum(rays[:, 2])])
    rows, _ = span_rows(rays)
    assert np.array_equal(rows, np.arange(k["M"]))
    huge = at[R_HUGE] + I_HUGE
    assert abs(float(tau[huge]) - TAU_HUGE) < 1e-3
    rest = np.ones(len(tau), bool)
    rest[huge] = False
    assert float(tau[rest].max()) <= 1.5, float(tau[rest].max())
    margin = np.abs(T - T_THRESH) / T_THRESH
    assert float(margin.min()) >= 1e-3, float(margin.min())          # every sample: none is left out
    # t increases along every span and a sample ends before the next begins (so that m is monotone), with real gaps
    d = k["deltas"].astype(np.float64)
    n_gaps = 0
    for _, off, cnt in rays.tolist():
        if cnt < 2:
            continue
        step = d[off + 1:off + cnt, 1] - (d[off:off + cnt - 1, 1] + d[off:off + cnt - 1, 0])
        assert (step >= -1e-6).all()
        n_gaps += int((step > 1e-3).sum())
    assert n_gaps > 100
    # what the case is for
    assert sorted(set(COUNTS)) == [0, 1, 2, 3, 40, 63, 64, 65, 127, 128, 129, 130, 192, 200]
    assert len(set(k["ids"].tolist())) == k["N"] < k["n_ids"] and (k["ids"] != np.arange(k["N"])).any()
    kill = T[at[R_KILL]:at[R_KILL + 1]] < T_THRESH
    assert kill.any() and 64 <= int(np.argmax(kill)) < 128, int(np.argmax(kill))
    dead = T[at[R_HUGE]:at[R_HUGE + 1]] < T_THRESH
    assert not dead[:I_HUGE + 1].any() and dead[I_HUGE + 1:].all()
    alive = np.ones(len(T), bool)
    alive[at[R_KILL]:at[R_KILL + 1]] = False
    alive[at[R_HUGE]:at[R_HUGE + 1]] = False
    assert (T[alive] >= T_THRESH).all()
    return w, T, tau
