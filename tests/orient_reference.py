"""References of the orientation regulariser of the shaded renders (csrc/shade.hip, ORIENT = true; contract in
include/lnerf_hip.h, "orientation regulariser"):  orient[ray] = sum_i w_i max(0, n_i . v)^2.

Built on tests/shading_reference.py (imported unchanged).  The per-sample terms -- the normal n, q = max(0, n . v) and the
per-unit gradient U (the seven dsigmas7 rows of one sample for e = go w = 1) -- are written ONCE, in the kernel's op order,
for any dtype: at float32 they are the op-order restatement (n is shading_reference._lambert's bit for bit,
tests/test_orient_cpu.py checks it), at float64 they are the reference the kernels are compared with.  The compositing
weights w are float64 always (the kernel's come from expf and a 64-lane scan: tolerance-checked), with the kernel's kill
rule T >= T_thresh.

  sample_terms()      n, s, r, d, lam, v, c, q of every span row
  weights()           w, T, tau per span row (float64)
  orient_forward()    orient [n_ids] (float64)
  orient_backward()   the seven dsigmas7 rows per span row, the Lambert part and the orientation part SEPARATELY, the
                      albedo rows, and U
  orient_torch() / total_torch()   the definition in torch (float64 in the tests) with autograd, weights detached: the numpy
                      gradient must match it
  op_case()           the op-level inputs of tests/test_gpu_orient.py and check_case(), their preconditions"""
import numpy as np
import torch

from tests import shading_reference as R
from tests import span_reference as S

FLOOR = 1e-20


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def view_dirs(rays_d, dtype=np.float64):
    """rays_d [n,3] -> unit directions, the kernel's op order: d * (1 / sqrt(fmax((dx dx + dy dy) + dz dz, 1e-20)))."""
    d = np.asarray(rays_d, dtype=np.float32).astype(dtype)
    s = _dot3(d, d)
    r = dtype(1.0) / np.sqrt(np.fmax(s, dtype(FLOOR)))
    return (d * r[:, None]).astype(dtype)


def sample_terms(sigmas7, rays, shade, rays_per_view, inv_2eps, rays_d, dtype=np.float64):
    """Per span row (ray order): rows, ids, sg [m,7], light, ambient, textureless, n [m,3], s, r, d, lam, v [m,3], c, q."""
    rows, ids = R._span_rows(rays)
    shade = np.asarray(shade, dtype=np.float32)
    rec = shade[R._views(ids, rays_per_view, shade.shape[0])].astype(dtype)
    light, ambient, tl = rec[:, :3], rec[:, 3], rec[:, 4] != 0
    sg = np.asarray(sigmas7, dtype=np.float32).reshape(-1, 7)[rows].astype(dtype)
    inv = dtype(np.float32(inv_2eps))
    n, s, r = S.fd_normal(sg, inv_2eps, dtype)
    with np.errstate(all="ignore"):
        d = _dot3(n, light)
        lam = ambient + (dtype(1.0) - ambient) * np.where(d > 0, d, dtype(0.0))
        v = view_dirs(rays_d, dtype)[ids]
        c = _dot3(n, v)
        q = np.where(c > 0, c, dtype(0.0)).astype(dtype)
    return dict(rows=rows, ids=ids, sg=sg, light=light, ambient=ambient, tl=tl, inv=inv, n=n, s=s, r=r, d=d, lam=lam, v=v,
                c=c, q=q)


def weights(sigma_c, deltas, rays, density_scale, T_thresh):
    """float64 compositing weights of every span row (ray order) on sigma' = density_scale * sigma_c -> (w, T, tau):
    span_reference.weights."""
    return S.weights(sigma_c, deltas, rays, T_thresh, density_scale)


def orient_forward(sigmas7, rays, shade, rays_per_view, inv_2eps, deltas, rays_d, density_scale, T_thresh, n_ids):
    """-> orient float64 [n_ids]: per ray id the sum of w (q q) over its span (0 for an empty span / an id of no ray)."""
    t = sample_terms(sigmas7, rays, shade, rays_per_view, inv_2eps, rays_d)
    w, _, _ = weights(np.asarray(sigmas7).reshape(-1, 7)[:, 0], deltas, rays, density_scale, T_thresh)
    out = np.zeros(int(n_ids))
    np.add.at(out, t["ids"], w * (t["q"] * t["q"]))
    return out


def _project(t, dn, dtype):
    """dn [m,3] -> the six offset rows of dsigmas7 (columns 1..6 of [m,7]; column 0 is left 0), the kernel's op order."""
    ds = np.zeros((len(t["s"]), 7), dtype=dtype)
    ds[:, 1:] = S.normal_backward(t["n"], t["s"], t["r"], dn.astype(dtype), t["inv"], dtype)
    return ds


def orient_backward(sigmas7, rgbs7, rays, shade, rays_per_view, inv_2eps, dsigma_c, dcolours, deltas, rays_d, density_scale,
                    T_thresh, d_orient, dtype=np.float64):
    """Per span row (ray order) -> dict(rows, ids, lam [m,7], orient [m,7], dalb [m,C], U [m,7], w [m], go [m]):
    `lam` the rows lnerf_shade_fd_backward writes to dsigmas7 (row 0 = dsigma_c), `orient` what the term adds (weights
    detached; d_orient None: zeros), U the term's rows per unit e = go w.  dsigmas7 of the fused backward = lam + orient
    up to the rounding of the ONE addition the kernel makes (in dn, before the projection, which is linear)."""
    t = sample_terms(sigmas7, rays, shade, rays_per_view, inv_2eps, rays_d, dtype)
    rows, ids = t["rows"], t["ids"]
    cap = len(np.asarray(sigmas7).reshape(-1)) // 7
    alb = np.asarray(rgbs7, dtype=np.float32).reshape(cap, 7, -1)[rows, 0].astype(dtype)
    C = alb.shape[1]
    dcol = np.asarray(dcolours, dtype=np.float32)[rows].astype(dtype)
    dl_t, dl_l = dcol[:, 0].copy(), dcol[:, 0] * alb[:, 0]
    for c in range(1, C):
        dl_t = dl_t + dcol[:, c]
        dl_l = dl_l + dcol[:, c] * alb[:, c]
    dlam = np.where(t["tl"], dl_t, dl_l)
    dalb = np.where(t["tl"][:, None], dtype(0.0), dcol * t["lam"][:, None]).astype(dtype)
    k = (dtype(1.0) - t["ambient"]) * dlam
    dn_lam = np.where((t["d"] > 0)[:, None], k[:, None] * t["light"], dtype(0.0)).astype(dtype)
    lam = _project(t, dn_lam, dtype)
    lam[:, 0] = np.asarray(dsigma_c, dtype=np.float32)[rows].astype(dtype)
    U = _project(t, (dtype(2.0) * t["q"])[:, None] * t["v"], dtype)
    w, _, _ = weights(np.asarray(sigmas7).reshape(-1, 7)[:, 0], deltas, rays, density_scale, T_thresh)
    go = np.zeros(len(rows)) if d_orient is None else np.asarray(d_orient, dtype=np.float32).astype(np.float64)[ids]
    return dict(rows=rows, ids=ids, lam=lam, orient=(go * w)[:, None] * U.astype(np.float64), dalb=dalb, U=U, w=w, go=go)


# ------------------------------------------------------------------------------------------ torch, with autograd
def weights_torch(sigma, dt, rays, density_scale, T_thresh):
    """sigma [m], dt [m] in SPAN-ROW order (ray after ray), rays [N,3] -> the compositing weights [m], DETACHED."""
    out, at = [], 0
    with torch.no_grad():
        for _, _, cnt in torch.as_tensor(rays).tolist():
            tau = (density_scale * sigma[at:at + cnt]) * dt[at:at + cnt]
            excl = torch.cat([tau.new_zeros(1), torch.cumsum(tau, 0)[:-1]]) if cnt else tau
            T = torch.exp(-excl)
            out.append(torch.where(T >= T_thresh, (1.0 - torch.exp(-tau)) * T, torch.zeros_like(T)))
            at += cnt
    return torch.cat(out) if out else sigma.new_zeros(0)


def orient_torch(sg, v, w, ray_of_row, n_ids, inv_2eps):
    """The definition: sg [m,7] (differentiable), v [m,3] unit view directions, w [m] weights (constants), ray_of_row
    int64 [m] -> orient [n_ids] = sum over each ray's rows of w max(0, n . v)^2, n as shading_reference.shade_torch."""
    g = torch.stack([(sg[:, 1 + 2 * a] - sg[:, 2 + 2 * a]) * inv_2eps for a in range(3)], -1)
    s = (g * g).sum(-1)
    r = 1.0 / torch.sqrt(torch.clamp(s, min=FLOOR))
    n = -(g * r[:, None])
    n = torch.where(torch.isnan(n), torch.zeros_like(n), n)
    c = (n * v).sum(-1)
    q = torch.where(c > 0, c, torch.zeros_like(c))
    return torch.zeros(int(n_ids), dtype=sg.dtype).index_add(0, ray_of_row, w.detach() * q * q)


def total_torch(sigmas7, rgbs7, rays, shade, rays_per_view, inv_2eps, dsigma_c, dcolours, deltas, rays_d, density_scale,
                T_thresh, d_orient, n_ids):
    """float64 autograd of  sum(colours dcolours) + sum(sigma_c dsigma_c) + sum(orient d_orient)  over the span rows
    -> (d/d sg [m,7], d/d albedo [m,C], orient [n_ids]) in ray order."""
    rows, ids = R._span_rows(rays)
    shade = np.asarray(shade, dtype=np.float32)
    rec = torch.from_numpy(shade[R._views(ids, rays_per_view, shade.shape[0])]).double()
    cap = len(np.asarray(sigmas7).reshape(-1)) // 7
    sg = torch.from_numpy(np.asarray(sigmas7, dtype=np.float32).reshape(cap, 7)[rows]).double().requires_grad_()
    alb = torch.from_numpy(np.asarray(rgbs7, dtype=np.float32).reshape(cap, 7, -1)[rows, 0]).double().requires_grad_()
    col, _ = R.shade_torch(sg, alb, rec[:, :3], rec[:, 3], rec[:, 4] != 0, float(np.float32(inv_2eps)))
    v = torch.from_numpy(view_dirs(rays_d))[ids]
    dt = torch.from_numpy(np.asarray(deltas, dtype=np.float32)[rows, 0]).double()
    w = weights_torch(sg[:, 0], dt, rays, float(density_scale), float(T_thresh))
    ori = orient_torch(sg, v, w, torch.from_numpy(ids), n_ids, float(np.float32(inv_2eps)))
    total = (col * torch.from_numpy(np.asarray(dcolours, dtype=np.float32)[rows]).double()).sum()
    total = total + (sg[:, 0] * torch.from_numpy(np.asarray(dsigma_c, dtype=np.float32)[rows]).double()).sum()
    if d_orient is not None:
        total = total + (ori * torch.from_numpy(np.asarray(d_orient, dtype=np.float32)).double()).sum()
    total.backward()
    return sg.grad, alb.grad, ori.detach()


# ------------------------------------------------------------------------------------------ the op-level case of the tests
COUNTS = (0, 1, 2, 63, 64, 65, 130, 200)       # the chunk edges and the carry
IDS = (3, 0, 4, 1, 6, 7, 5, 2)                 # ray r -> id, a permutation with id != r
RAYS_PER_VIEW, N_VIEWS, EPS, T_THRESH, SENTINEL_ROWS = 4, 2, 1e-2, 1e-4, 17
R_BACK, R_LONG, R_KILL = 5, 6, 7               # the back-facing ray (65), a two-carry ray that stays alive (130), the killed one
I_OPAQUE, I_FLAT = 70, 9                       # the opaque sample of R_KILL (second chunk); the g = 0 sample of R_KILL
SEED = 4          # (chosen on the CPU: the preconditions of check_case hold for both density scales)


def op_case(C, density_scale, seed=SEED):
    """N = 8 rays in 2 views (view 0 lambertian, view 1 textureless), see tests/test_gpu_orient.py.  The densities and
    normals do not depend on C or density_scale; dt is divided by density_scale, so that sigma' dt is the same design
    for every scale.  -> dict of numpy arrays."""
    rng = np.random.default_rng(seed)
    N, cnts = len(COUNTS), np.array(COUNTS)
    offs = np.concatenate([[0], np.cumsum(cnts)[:-1]])
    rays = np.stack([np.array(IDS), offs, cnts], -1).astype(np.int32)
    M = int(cnts.sum())
    cap = M + SENTINEL_ROWS
    rays_d = (rng.normal(size=(N, 3)) * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)      # not unit
    sig = rng.uniform(0.0, 4.0, (cap, 7)).astype(np.float32)
    dt = rng.uniform(0.005, 0.02, cap)
    # the killed ray: sigma' dt ~ 0.1 on average, one opaque sample (1.45) inside the second chunk -> T < T_thresh there
    o, c = int(offs[R_KILL]), int(cnts[R_KILL])
    dt[o:o + c] = 0.05
    sig[o + I_OPAQUE, 0] = 29.0
    sig[o + I_FLAT] = 2.25                                                       # seven equal densities: g = 0, n = 0
    # the back-facing ray: g = a (v + a small perpendicular part), a > 0, so n . v < 0 on every sample
    o, c = int(offs[R_BACK]), int(cnts[R_BACK])
    v = rays_d[IDS[R_BACK]].astype(np.float64)
    v = v / np.linalg.norm(v)
    g = rng.uniform(20.0, 60.0, (c, 1)) * (v[None] + 0.4 * rng.normal(size=(c, 3)))
    g = np.where(((g @ v) > 0)[:, None], g, g - 2.0 * (g @ v)[:, None] * v[None])     # (mirror the few that turned)
    base = rng.uniform(1.0, 3.0, (c, 3))
    for a in range(3):
        sig[o:o + c, 1 + 2 * a] = base[:, a] + g[:, a] * EPS
        sig[o:o + c, 2 + 2 * a] = base[:, a] - g[:, a] * EPS
    deltas = np.stack([dt / float(density_scale), rng.uniform(0.1, 3.0, cap)], -1).astype(np.float32)
    alb = rng.normal(size=(cap, 7, C)).astype(np.float32)
    l0 = np.array([0.6, 0.0, 0.8])
    l1 = np.array([-0.48, 0.6, -0.64])
    shade = np.array([[*l0, 0.1, 0.0], [*l1, 0.1, 1.0]], dtype=np.float32)
    return dict(rays=rays, M=M, cap=cap, N=N, sig=sig, alb=alb, shade=shade, deltas=deltas, rays_d=rays_d,
                dsig=rng.normal(size=cap).astype(np.float32), dcol=rng.normal(size=(cap, C)).astype(np.float32),
                d_orient=rng.normal(size=N).astype(np.float32), density_scale=float(density_scale), C=C,
                inv=1.0 / (2.0 * EPS))


def check_case(case):
    """The preconditions of the op-level comparisons, on the float64 reference (AssertionError otherwise)."""
    k = case
    t = sample_terms(k["sig"].reshape(-1), k["rays"], k["shade"], RAYS_PER_VIEW, k["inv"], k["rays_d"])
    w, T, tau = weights(k["sig"][:, 0], k["deltas"], k["rays"], k["density_scale"], T_THRESH)
    assert float(tau.max()) <= 1.5, float(tau.max())
    margin = np.abs(T - T_THRESH) / T_THRESH
    assert float(margin.min()) >= 1e-3, float(margin.min())
    ang_v = np.arccos(np.clip(t["c"], -1, 1))[t["q"] > 0]
    ang_l = np.arccos(np.clip(t["d"], -1, 1))[t["d"] > 0]
    assert float(ang_v.min()) > 0.1 and float(ang_l.min()) > 0.1, (float(ang_v.min()), float(ang_l.min()))
    # what the case is for: the kill inside the second chunk of R_KILL, the back-facing ray, the flat sample
    at = np.concatenate([[0], np.cumsum(k["rays"][:, 2])])
    kill = T[at[R_KILL]:at[R_KILL + 1]] < T_THRESH
    first = int(np.argmax(kill))
    assert kill.any() and 64 <= first < 128 and first > I_OPAQUE, first
    assert not (T[at[R_LONG]:at[R_LONG + 1]] < T_THRESH).any()
    assert float(t["q"][at[R_BACK]:at[R_BACK + 1]].max()) == 0.0 and float(t["c"][at[R_BACK]:at[R_BACK + 1]].max()) < -0.05
    assert float(t["s"][at[R_KILL] + I_FLAT]) == 0.0
    for view in (0, 1):
        sel = (t["ids"] // RAYS_PER_VIEW) == view
        assert (t["q"][sel] > 0).any() and (t["d"][sel] > 0).any() and (t["d"][sel] < 0).any()
    return t, w, T
