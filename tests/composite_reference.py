"""float64 reference of the training compositor (csrc/composite.hip, lnerf_composite_rays_train_forward / _backward) with
per-sample outputs, and the input cases shared by tests/test_composite_reference_cpu.py and tests/test_gpu_composite.py.

    image = sum_k w_k c_k + (1 - sum_k w_k) bg,   w_k = alpha_k T_k,   alpha_k = -expm1(-tau_k),   T_k = exp(-sum_{j<k} tau_j)

The exclusive optical depth sum_{j<k} tau_j is the inclusive cumsum SHIFTED BY ONE SLOT, never `cumsum - tau_k`: it is
then exact for any tau_k (a surface sample has sigma dt ~ 1e4 and more; sigma = exp(h) is unclamped), +inf included.
Everything is torch float64 with autograd; gradients are taken with torch.autograd.grad on this graph."""
import math

import torch

ULP = 2.0 ** -24
DT = 3.4e-3
SPANS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
T_THRESHES = (1e-4, 1e-2, 0.0)
REGIMES = ("benign", "one", "empty", "edge", "saturated", "bigbg")
EDGE_B = (1, 63, 64, 65, 128)
EDGE_SPANS = (65, 129, 300)
SAT_SIGMAS = (math.exp(15.0), math.exp(18.0), math.exp(30.0), 3e38, float("inf"))
SAT_POS = (0, 20, 63, 64)
SAT_TAIL = 12                      # thin samples behind the surface sample
EXTRA = 3                          # rows of every output / gradient buffer beyond what the call may touch


def COMPOSITE_TOL(k):
    """The project's compositing bound for a ray of k samples (tests/test_gpu_inference.py)."""
    return 32 * ULP * (k + 1)


def _by_id(ids, values):
    return torch.zeros_like(values).index_add(0, ids, values)


def composite_reference(sigmas, rgbs, deltas, rays, T_thresh=1e-4, bg=None):
    """Inputs as oracle.nerf_oracle.composite_rays_train (float64; bg [N,C] by ray id or None).  Returns a dict:
    weights_sum [N], depth [N], image [N,C] by ray id (differentiable in sigmas, rgbs, bg); per sample (detached) w [M] and
    T [M] (0 outside every span), keep [M] (in a span and T >= T_thresh), in_span [M], pos [M] (index inside its ray, -1
    outside), ray [M] (the id of its ray, -1 outside); per ray id count [N], tmax [N] = max t and rgbmax [N,C] =
    max_k |rgb_kc| over the span (0 for an empty one); margin = the smallest |T - T_thresh| / T_thresh over the samples
    of all spans (inf for T_thresh = 0, where T >= T_thresh cannot fail)."""
    assert sigmas.dtype == torch.float64 and rgbs.dtype == torch.float64 and deltas.dtype == torch.float64
    N, M, C = rays.shape[0], sigmas.shape[0], rgbs.shape[1]
    ids = rays[:, 0].to(torch.int64)
    offs = rays[:, 1].to(torch.int64)
    cnts = rays[:, 2].to(torch.int64)
    K = max(int(cnts.max().item()), 1)
    k = torch.arange(K)
    valid = k[None, :] < cnts[:, None]
    idx = torch.where(valid, (offs[:, None] + k[None, :]).clamp(max=max(M - 1, 0)), torch.zeros(1, dtype=torch.int64))
    zero = torch.zeros(1, dtype=torch.float64)
    sg = torch.where(valid, sigmas[idx], zero)
    dt = torch.where(valid, deltas[idx, 0], zero)
    tt = torch.where(valid, deltas[idx, 1], zero)
    rgb = torch.where(valid[..., None], rgbs[idx], zero)
    tau = sg * dt
    inc = torch.cumsum(tau, 1)
    excl = torch.cat([torch.zeros(N, 1, dtype=torch.float64), inc[:, :-1]], 1)      # shifted, not `inc - tau`
    T = torch.exp(-excl)
    alpha = -torch.expm1(-tau)
    keep = valid & (T >= T_thresh)
    w = torch.where(keep, alpha * T, zero)
    ws = w.sum(1)
    depth = (w * tt).sum(1)
    image = (w[..., None] * rgb).sum(1)
    ws, depth, image = _by_id(ids, ws), _by_id(ids, depth), _by_id(ids, image)
    if bg is not None:
        image = image + (1.0 - ws)[:, None] * bg

    def scatter(values, fill, dtype):
        out = torch.full((M,), fill, dtype=dtype)
        out[idx[valid]] = values[valid].to(dtype)
        return out

    Td = T.detach()
    if T_thresh > 0 and bool(valid.any()):
        margin = float(((Td - T_thresh).abs() / T_thresh)[valid].min())
    else:
        margin = float("inf")
    return {"weights_sum": ws, "depth": depth, "image": image,
            "w": scatter(w.detach(), 0.0, torch.float64), "T": scatter(Td, 0.0, torch.float64),
            "keep": scatter(keep, False, torch.bool), "in_span": scatter(valid, False, torch.bool),
            "pos": scatter(k[None, :].expand(N, K), -1, torch.int64),
            "ray": scatter(ids[:, None].expand(N, K), -1, torch.int64),
            "count": _by_id(ids, cnts), "tmax": _by_id(ids, tt.detach().amax(1)),
            "rgbmax": _by_id(ids, rgb.detach().abs().amax(1)), "margin": margin}


# ------------------------------------------------------------------------------ the input cases
def _table(cnts, g):
    """Ray table over spans of the given lengths, ids a permutation, with samples that belong to no span: 1..3 between
    consecutive spans and 5 behind the last one.  -> rays int32 [N,3], M."""
    N = len(cnts)
    gaps = torch.randint(1, 4, (N,), generator=g)
    offs, at = [], 0
    for c, gap in zip(cnts, gaps.tolist()):
        offs.append(at)
        at += int(c) + gap
    M = at + 5
    rays = torch.stack([torch.randperm(N, generator=g), torch.tensor(offs), torch.tensor(cnts)], -1).to(torch.int32)
    return rays, M


def edge_rays():
    """(span, b) of the stop-boundary rays: every b of EDGE_B on every span of EDGE_SPANS that is at least b long."""
    return [(s, b) for s in EDGE_SPANS for b in EDGE_B if b <= s]


def saturated_rays():
    """(sigma, position) of the saturated rays."""
    return [(s, p) for s in SAT_SIGMAS for p in SAT_POS]


def composite_inputs(regime, C, T_thresh):
    """f32 inputs of one case (deterministic).  dt = 3.4e-3 throughout, t in [0.3, 1.3], rgb ~ N(0, 1), bg in [0, 1)
    unless stated.  N + EXTRA ids exist (output rows); the last EXTRA are named by no ray.

    benign     SPANS; sigma <= 20, the 300-sample span up to 400 (sigma dt <= 1.36): it stops after a few dozen samples
    one        N = 1, one ray of 65 samples, benign densities
    empty      SPANS; sigma in [0, 1e-3] with exact zeros among them (alpha of a few ulp of 1)
    edge       the rays of edge_rays(): constant sigma dt = ln(1 / T_thresh) / (b - 0.5), so that T_i = T_thresh^(i / (b - 0.5))
               and the first dropped sample is index b (relative distance of T_{b-1}, T_b from T_thresh >= 1.8%).
               T_thresh = 0 has no stop: it takes the densities of T_thresh = 1e-4 and nothing is dropped
    saturated  the rays of saturated_rays(): thin samples of total optical depth 2.0 in front (20 of sigma dt = 0.1 at
               position 20; 63 / 64 of 2.0 / position, so that the surface sample is kept at every threshold; none at
               position 0), ONE sample of the listed sigma, then SAT_TAIL thin samples (sigma dt = 0.1)
    bigbg      bg in [-100, 100]; spans (5, 64, 130) once nearly empty (weights_sum ~ 1e-3) and once dense
               (weights_sum ~ 1), and one empty span"""
    g = torch.Generator().manual_seed(1000 * REGIMES.index(regime) + 10 * C + T_THRESHES.index(T_thresh))
    meta = {}
    if regime in ("benign", "empty"):
        cnts = list(SPANS)
    elif regime == "one":
        cnts = [65]
    elif regime == "edge":
        cnts = [s for s, _ in edge_rays()]
    elif regime == "saturated":
        cnts = [p + 1 + SAT_TAIL for _, p in saturated_rays()]
    else:
        cnts = [5, 64, 130, 0, 5, 64, 130]
    rays, M = _table(cnts, g)
    N = len(cnts)
    offs = rays[:, 1].tolist()
    sigmas = torch.rand(M, generator=g) * 20
    if regime in ("benign", "one"):
        for r, c in enumerate(cnts):
            if c == 300:
                sigmas[offs[r]:offs[r] + 300] = torch.rand(300, generator=g) * 400
    elif regime == "empty":
        sigmas = torch.rand(M, generator=g) * 1e-3
        sigmas[torch.rand(M, generator=g) < 0.25] = 0.0
    elif regime == "edge":
        L = math.log(1.0 / (T_thresh if T_thresh > 0 else 1e-4))
        for r, (s, b) in enumerate(edge_rays()):
            sigmas[offs[r]:offs[r] + s] = L / (b - 0.5) / DT
        meta["first_dropped"] = [b if T_thresh > 0 else s for s, b in edge_rays()]
    elif regime == "saturated":
        meta["surface"] = []
        for r, (s, p) in enumerate(saturated_rays()):
            sigmas[offs[r]:offs[r] + cnts[r]] = 0.1 / DT
            if p:
                sigmas[offs[r]:offs[r] + p] = 2.0 / p / DT
            sigmas[offs[r] + p] = s
            meta["surface"].append(offs[r] + p)
    else:
        for r, c in enumerate(cnts):
            u = torch.rand(c, generator=g)
            sigmas[offs[r]:offs[r] + c] = u * 2e-3 / max(c, 1) / DT if r < 4 else (u + 0.5) * 600.0   # dense: tau in [1, 3]
    deltas = torch.stack([torch.full((M,), DT), torch.rand(M, generator=g) + 0.3], -1)
    rgbs = torch.randn(M, C, generator=g)
    bg = torch.rand(N + EXTRA, C, generator=g)
    if regime == "bigbg":
        bg = bg * 200 - 100
    grads = {"image": torch.randn(N + EXTRA, C, generator=g), "weights_sum": torch.randn(N + EXTRA, generator=g),
             "depth": torch.randn(N + EXTRA, generator=g)}
    return {"rays": rays, "sigmas": sigmas, "rgbs": rgbs, "deltas": deltas, "bg": bg, "grads": grads, "N": N, "M": M,
            "C": C, "meta": meta}


# which outputs receive a gradient: all three, and each one left out (tests/test_gpu_latent_tune.py)
GRAD_SELECTIONS = (("image", "weights_sum", "depth"), ("image", "depth"), ("image", "weights_sum"),
                   ("weights_sum", "depth"))
CASES = [(r, C, b, T) for r in REGIMES for C in (3, 4) for b in (True, False) for T in T_THRESHES]
_CACHE = {}


def composite_case(regime, C, with_bg, T_thresh):
    """Inputs, the float64 reference and, for every selection of GRAD_SELECTIONS, the float64 autograd gradients of
    sum(output * grads[output]) with respect to sigmas, rgbs and bg (rows by sample / by ray id, zeros where an input
    has no influence): computed once, shared, never modified.  The reference sees N + EXTRA ray ids."""
    key = (regime, C, with_bg, T_thresh)
    if key in _CACHE:
        return _CACHE[key]
    inp = composite_inputs(regime, C, T_thresh)
    sg = inp["sigmas"].double().requires_grad_()
    rgb = inp["rgbs"].double().requires_grad_()
    bg = inp["bg"][:inp["N"]].double().requires_grad_() if with_bg else None
    ref = composite_reference(sg, rgb, inp["deltas"].double(), inp["rays"], T_thresh, bg)
    leaves = [sg, rgb] + ([bg] if with_bg else [])
    names = ["sigmas", "rgbs"] + (["bg"] if with_bg else [])
    ref_grads = {}
    for sel in GRAD_SELECTIONS:
        got = torch.autograd.grad([ref[k] for k in sel], leaves, [inp["grads"][k][:inp["N"]].double() for k in sel],
                                  retain_graph=True, allow_unused=True)
        ref_grads[sel] = {n: (torch.zeros_like(l) if g is None else g) for n, g, l in zip(names, got, leaves)}
    out = {"inp": inp, "ref": {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ref.items()},
           "ref_grads": ref_grads}
    _CACHE[key] = out
    return out
