"""float64 reference of the RGB refinement stage's compositing (render.nerf_type = latent_tune), shared by
tests/test_latent_tune_cpu.py and tests/test_gpu_latent_tune.py.

oracle.nerf_oracle.composite_rays_train is the project's statement of the compositing, but it accumulates in float32
whatever it is given.  `weights64` restates its per-sample weights (same formulas, same padded layout) in the dtype of
its inputs and with autograd; the CPU suite checks the restatement against the oracle itself on float32 inputs, so the
float64 numbers used here are the oracle's compositing weights to float32 rounding."""
import torch


def weights64(sigmas, deltas, rays, T_thresh=1e-4):
    """sigmas [M], deltas [M,2] = (dt, t), rays int [N,3] = (id, offset, count)  ->  (w [N,K], idx [N,K], valid [N,K],
    keep [N,K], margin): per-sample weights w = alpha T of oracle.nerf_oracle.composite_rays_train (0 on padding and
    behind the early stop T < T_thresh), the sample index of every slot, and the smallest relative distance of any
    valid sample's T from T_thresh (the kill decisions of an f32 kernel can only be compared when that is large)."""
    offs = rays[:, 1].to(torch.int64)
    cnts = rays[:, 2].to(torch.int64)
    K = max(int(cnts.max().item()), 1)
    k = torch.arange(K)
    valid = k[None, :] < cnts[:, None]
    idx = (offs[:, None] + k[None, :]).clamp(max=max(sigmas.shape[0] - 1, 0))
    idx = torch.where(valid, idx, torch.zeros_like(idx))
    zero = torch.zeros(1, dtype=sigmas.dtype)
    sg = torch.where(valid, sigmas[idx], zero)
    dt = torch.where(valid, deltas[idx, 0], zero)
    tau = sg * dt
    # exclusive prefix = the inclusive sum shifted by one slot (never `cumsum - tau`: a large tau would round the
    # small prefix in front of it away, and tau = inf would give inf - inf)
    csum = torch.cat([torch.zeros_like(tau[:, :1]), torch.cumsum(tau, 1)[:, :-1]], 1)
    T = torch.exp(-csum)
    alpha = 1.0 - torch.exp(-tau)
    keep = valid & (T >= T_thresh)
    w = torch.where(keep, alpha * T, zero)
    rel = ((T.detach() - T_thresh).abs() / T_thresh)[valid]
    margin = float(rel.min()) if rel.numel() else float("inf")
    return w, idx, valid, keep, margin


def _by_id(ids, values):
    return torch.zeros_like(values).index_add(0, ids, values)


def composite_decode_ref(sigmas, latents, deltas, rays, decoder, bg=None, T_thresh=1e-4):
    """The DEFINITION of the stage, per sample:  c_k = (D z_k + 1) / 2 (no clamp),  image = sum_k w_k c_k + (1 - ws) bg.
    -> dict(weights_sum [N], depth [N], latent_image [N,4] = sum_k w_k z_k, image [N,3], cmax [N] = max_k |c_k|_inf over
    the ray's samples (0 for an empty span), count [N], keep_samples [M] bool, margin), rows indexed by ray id, in the
    dtype of the inputs, differentiable in sigmas, latents, decoder and bg."""
    ids = rays[:, 0].to(torch.int64)
    w, idx, valid, keep, margin = weights64(sigmas, deltas, rays, T_thresh)
    zero = torch.zeros(1, dtype=sigmas.dtype)
    tt = torch.where(valid, deltas[idx, 1], zero)
    z = torch.where(valid[..., None], latents[idx], zero)                       # [N,K,4]
    c = (z @ decoder.T + 1.0) / 2.0                                             # [N,K,3]
    ws = w.sum(1)
    image = (w[..., None] * c).sum(1)
    if bg is not None:
        image = image + (1.0 - ws)[:, None] * bg[ids]
    cmax = torch.where(valid, c.detach().abs().amax(-1), zero).amax(1)
    keep_samples = torch.zeros(sigmas.shape[0], dtype=torch.bool)
    keep_samples[idx[keep]] = True
    return {"weights_sum": _by_id(ids, ws), "depth": _by_id(ids, (w * tt).sum(1)),
            "latent_image": _by_id(ids, (w[..., None] * z).sum(1)), "image": _by_id(ids, image),
            "cmax": _by_id(ids, cmax), "count": _by_id(ids, rays[:, 2].to(torch.int64)), "keep_samples": keep_samples,
            "margin": margin}
