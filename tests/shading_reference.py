"""References of the shaded renders (csrc/shade.hip; contract in include/lnerf_hip.h, "shaded renders").

1. numpy f32 restatements of lnerf_fd_points, lnerf_shade_fd_forward and lnerf_shade_fd_backward in the stated op order:
   numpy rounds every + - * / sqrt to f32 and fuses nothing, as the library does (-ffp-contract=off), so the kernels are
   compared with these bit for bit.
2. shade_torch(): the same formulas in torch (any dtype) with autograd -- the f64 reference of the numpy backward.
3. render_shaded_oracle(): a shaded training frame composed from oracle.nerf_oracle's pieces (march, grid_encode,
   sigma_latent_mlp, composite_rays_train) with autograd, and render_shaded_oracle_infer(), its evaluation-loop form."""
import numpy as np
import torch

F = np.float32
FLOOR = F(1e-20)


# ------------------------------------------------------------------------------------------ numpy f32, bit for bit
def fd_points(xyzs, bound, eps, m):
    """xyzs f32 [>= m, 3] -> pts7 f32 [7 m, 3]: row 7 i = x_i, then +x, -x, +y, -y, +z, -z with the moved coordinate
    clamp(x_a +- eps, -bound, bound)."""
    x = np.asarray(xyzs, dtype=F)[:m]
    bound, eps = F(bound), F(eps)
    out = np.repeat(x[:, None, :], 7, axis=1).copy()
    for a in range(3):
        out[:, 1 + 2 * a, a] = np.minimum(np.maximum(x[:, a] + eps, -bound), bound)
        out[:, 2 + 2 * a, a] = np.minimum(np.maximum(x[:, a] - eps, -bound), bound)
    return out.reshape(7 * m, 3)


def _span_rows(rays):
    """(sample rows, ray id of each row) of every span of rays int32 [N,3] = (id, off, cnt), in ray order."""
    rows, ids = [], []
    for rid, off, cnt in np.asarray(rays).tolist():
        rows.append(np.arange(off, off + cnt, dtype=np.int64))
        ids.append(np.full(cnt, rid, dtype=np.int64))
    return (np.concatenate(rows), np.concatenate(ids)) if rows else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def _lambert(sg, light, ambient, inv_2eps):
    """sg f32 [m,7], light f32 [m,3], ambient f32 [m] -> n [m,3], s, r, d, lam (all f32, the kernel's op order)."""
    inv_2eps = F(inv_2eps)
    with np.errstate(all="ignore"):
        g = np.stack([(sg[:, 1 + 2 * a] - sg[:, 2 + 2 * a]) * inv_2eps for a in range(3)], -1)
        s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        r = F(1.0) / np.sqrt(np.fmax(s, FLOOR))                     # (fmax: a NaN s gives the floor, as fmaxf does)
        n = -(g * r[:, None])
        n = np.where(n != n, F(0.0), n).astype(F)
        d = (n[:, 0] * light[:, 0] + n[:, 1] * light[:, 1]) + n[:, 2] * light[:, 2]
        lam = ambient + (F(1.0) - ambient) * np.where(d > 0, d, F(0.0)).astype(F)
    return n, s, r, d, lam


def _views(ids, rays_per_view, B):
    return np.minimum(ids // int(rays_per_view), B - 1)


def shade_forward(sigmas7, rgbs7, rays, shade, rays_per_view, inv_2eps, sigma_c, colours):
    """Writes sigma_c [cap] and colours [cap, C] (f32 arrays, in place) for the rows inside the rays' spans."""
    rows, ids = _span_rows(rays)
    shade = np.asarray(shade, dtype=F)
    rec = shade[_views(ids, rays_per_view, shade.shape[0])]
    sg = np.asarray(sigmas7, dtype=F).reshape(-1, 7)[rows]
    alb = np.asarray(rgbs7, dtype=F).reshape(len(sigmas7) // 7, 7, -1)[rows, 0]
    _, _, _, _, lam = _lambert(sg, rec[:, :3], rec[:, 3], inv_2eps)
    tl = rec[:, 4] != 0
    sigma_c[rows] = sg[:, 0]
    colours[rows] = np.where(tl[:, None], lam[:, None], alb * lam[:, None]).astype(F)
    return sigma_c, colours


def shade_backward(sigmas7, rgbs7, rays, shade, rays_per_view, inv_2eps, dsigma_c, dcolours, dsigmas7, drgbs7):
    """Writes dsigmas7 [7 cap] and drgbs7 [7 cap, C] (f32 arrays, in place) for the rows inside the rays' spans."""
    rows, ids = _span_rows(rays)
    shade = np.asarray(shade, dtype=F)
    rec = shade[_views(ids, rays_per_view, shade.shape[0])]
    light, ambient, tl = rec[:, :3], rec[:, 3], rec[:, 4] != 0
    inv = F(inv_2eps)
    cap = len(sigmas7) // 7
    sg = np.asarray(sigmas7, dtype=F).reshape(cap, 7)[rows]
    alb = np.asarray(rgbs7, dtype=F).reshape(cap, 7, -1)[rows, 0]
    C = alb.shape[1]
    dcol = np.asarray(dcolours, dtype=F)[rows]
    n, s, r, d, lam = _lambert(sg, light, ambient, inv)
    with np.errstate(all="ignore"):
        dl_t, dl_l = dcol[:, 0].copy(), dcol[:, 0] * alb[:, 0]
        for c in range(1, C):
            dl_t = dl_t + dcol[:, c]
            dl_l = dl_l + dcol[:, c] * alb[:, c]
        dlam = np.where(tl, dl_t, dl_l).astype(F)
        dalb = np.where(tl[:, None], F(0.0), dcol * lam[:, None]).astype(F)
        k = (F(1.0) - ambient) * dlam
        dn = np.where((d > 0)[:, None], k[:, None] * light, F(0.0)).astype(F)
        q = (n[:, 0] * dn[:, 0] + n[:, 1] * dn[:, 1]) + n[:, 2] * dn[:, 2]
        t = np.where((s > FLOOR)[:, None], dn - n * q[:, None], dn).astype(F)
        dg = -(r[:, None] * t)
        v = dg * inv
    ds = np.empty((len(rows), 7), dtype=F)
    ds[:, 0] = np.asarray(dsigma_c, dtype=F)[rows]
    for a in range(3):
        ds[:, 1 + 2 * a] = v[:, a]
        ds[:, 2 + 2 * a] = -v[:, a]
    dsigmas7.reshape(cap, 7)[rows] = ds
    dr = np.zeros((len(rows), 7, C), dtype=F)
    dr[:, 0] = dalb
    drgbs7.reshape(cap, 7, C)[rows] = dr
    return dsigmas7, drgbs7


# ------------------------------------------------------------------------------------------ torch, with autograd
def shade_torch(sg, alb, light, ambient, textureless, inv_2eps):
    """sg [m,7], alb [m,C], light [m,3], ambient [m], textureless bool [m] -> (colours [m,C], s [m]); differentiable
    w.r.t. sg and alb in the tensors' dtype (f64 in the tests)."""
    g = torch.stack([(sg[:, 1 + 2 * a] - sg[:, 2 + 2 * a]) * inv_2eps for a in range(3)], -1)
    s = (g * g).sum(-1)
    r = 1.0 / torch.sqrt(torch.clamp(s, min=1e-20))
    n = -(g * r[:, None])
    n = torch.where(torch.isnan(n), torch.zeros_like(n), n)
    d = (n * light).sum(-1)
    lam = ambient + (1.0 - ambient) * torch.where(d > 0, d, torch.zeros_like(d))   # (no gradient at d = 0 exactly)
    col = torch.where(textureless[:, None], lam[:, None].expand(-1, alb.shape[1]), alb * lam[:, None])
    return col, s


def _pts7_torch(xyzs, bound, eps):
    """fd_points on a torch f32 tensor (the f32 arithmetic of the kernel: positions are inputs, not under test)."""
    return torch.from_numpy(fd_points(xyzs.detach().cpu().numpy(), bound, eps, xyzs.shape[0]))


def _field64(O, pts, table, params, lv, bound, blob_scale, blob_std):
    feat = O.grid_encode((pts + bound) / (2.0 * bound), table, lv)
    return O.sigma_latent_mlp(feat, pts, params, blob_scale, blob_std)


def render_shaded_oracle(O, rays_o, rays_d, table, params, lv, bitfield, *, light, ambient, textureless, eps=1e-2,
                         bound=1.0, cascade=1, G=128, min_near=0.1, max_steps=1024, bg_color=None, T_thresh=1e-4,
                         blob_scale=5.0, blob_std=0.2, density_scale=1.0, shaded=True):
    """One view's shaded training frame from the oracle's pieces, differentiable w.r.t. `table` and `params`.  Pass f64
    leaves for an f64 field and shade; the march and the compositing are the oracle's own, which exist in f32 only (the
    per-sample densities and colours are rounded to f32 in front of composite_rays_train; bg_color f32).  light: [3] toward the light (normalised here).
    shaded=False: the plain albedo frame through the same code (the yardstick of the gradient bound).
    -> dict(image, depth, weights_sum, rays, s (the per-sample |g|^2), albedo, colours, M)."""
    aabb = [-bound] * 3 + [bound] * 3
    with torch.no_grad():
        nears, fars = O.near_far_from_aabb(rays_o, rays_d, aabb, min_near)
        xyzs, dirs, deltas, rays, M = O.march_rays_train(rays_o, rays_d, nears, fars, bitfield, bound, cascade, G,
                                                         max_steps, 0.0, None)
    dt = table.dtype
    if not shaded:
        sig, alb = _field64(O, xyzs.to(dt), table, params, lv, bound, blob_scale, blob_std)
        ws, depth, image = O.composite_rays_train((density_scale * sig).float(), alb.float(), deltas, rays, T_thresh,
                                                  bg_color)
        return {"image": image, "depth": depth, "weights_sum": ws, "rays": rays, "M": M, "albedo": alb}
    pts7 = _pts7_torch(xyzs, bound, eps).to(dt)
    sig7, rgb7 = _field64(O, pts7, table, params, lv, bound, blob_scale, blob_std)
    sg, alb = sig7.reshape(M, 7), rgb7.reshape(M, 7, rgb7.shape[1])[:, 0]
    l = torch.as_tensor(light, dtype=dt).reshape(3)
    l = (l / l.norm()).expand(M, 3)
    col, s = shade_torch(sg, alb, l, torch.full((M,), float(ambient), dtype=dt),
                         torch.full((M,), bool(textureless)), 1.0 / (2.0 * eps))
    ws, depth, image = O.composite_rays_train((density_scale * sg[:, 0]).float(), col.float(), deltas, rays, T_thresh,
                                              bg_color)
    return {"image": image, "depth": depth, "weights_sum": ws, "rays": rays, "M": M, "s": s.detach(), "albedo": alb.detach(),
            "colours": col.detach()}


def render_shaded_oracle_infer(O, rays_o, rays_d, table, params, lv, bitfield, *, light, ambient, textureless, eps=1e-2,
                               bound=1.0, G=128, max_steps=1024, bg_color=None, **kw):
    """The evaluation loop (oracle.render_frame_infer, the renderer's chunk schedule) with the shaded field."""
    dt = table.dtype
    l1 = torch.as_tensor(light, dtype=dt).reshape(3)
    l1 = l1 / l1.norm()
    albedo_max = [0.0]

    def field(x):
        m = x.shape[0]
        pts7 = _pts7_torch(x, bound, eps).to(dt)
        sig7, rgb7 = _field64(O, pts7, table, params, lv, bound, kw.get("blob_scale", 5.0), kw.get("blob_std", 0.2))
        sg, alb = sig7.reshape(m, 7), rgb7.reshape(m, 7, rgb7.shape[1])[:, 0]
        col, _ = shade_torch(sg, alb, l1.expand(m, 3), torch.full((m,), float(ambient), dtype=dt),
                             torch.full((m,), bool(textureless)), 1.0 / (2.0 * eps))
        if m:
            albedo_max[0] = max(albedo_max[0], float(alb.abs().max()))
        return sg[:, 0], col

    out = O.render_frame_infer(rays_o, rays_d, field, bitfield=bitfield, bound=bound, G=G, max_steps=max_steps,
                               bg_color=bg_color, schedule=lambda N, n, s: O.renderer_schedule(N, n, s, max_steps),
                               **{k: v for k, v in kw.items() if k not in ("blob_scale", "blob_std")})
    out["albedo_max"] = albedo_max[0]
    return out


# ------------------------------------------------------------------------------------------ the tiny scene of the tests
SCENE = dict(G=16, HW=8, LOG2_T=12, MAX_STEPS=32, EPS=1e-2, AMBIENT=0.1, LIGHT=(0.3, 0.8, 0.5))
W_NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")


def scene_net(O, precision, seed=6):
    """The tiny model of tests/test_gpu_shading.py on the CPU (move it with .to(device)) and its occupancy bitfield: grid
    16, table 2^12 rows per level, normal(0, 0.1) entries, a solid ball of radius 0.5; the density blob is on."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    G, HW = SCENE["G"], SCENE["HW"]
    torch.manual_seed(seed)
    cfg = RenderConfig(grid_size=G, train_h=HW, train_w=HW, mlp_precision=precision, table_dtype=precision,
                       gridtype="blocked" if precision == "bf16" else "hash")
    net = NeRFNetwork(cfg, log2_hashmap_size=SCENE["LOG2_T"])
    net.encoder.embeddings.data.normal_(0, 0.1)
    grid = O.density_grid_from_function(lambda p: (p.norm(dim=-1) < 0.5).float() * 10.0, G, 1, 1.0)
    bits = O.packbits(grid.reshape(-1), 0.01)
    net.density_grid.copy_(grid)
    net.density_bitfield.copy_(bits)
    return net, bits


def scene_rays(O):
    """(rays_o [N,3], rays_d [N,3], background [N,4], upstream image gradient [1,N,4]) of the scene's one view."""
    import math
    HW = SCENE["HW"]
    f = HW / (2 * math.tan(math.radians(55) / 2))
    ro, rd = O.get_rays(O.pose_from_angles(math.radians(60), 0.3, 1.25), f, f, HW / 2, HW / 2, HW, HW)
    gen = torch.Generator().manual_seed(8)
    bg = torch.rand(HW * HW, 4, generator=gen)
    g = torch.randn(1, HW * HW, 4, generator=gen)
    return ro[0].contiguous(), rd[0].contiguous(), bg, g


def scene_oracle_leaves(O, net):
    lv = O.make_grid_levels(16, 2, 16, 2048, SCENE["LOG2_T"])
    assert lv.offsets == net.encoder.levels.offsets
    table = net.encoder.embeddings.detach().cpu().clone()
    params = {k: getattr(net, k).detach().cpu().clone() for k in W_NAMES}
    return lv, table, params
