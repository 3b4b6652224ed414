"""NeRFRenderer: the `render()/run_cuda()/run()` surface the north star names (SURVEY.md §8 row
H0, boundary §8(b)).  The reference imports it through src.latent_nerf (scripts/train_latent_nerf.py:3-4)
but does not ship it; what it does pin is the hand-off around it: the renderer returns a dict with
'image' that the trainer reshapes to [B,C,H,W] latents (src/latent_paint/models/textured_mesh.py:181-220,
src/stable_diffusion.py:259) and receives the SDS gradient via `pred.backward(gradient=grad)`
(src/latent_paint_mesh/training/trainer.py:657-658).

Everything below runs on the HIP library; there is no PyTorch/CPU fallback path."""
import math
import os

import torch
import torch.nn as nn

from ..raymarching import backend as _b
from ..raymarching import raymarching as rm
from ..raymarching.raymarching import _p, _stream


def _sample_pdf(bins, weights, n_samples, stratified):
    """Inverse-transform sampling of `n_samples` positions per ray from the piecewise-constant density that `weights`
    [N, B-1] puts on the intervals between `bins` [N, B] (hierarchical sampling of NeRF)."""
    w = weights + 1e-5
    cdf = torch.cumsum(w / w.sum(-1, keepdim=True), -1)
    cdf = torch.cat([torch.zeros_like(cdf[:, :1]), cdf], -1)                     # [N, B]
    if stratified:
        u = torch.linspace(0.5 / n_samples, 1.0 - 0.5 / n_samples, n_samples, device=bins.device)
        u = u[None].expand(bins.shape[0], n_samples).contiguous()
    else:
        u = torch.rand(bins.shape[0], n_samples, device=bins.device)
    hi = torch.searchsorted(cdf, u, right=True).clamp(max=cdf.shape[-1] - 1)
    lo = (hi - 1).clamp(min=0)
    c0, c1 = torch.gather(cdf, 1, lo), torch.gather(cdf, 1, hi)
    b0, b1 = torch.gather(bins, 1, lo), torch.gather(bins, 1, hi)
    span = c1 - c0
    t = (u - c0) / torch.where(span < 1e-5, torch.ones_like(span), span)
    return b0 + t * (b1 - b0)


class PreparedRays:
    """Output of NeRFRenderer.prepare_rays(): the marched samples of one view (a MarchResult in one of the renderer's
    two sample-buffer sets), its background colours, the ray-batch shape and the ray directions [N,3] the march read (in
    the camera form: the buffer it generated them into), which the orientation term of a shaded render reads."""
    __slots__ = ("march", "bg", "prefix", "N", "cap", "rays_d")

    def __init__(self, march, bg, prefix, N, cap, rays_d=None):
        self.march, self.bg, self.prefix, self.N, self.cap, self.rays_d = march, bg, prefix, N, cap, rays_d


class _ShadowExtraState:
    NAMES = ("density_grid", "density_bitfield", "mean_density_dev")

    def __init__(self, renderer):
        self.r = renderer

    def __enter__(self):
        r = self.r
        if r._shadow_state is None or r._shadow_state[0].device != r.density_grid.device:
            r._shadow_state = [getattr(r, n).clone() for n in self.NAMES]
        self.real = [r._buffers[n] for n in self.NAMES]
        for n, t in zip(self.NAMES, r._shadow_state):
            r._buffers[n] = t
        return r

    def __exit__(self, *exc):
        for n, t in zip(self.NAMES, self.real):
            self.r._buffers[n] = t
        return False


class NeRFRenderer(nn.Module):
    def __init__(self, cfg, latent_mode: bool = True):
        super().__init__()
        self.cfg = cfg
        self.latent_mode = latent_mode
        self.tuned = False            # NeRFNetwork: render.nerf_type = latent_tune (4 latents per sample + a decoder)
        self.bound = float(cfg.bound)
        self.cascade = 1 + math.ceil(math.log2(cfg.bound)) if cfg.bound > 1 else 1
        self.grid_size = int(cfg.grid_size)
        self.density_scale = 1.0
        self.min_near = cfg.min_near
        self.density_thresh = cfg.density_thresh
        self.bg_radius = cfg.bg_radius
        self.cuda_ray = cfg.cuda_ray
        aabb = torch.tensor([-self.bound] * 3 + [self.bound] * 3, dtype=torch.float32)
        self.register_buffer("aabb_train", aabb)
        self.register_buffer("aabb_infer", aabb.clone())
        G3 = self.grid_size ** 3
        self.register_buffer("density_grid", torch.zeros(self.cascade, G3))
        self.register_buffer("density_bitfield", torch.zeros(self.cascade * G3 // 8, dtype=torch.uint8))
        self.register_buffer("mean_density_dev", torch.zeros(1))
        self.mean_density = 0.0
        self.iter_density = 0
        self.local_step = 0
        self._march = None            # the most recent training march
        self._march_slots = [None, None]  # two sample-buffer sets: prepare_rays(slot=...) alternates them when pipelined
        self._ray_slots = [None, None]    # ray buffers of the camera form of prepare_rays
        self._march_key = None
        self._budget = None       # ((N, max_steps), capacity) derived from observed marches
        self.mean_count = 0
        self._noise_counter = None
        self._occ_scratch = None
        self._occ_cells = None
        self._occ_gen = None
        self._occ_seed = 0x0CC0
        self._occ_sample_ws = None
        self._bg_const = {}
        self._shadow_state = None

    # subclasses provide the field -------------------------------------------------------
    def forward(self, x, d=None):
        raise NotImplementedError()

    def density(self, x):
        raise NotImplementedError()

    def field(self, xyzs, m_host, m_dev=None, level_stride=None):
        raise NotImplementedError()

    def background(self, d):
        raise NotImplementedError()

    def normal(self, x):
        raise NotImplementedError()

    def decode_points(self, latents):
        raise NotImplementedError()

    def density_normals(self, xyzs):
        """xyzs [M,3] -> (sigmas [M] (x density_scale), unit normals [M,3]), outside autograd."""
        raise NotImplementedError()

    SHADED = ("lambertian", "textureless")

    def _check_shading(self, shading, light_d=None, sampler="run_cuda", orient=False, normal_image=False):
        """Validates `shading` (and `orient`, `normal_image`) before any tensor is touched.  -> (normal render?, shaded
        render?)."""
        if normal_image and (shading not in self.SHADED or not self.training or sampler != "run_cuda" or self.tuned):
            # the image composites the finite-difference normal of a shaded TRAINING render on the march's spans
            raise ValueError("normal_image=True needs shading='lambertian' / 'textureless' in training mode on the "
                             "occupancy-marched renderer, not latent_tune (got shading=%r, %s mode, %s%s)"
                             % (shading, "training" if self.training else "evaluation", sampler,
                                ", latent_tune" if self.tuned else ""))
        if orient and (shading not in self.SHADED or not self.training or sampler != "run_cuda"):
            # the term reads the finite-difference normal of a shaded TRAINING render and the march's spans
            raise ValueError("orient=True needs shading='lambertian' / 'textureless' in training mode on the "
                             "occupancy-marched renderer (got shading=%r, %s mode, %s)"
                             % (shading, "training" if self.training else "evaluation", sampler))
        if shading in self.SHADED:
            if light_d is None:
                # there is no random light inside the renderer: a render is a function of its arguments
                raise ValueError("shading must be 'albedo' or 'normal' unless light_d is given: shading=%r needs "
                                 "light_d=[3] / [B,3] (direction toward the light)" % (shading,))
            if sampler != "run_cuda":
                raise ValueError("shading=%r is built for the occupancy-marched renderer (cuda_ray = true); the uniform "
                                 "sampler renders 'albedo' and 'normal'" % (shading,))
            if self.tuned:
                raise ValueError("shading=%r is not available with render.nerf_type = latent_tune (the decoded colours "
                                 "are composited per ray)" % (shading,))
            return False, True
        if shading not in ("albedo", "normal"):
            raise ValueError("shading must be 'albedo', 'normal', or 'lambertian' / 'textureless' with light_d "
                             "(got %r)" % (shading,))
        if shading == "normal" and self.training:
            # the analytic normal inside the training graph would need the encoder's second-order backward, which is
            # not built (training renders shade with the finite-difference normal instead: 'lambertian' /
            # 'textureless'): refuse rather than hand back an image whose gradient is wrong
            raise ValueError("shading='normal' is an evaluation render: call .eval() first (normals are not "
                             "differentiable here)")
        return shading == "normal", False

    def _check_distortion(self, distortion, sampler="run_cuda"):
        """Validates `distortion` before any tensor is touched."""
        if distortion and (not self.training or sampler != "run_cuda"):
            # the term is a training loss on the march's spans (deltas = (dt, t) with the occupancy skips)
            raise ValueError("distortion=True needs training mode on the occupancy-marched renderer (got %s mode, %s)"
                             % ("training" if self.training else "evaluation", sampler))

    def _check_fd_stride(self, cap):
        """The shaded render evaluates the field at 7 points per sample in ONE node: its level stride is 7 * cap."""
        if getattr(self, "precision", "f32") == "bf16" and 7 * int(cap) > (1 << 24):
            raise ValueError("a shaded bf16 render evaluates the field at 7 x %d samples, past the bf16 kernels' level "
                             "stride limit of 2^24: set render.max_samples <= %d" % (int(cap), (1 << 24) // 7))

    def reset_extra_state(self):
        self.density_grid.zero_()
        self.density_bitfield.zero_()
        self.mean_density_dev.zero_()
        self.mean_density = 0.0
        self.iter_density = 0
        self.local_step = 0

    # ------------------------------------------------------------------------------------
    def _bg_tensor(self, bg_color, rays_d, N, C):
        if self.bg_radius > 0:
            return self.background(rays_d)
        if bg_color is None:
            bg_color = 1.0
        if not torch.is_tensor(bg_color):
            # a constant background is read-only for every consumer: one cached tensor per (N, C, value) instead of a
            # fill dispatch per render (a dependent ~5 us launch in a replayed step)
            key = (N, C, float(bg_color), str(rays_d.device))
            cached = self._bg_const.get(key)
            if cached is None:
                if len(self._bg_const) > 8:
                    self._bg_const.clear()
                cached = torch.full((N, C), float(bg_color), device=rays_d.device, dtype=torch.float32)
                self._bg_const[key] = cached
            return cached
        bg = bg_color.to(rays_d.device, torch.float32)
        if bg.dim() == 1:
            bg = bg[None].expand(N, C)
        return bg.reshape(N, C).contiguous()

    def _capacity(self, N, max_steps):
        """Sample-buffer capacity of a training march of N rays.  `cfg.max_samples` if set; else the worst case
        N * min(max_steps, 256) until update_sample_budget() has seen real marches of this shape, then the budget it
        derived from them (every capacity-sized buffer, the scatter workspace included, shrinks with it)."""
        worst = max(N * min(int(max_steps), 256), 64)
        if self.cfg.max_samples > 0:
            return int(self.cfg.max_samples)
        if self._budget is not None and self._budget[0] == (N, int(max_steps)):
            return min(worst, self._budget[1])
        return worst

    def update_sample_budget(self):
        """Called where the training loop synchronises anyway (the occupancy refresh, every `update_extra_interval`
        steps): reads the march statistics back ONCE -- the largest sample count M and the largest dropped-ray count of
        any training march since the previous call (running maxima kept on the device by prepare_rays) -- and re-derives the
        capacity for marches of that shape: 1.5 x M rounded up to 64 Ki samples.  It changes only when the peak came
        within 80 % of the current capacity (or rays were dropped: back to the worst case) or fell below 40 % of it.
        The upstream renderer sizes its buffers from a running `mean_count` the same way, but reads the counter
        back every step."""
        m = self._march
        if m is None or self.cfg.max_samples > 0:
            return None
        # window maxima, not the last march: the march itself keeps them in word 3 of its counter (no launch per step)
        peak, dropped = 0, 0
        for slot in {id(s): s for s in self._march_slots + [m] if s is not None}.values():
            pk, dr = slot.take_peak()
            peak, dropped = max(peak, pk), dropped + int(dr)
        key, cap = self._march_key, m.capacity
        self.mean_count = peak if self.mean_count == 0 else int(0.9 * self.mean_count + 0.1 * peak)
        want = -(-max(int(1.5 * peak), 1) // 65536) * 65536
        if dropped > 0:
            self._budget = None                      # back to the worst case for the next marches
        elif 5 * peak > 4 * cap or 5 * peak < 2 * cap or self._budget is None or self._budget[0] != key:
            self._budget = (key, want)
        return self._budget

    def _noise_state(self, dev):
        """(seed, device counter) of the march's counter-based jitter generator (cfg.noise_seed; None = torch.rand)."""
        seed = getattr(self.cfg, "noise_seed", None)
        if seed is None:
            return None
        if self._noise_counter is None or self._noise_counter.device != dev:
            self._noise_counter = torch.zeros(1, device=dev, dtype=torch.int32)
        return (int(seed), self._noise_counter)

    def _aabb_values(self):
        aabb = self.aabb_train if self.training else self.aabb_infer
        a = [-self.bound] * 3 + [self.bound] * 3 if aabb is None else aabb
        if torch.is_tensor(a) and a.is_cuda:
            a = self._aabb_host(a)
        return a

    def _near_far(self, rays_o, rays_d):
        return rm.near_far_from_aabb(rays_o, rays_d, self._aabb_values(), self.min_near)

    def prepare_rays(self, rays_o, rays_d, dt_gamma=0.0, bg_color=None, perturb=False, max_steps=1024, slot=0,
                     camera=None, **kwargs):
        """The part of a TRAINING render that depends only on the rays and the occupancy bitfield -- AABB clip,
        background, occupancy-pruned march -- done ahead of time into sample-buffer set `slot` (0 or 1).  Returns
        a PreparedRays that `render(..., prepared=p)` / `run_cuda(..., prepared=p)` shades.  A training loop that
        knows its next view calls this for view k+1 on a side stream while view k is shaded and back-propagated
        (Trainer / bench.py: the two sets alternate); nothing in it reads the hash table or the MLP, so the result is
        the one the un-pipelined order gives as long as the bitfield is not refreshed in between (after
        update_extra_state() prepare again)."""
        if not self.training:
            raise RuntimeError("prepare_rays is the training-mode march; inference marches adaptively inside run_cuda")
        if camera is not None:
            # camera = (poses [B,4,4], (fx, fy, cx, cy), H, W) instead of rays: they are generated inside the march's
            # count pass (one dispatch less than get_rays + render) into buffers of this sample-buffer set
            poses, _intr, him, wim = camera
            B = 1 if poses.dim() == 2 else poses.shape[0]
            camera = (poses.view(B, 4, 4).float(), _intr, int(him), int(wim))
            key = (B * him * wim, str(poses.device))
            bufs = self._ray_slots[slot]
            if bufs is None or bufs[0] != key:
                bufs = (key, torch.empty(B * him * wim, 3, device=poses.device), torch.empty(B * him * wim, 3, device=poses.device))
                self._ray_slots[slot] = bufs
            else:   # rewritten through raw pointers: a stale backward that saved them (background net) must fail loudly
                torch.autograd.graph.increment_version(bufs[1])
                torch.autograd.graph.increment_version(bufs[2])
            rays_o, rays_d = bufs[1], bufs[2]
            prefix = (B, him * wim)
        else:
            prefix = rays_o.shape[:-1]
            rays_o = rays_o.contiguous().view(-1, 3).float()
            rays_d = rays_d.contiguous().view(-1, 3).float()
        N = rays_o.shape[0]
        if camera is None or self.bg_radius <= 0:
            bg = self._bg_tensor(bg_color, rays_d, N, self.img_dims)
        cap = self._capacity(N, max_steps)
        a = self._aabb_values()
        a = [float(v) for v in (a.tolist() if torch.is_tensor(a) else a)]
        # (the AABB clip runs inside the march passes: near_far_from_aabb's arithmetic, one dispatch less)
        march = rm.march_rays_train(rays_o, rays_d, self.bound, self.density_bitfield, self.cascade,
                                    self.grid_size, None, None, perturb=perturb, dt_gamma=dt_gamma,
                                    max_steps=max_steps, capacity=cap, out=self._march_slots[slot],
                                    noises=kwargs.get("noises"), noise_state=self._noise_state(rays_o.device),
                                    aabb=a, min_near=self.min_near, camera=camera)
        if camera is not None and self.bg_radius > 0:
            bg = self._bg_tensor(bg_color, rays_d, N, self.img_dims)   # the background net reads the generated directions
        self._march_slots[slot] = march
        self._march = march
        self._march_key = (N, int(max_steps))
        return PreparedRays(march, bg, prefix, N, cap, rays_d)

    def run_cuda(self, rays_o, rays_d, dt_gamma=0.0, bg_color=None, perturb=False, force_all_rays=False,
                 max_steps=1024, T_thresh=1e-4, prepared=None, shading="albedo", light_d=None, ambient_ratio=0.1,
                 normal_eps=1e-2, orient=False, distortion=False, normal_image=False, **kwargs):
        """rays_o, rays_d [B,N,3] -> dict(image [B,N,C], depth [B,N], weights_sum [B,N]).
        Training mode: march -> hash gather -> MLP -> composite, all on device, no host sync (latent_tune: the fused
        composite + decode, image in RGB);
        additionally returns the capacity-sized 'xyzs'/'sigmas' with the device counter 'counter'.
        prepared: a PreparedRays of prepare_rays() (rays_o / rays_d are then ignored and may be None).
        shading="normal" (evaluation only): the per-sample colours are (n + 1) / 2 of the field's surface normal n --
        3 channels whatever img_dims is -- and no background is added; the densities, hence the march, depth and
        weights_sum, are those of the albedo render.
        shading="lambertian" / "textureless" with light_d (training and evaluation): the per-sample colours are albedo x
        lam, or lam alone, lam = ambient_ratio + (1 - ambient_ratio) max(n . l, 0), n the FINITE-DIFFERENCE normal of the
        density at distance normal_eps (the upstream renderer's training normal: six more field queries per sample, whose
        gradient is the field's ordinary backward at 7 M points).  light_d: [3] or [B,3], the direction toward the light
        of each of the B views (normalised here) -- or a ready device record [B,5] = (unit l, ambient, textureless 0 / 1)
        (raymarching.shade_record), taken as it is: the kind and the ambient share are then the record's.
        orient=True (shaded training renders only): additionally 'loss_orient' [B,N], per ray sum_i w_i max(0, n_i . v)^2
        with the compositing weights w (detached) and the unit ray direction v -- the orientation regulariser, computed and
        differentiated inside the shade kernels (raymarching.shade_fd(orient=...)); image, depth and weights_sum keep
        their bits.
        distortion=True (training renders of every kind): additionally 'loss_distortion' [B,N], per ray the distortion
        loss of mip-NeRF 360, sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i on the march's samples, with the
        compositing weights w NOT detached (raymarching.distortion_loss on the very sigmas the compositing gets); image,
        depth and weights_sum keep their bits.
        normal_image=True (shaded training renders only): additionally 'normal_image' [B,N,3], per ray sum_i w_i n_i, the
        finite-difference normals of the samples under the compositing weights (NOT detached) -- raymarching.normal_image
        on the very sigmas7 the shade node gets; differentiable, the input of the 2D normal-smoothness term
        (raymarching.image_smooth).  image, depth, weights_sum, loss_orient and loss_distortion keep their bits."""
        self._check_distortion(distortion)
        shade_normal, shaded = self._check_shading(shading, light_d, orient=orient, normal_image=normal_image)
        C = 3 if shade_normal else self.img_dims
        decode = self.tuned and not shade_normal   # composite 4 latent channels, decode per ray (bg_color is RGB)
        results = {}
        if shaded and self.training:
            # the capacity is known before any tensor is read: refuse the stride the bf16 kernels cannot address here
            if prepared is not None:
                self._check_fd_stride(prepared.cap)
            else:
                cam = kwargs.get("camera")
                n_rays = (int(cam[0].numel() // 16) * int(cam[2]) * int(cam[3]) if cam is not None
                          else int(rays_o.numel() // 3))
                self._check_fd_stride(self._capacity(n_rays, max_steps))
        if self.training:
            if prepared is None:
                prepared = self.prepare_rays(rays_o, rays_d, dt_gamma=dt_gamma, bg_color=bg_color, perturb=perturb,
                                             max_steps=max_steps, **kwargs)   # (kwargs may carry camera=...)
            march, bg, prefix, N, cap = prepared.march, prepared.bg, prepared.prefix, prepared.N, prepared.cap
            self.local_step += 1
            m_dev = march.counter[0:1]
            if shaded:
                # stencil -> ONE field node over the 7 cap rows (every backward route applies as it stands) -> shade
                n_views = prefix[0] if len(prefix) == 2 else 1
                shade = rm.shade_record(light_d, ambient_ratio, shading == "textureless", n_views, march.xyzs.device)
                pts7, m7_dev = rm.fd_points(march.xyzs, self.bound, normal_eps, cap, m_dev)
                sigmas7, rgbs7 = self.field(pts7, 7 * cap, m7_dev, 7 * cap)
                if orient:
                    if prepared.rays_d is None:
                        raise ValueError("orient=True needs a PreparedRays of prepare_rays() (it carries the ray directions)")
                    sigmas, rgbs, loss_orient = rm.shade_fd(
                        sigmas7, rgbs7, march.rays, shade, max(N // n_views, 1), normal_eps,
                        orient=(march.deltas, prepared.rays_d, self.density_scale, T_thresh, N))
                    results["loss_orient"] = loss_orient.view(*prefix)
                else:
                    sigmas, rgbs = rm.shade_fd(sigmas7, rgbs7, march.rays, shade, max(N // n_views, 1), normal_eps)
                if normal_image:
                    results["normal_image"] = rm.normal_image(sigmas7, march.deltas, march.rays, N, normal_eps,
                                                              self.density_scale, T_thresh).view(*prefix, 3)
            else:
                sigmas, rgbs = self.field(march.xyzs, cap, m_dev, cap)
            sigmas = self.density_scale * sigmas if self.density_scale != 1.0 else sigmas
            if distortion:
                results["loss_distortion"] = rm.distortion_loss(sigmas, march.deltas, march.rays, T_thresh, N).view(*prefix)
            if decode:
                weights_sum, depth, image, _ = rm.composite_rays_train_decode(sigmas, rgbs, march.deltas, march.rays,
                                                                             self.decoder, T_thresh, bg)
            else:
                weights_sum, depth, image = rm.composite_rays_train(sigmas, rgbs, march.deltas, march.rays, T_thresh, bg)
            results.update(xyzs=march.xyzs, sigmas=sigmas, counter=march.counter, rays=march.rays,
                           deltas=march.deltas)
        else:
            prefix = rays_o.shape[:-1]
            rays_o = rays_o.contiguous().view(-1, 3).float()
            rays_d = rays_d.contiguous().view(-1, 3).float()
            N = rays_o.shape[0]
            nears, fars = self._near_far(rays_o, rays_d)
            bg = None if shade_normal else self._bg_tensor(bg_color, rays_d, N, C)
            dev = rays_o.device
            weights_sum = torch.zeros(N, device=dev)
            depth = torch.zeros(N, device=dev)
            image = torch.zeros(N, 4 if decode else C, device=dev)
            trans = torch.ones(N, device=dev)
            rays_alive = torch.arange(N, dtype=torch.int32, device=dev)
            spare = torch.empty_like(rays_alive)
            n_dev = torch.empty(1, dtype=torch.int32, device=dev)
            rays_t = nears.clone()
            if shaded:
                n_views = prefix[0] if len(prefix) == 2 else 1
                shade = rm.shade_record(light_d, ambient_ratio, shading == "textureless", n_views, dev)
            n_alive, step = N, 0
            while step < max_steps and n_alive > 0:
                # the last chunk stops at max_steps: a live ray never takes more samples than the training march
                n_step = min(max(min(N // n_alive, 8), 1), max_steps - step)
                xyzs, dirs, deltas = rm.march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, self.bound,
                                                   self.density_bitfield, self.cascade, self.grid_size, fars,
                                                   dt_gamma, max_steps)
                if shade_normal:
                    sigmas, rgbs = self.density_normals(xyzs)       # (sigmas: scaled already)
                    rgbs = (rgbs + 1.0) / 2.0
                elif shaded:
                    # the training definition per chunk: ray j of the chunk owns samples j n_step .. (j + 1) n_step - 1
                    with torch.no_grad():
                        pts7, _ = rm.fd_points(xyzs, self.bound, normal_eps, xyzs.shape[0])
                        sigmas7, rgbs7 = self.field(pts7, pts7.shape[0])
                        j = torch.arange(n_alive, dtype=torch.int32, device=dev)
                        table = torch.stack([rays_alive[:n_alive], j * n_step, torch.full_like(j, n_step)], -1).contiguous()
                        sigmas, rgbs = rm.shade_fd(sigmas7, rgbs7, table, shade, max(N // n_views, 1), normal_eps)
                    sigmas = self.density_scale * sigmas if self.density_scale != 1.0 else sigmas
                else:
                    with torch.no_grad():
                        sigmas, rgbs = self.field(xyzs, xyzs.shape[0])
                    sigmas = self.density_scale * sigmas if self.density_scale != 1.0 else sigmas
                rm.composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image,
                                  trans, T_thresh)
                spare, n_dev = rm.compact_rays(rays_alive, n_alive, spare, n_dev)
                rays_alive, spare = spare, rays_alive
                n_alive = int(n_dev.item())  # live-ray count decides the next launch shape
                step += n_step
            if decode:
                image = rm.decode_image(image, weights_sum, self.decoder, bg)
            elif not shade_normal:
                image = image + (1.0 - weights_sum)[:, None] * bg
        results["image"] = image.view(*prefix, C)
        results["depth"] = depth.view(*prefix)
        results["weights_sum"] = weights_sum.view(*prefix)
        return results

    def _aabb_host(self, a):
        key = "_aabb_host_cache"
        cached = getattr(self, key, None)
        if cached is None or cached[0] is not a:
            cached = (a, [float(v) for v in a.tolist()])
            setattr(self, key, cached)
        return cached[1]

    def run(self, rays_o, rays_d, num_steps=128, upsample_steps=0, bg_color=None, perturb=False, shading="albedo",
            **kwargs):
        """Uniform-sampling renderer (`cuda_ray=False`): num_steps samples in [near, far] per ray, optionally refined
        by `upsample_steps` importance samples drawn from the coarse pass's weights (inverse-CDF sampling between
        the mid-points of the coarse samples, stratified when not training), evaluated with the same HIP gather/MLP
        kernels and composited with the same HIP kernels (every ray owns a fixed span of samples).
        shading="normal" (evaluation only): as in run_cuda; the shaded renders ('lambertian' / 'textureless') are
        run_cuda's alone."""
        self._check_distortion(kwargs.get("distortion", False), sampler="run")
        shade_normal, _ = self._check_shading(shading, kwargs.get("light_d"), sampler="run",
                                              orient=kwargs.get("orient", False),
                                              normal_image=kwargs.get("normal_image", False))
        prefix = rays_o.shape[:-1]
        rays_o = rays_o.contiguous().view(-1, 3).float()
        rays_d = rays_d.contiguous().view(-1, 3).float()
        N, C, dev = rays_o.shape[0], (3 if shade_normal else self.img_dims), rays_o.device
        aabb = self._aabb_host(self.aabb_train if self.training else self.aabb_infer)
        nears, fars = rm.near_far_from_aabb(rays_o, rays_d, aabb, self.min_near)
        hit = nears < fars
        near = torch.where(hit, nears, torch.zeros_like(nears))
        far = torch.where(hit, fars, torch.zeros_like(fars))
        z = torch.linspace(0.0, 1.0, num_steps, device=dev)[None, :]
        z = near[:, None] + (far - near)[:, None] * z
        sample_dist = (far - near) / num_steps
        if perturb:
            z = z + (torch.rand_like(z) - 0.5) * sample_dist[:, None]

        def positions(zv):
            return (rays_o[:, None, :] + rays_d[:, None, :] * zv[..., None]).clamp(-self.bound, self.bound)

        def spacing(zv):
            return torch.cat([zv[:, 1:] - zv[:, :-1], sample_dist[:, None]], dim=1) * hit[:, None]

        if upsample_steps > 0:
            with torch.no_grad():
                flat = positions(z).reshape(-1, 3).contiguous()
                sigma_c, _ = self.field(flat, flat.shape[0])
                dt = spacing(z)
                alpha = 1.0 - torch.exp(-dt * (self.density_scale * sigma_c).view(N, num_steps))
                trans = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :1]), 1.0 - alpha + 1e-15], dim=1), dim=1)
                weights = alpha * trans[:, :-1]
                mids = z[:, :-1] + 0.5 * dt[:, :-1]
                z_fine = _sample_pdf(mids, weights[:, 1:-1], upsample_steps, stratified=not self.training)
                z = torch.sort(torch.cat([z, z_fine], dim=1), dim=1)[0]
        S = z.shape[1]
        deltas = torch.stack([spacing(z), z], -1).reshape(-1, 2).contiguous()
        ar = torch.arange(N, device=dev)
        rays = torch.stack([ar, ar * S, torch.full((N,), S, device=dev)], -1).to(torch.int32)
        flat = positions(z).reshape(-1, 3).contiguous()
        if shade_normal:
            sigmas, rgbs = self.density_normals(flat)
            rgbs = (rgbs + 1.0) / 2.0
            bg = torch.zeros(N, C, device=dev)            # (no background under a normal render)
        else:
            sigmas, rgbs = self.field(flat, flat.shape[0])
            sigmas = self.density_scale * sigmas if self.density_scale != 1.0 else sigmas
            bg = self._bg_tensor(bg_color, rays_d, N, C)
        if self.tuned and not shade_normal:
            weights_sum, depth, image, _ = rm.composite_rays_train_decode(sigmas, rgbs, deltas, rays, self.decoder, 0.0, bg)
        else:
            weights_sum, depth, image = rm.composite_rays_train(sigmas, rgbs, deltas, rays, 0.0, bg)
        return {"image": image.view(*prefix, C), "depth": depth.view(*prefix),
                "weights_sum": weights_sum.view(*prefix)}

    @torch.no_grad()
    def seed_density_grid(self, density_fn, thresh=None):
        """Fill the occupancy grid from an analytic density: `density_fn(xyz [G^3,3]) -> [G^3]` evaluated at the cell
        centres of every cascade (the points lnerf_occ_cell_points gives, Morton order), mean and bitfield recomputed
        (`thresh` overrides `density_thresh` for the bitfield).  Used to start from a known shape (bench.py: the sphere
        of SURVEY.md section 8(d); training/shape.py seeds from a mesh the same way)."""
        G, dev = self.grid_size, self.density_grid.device
        for cas in range(self.cascade):
            xyz = torch.empty(G ** 3, 3, device=dev)
            _b.call("lnerf_occ_cell_points", None, G ** 3, cas, G, self.bound, None, _p(xyz), _stream())
            self.density_grid[cas] = density_fn(xyz).to(torch.float32)
        self.mean_density_dev.fill_(float(self.density_grid.clamp(min=0).mean()))
        rm.packbits(self.density_grid, self.density_thresh if thresh is None else float(thresh), self.density_bitfield,
                    None if thresh is not None else self.mean_density_dev)
        return self.density_bitfield

    @torch.no_grad()
    def density_lattice(self, resolution=None, S=128):
        """sigma x density_scale on a resolution^3 lattice spanning [-bound, bound]^3 -> [R, R, R] f32 on the device
        (z fastest; point (i, j, k) at -bound + 2 bound * (i, j, k) / (R - 1), the coordinates lnerf_marching_cubes
        gives the lattice), queried through field() in S^3-point chunks."""
        R = int(resolution or self.grid_size)
        S = int(S)
        dev = self.density_grid.device
        lo = torch.tensor(-self.bound, dtype=torch.float32, device=dev)
        span = torch.tensor(self.bound, dtype=torch.float32, device=dev) - lo
        den = torch.tensor(float(R - 1), dtype=torch.float32, device=dev)
        coords = lo + (span * torch.arange(R, dtype=torch.float32, device=dev)) / den
        vol = torch.empty(R, R, R, device=dev, dtype=torch.float32)
        for x0 in range(0, R, S):
            for y0 in range(0, R, S):
                for z0 in range(0, R, S):
                    xs, ys, zs = coords[x0:x0 + S], coords[y0:y0 + S], coords[z0:z0 + S]
                    pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3).contiguous()
                    sigmas, _ = self.field(pts, pts.shape[0])
                    vol[x0:x0 + S, y0:y0 + S, z0:z0 + S] = (sigmas * self.density_scale).view(len(xs), len(ys), len(zs))
        return vol

    def _latent_preview(self, feats):
        """[N,C] field features -> [N,3] RGB in [0, 1]: latent mode, the linear latent->RGB preview; latent_tune, the
        model's decoder; RGB mode, the first three channels."""
        from ..training.guidance import LATENT_TO_RGB
        if self.tuned and feats.shape[-1] == 4:
            return self.decode_points(feats)
        if self.latent_mode and feats.shape[-1] == 4:
            m = torch.tensor(LATENT_TO_RGB, device=feats.device, dtype=torch.float32)
            rgb = (feats.float() @ m) / 2 + 0.5
        else:
            rgb = feats[:, :3].float()
        return rgb.clamp(0, 1)

    @torch.no_grad()
    def bake_texture(self, verts, faces, vt, ft, resolution=1024, gutter=4, S=128, fn=None, fill="dilate"):
        """Sample the field over a mesh's UV atlas.  Every texel whose centre a face covers (lnerf_uv_raster: the
        face with the largest index where charts overlap) gets fn(surface point), fn(pts [P,3]) -> [P,C] queried in
        S^3-point chunks (default: the field's features, 4-channel latents -- latent_tune included -- or RGB); then `gutter` dilation rounds
        (lnerf_uv_dilate) spread the chart borders outwards so that bilinear lookups there do not blend in zeros.
        Texel (i, j) sits at u = (j + 0.5) / R, v = 1 - (i + 0.5) / R, the convention Latent-Paint's texture lookup uses.
        fill="pullpush": the texels the gutter leaves empty are then filled from the rest (view_bake.fill_atlas: a
        coverage-weighted pull-push over the whole atlas; mask code 3), so that mip levels built from the image do not seam.
        -> dict(texture [C,R,R] f32, mask [R,R] uint8 (2 covered, 1 gutter, 3 filled, 0 empty), rgb [3,R,R] in [0, 1])."""
        from ... import view_bake
        view_bake.check_choice(fill, view_bake.TEXTURE_FILLS, "bake_texture: fill")
        if fn is None:
            def fn(pts):
                return self.field(pts, pts.shape[0])[1]
        R = int(resolution)
        verts = verts.to(torch.float32).contiguous()
        dev = verts.device
        texel_face, texel_idx, pos = rm.uv_raster(verts, faces, vt, ft, R)
        P = pos.shape[0]
        chunk = int(S) ** 3
        feats = [fn(pos[s:s + chunk].contiguous()).float() for s in range(0, P, chunk)]
        C = feats[0].shape[-1] if feats else (4 if (self.latent_mode or self.tuned) else 3)
        texture = torch.zeros(C, R * R, device=dev, dtype=torch.float32)
        if P > 0:
            texture[:, texel_idx.long()] = torch.cat(feats).T
        mask = (texel_face.reshape(-1) >= 0).to(torch.uint8) * 2
        texture, mask = texture.view(C, R, R), mask.view(R, R)
        rm.uv_dilate(texture, mask, gutter)
        texture, mask = view_bake.fill_atlas(texture, mask, fill)
        rgb = self._latent_preview(texture.reshape(C, -1).T).T.reshape(3, R, R).contiguous()
        return {"texture": texture, "mask": mask, "rgb": rgb}

    @torch.no_grad()
    def bake_views(self, verts, faces, vt, ft, images, cams, resolution, gutter=4, fallback=None, erode=0, cos_min=0.2,
                   power=4.0, slack=2.0, fill="dilate", unseen="fallback", blend="mean", exposure=False, band_sigma=0.0):
        """Project K images of the mesh (images [K,C,H,W] seen by the camera records cams [K,14]) into its UV atlas:
        texels from lnerf_uv_raster, texel normal = the winding normal of the covering face (marching cubes winds
        outwards), visibility from view_zbuffer at the images' size, colours from project_views, `fallback` [C,R,R]
        where no view sees a texel (unseen="inpaint": filled from the seen texels instead), `gutter` dilation rounds and
        `fill` as bake_texture (view_bake.bake_views, shared with Latent-Paint).  blend = "bands" (two-band blending
        at `band_sigma` pixels) and exposure = True (one gain per view and channel): view_bake.bake_views.
        -> dict(rgb [C,R,R], view_weight [R,R], view_count [R,R] int32, mask [R,R] uint8; + view_gains [K,C] with
        exposure, view_best [R,R] int32 with "bands")."""
        from ... import view_bake
        return view_bake.bake_views(verts, faces, vt, ft, images, cams, resolution, gutter=gutter, fallback=fallback,
                                    erode=erode, cos_min=cos_min, power=power, slack=slack, fill=fill, unseen=unseen,
                                    blend=blend, exposure=exposure, band_sigma=band_sigma)

    @torch.no_grad()
    def render_bake_views(self, K, view_size=None):
        """K evaluation renders for a view bake: the directions of raymarching.bake_view_poses at the evaluation
        camera (radius_range[1] * 1.2, the mean fovy), rendered as Trainer.eval_render does (evaluation mode,
        unperturbed, the evaluation background) at `view_size` (an int or (h, w); default eval_h x eval_w).
        -> (images [K,C,h,w], cams [K,14] rasteriser records of the same cameras)."""
        from ...view_bake import view_cameras
        cfg = self.cfg
        if view_size is None or view_size == 0:
            h, w = int(cfg.eval_h), int(cfg.eval_w)
        elif isinstance(view_size, (tuple, list)):
            h, w = int(view_size[0]), int(view_size[1])
        else:
            h = w = int(view_size)
        if h < 2 or w < 2:
            raise ValueError("render_bake_views: view_size %r is smaller than 2 x 2" % (view_size,))
        dev = self.density_grid.device
        fovy = 0.5 * (cfg.fovy_range[0] + cfg.fovy_range[1])
        cams, c2w, intr = view_cameras(rm.bake_view_poses(K), cfg.radius_range[1] * 1.2, fovy, h, w, dev)
        was_training = self.training
        self.eval()
        try:
            views = []
            for pose in c2w:
                rays_o, rays_d = rm.get_rays(pose[None].to(dev), intr, h, w)
                out = self.render(rays_o, rays_d, staged=True, perturb=False, bg_color=None)
                views.append(out["image"].reshape(h, w, -1).permute(2, 0, 1).float())
        finally:
            self.train(was_training)
        return torch.stack(views).contiguous(), cams

    @torch.no_grad()
    def export_mesh(self, path, resolution=None, S=128, thresh=None, texture_resolution=0, gutter=4, target_faces=0,
                    field_normals=False, atlas="triangle", min_component_faces=0, min_component_diameter=0.0,
                    keep_largest=0, smooth_iterations=0, bake_views=0, view_size=None, view_decoder=None,
                    view_erode=None, fill="dilate", unseen="fallback", view_blend="mean", view_exposure=False,
                    view_band_sigma=0.0):
        """Triangle mesh of the density field -> `path`/mesh.obj (the upstream renderer's export_mesh(path, resolution,
        S)): the density on a `resolution`^3 lattice over [-bound, bound]^3 (density_lattice), marching cubes on the GPU
        at iso `thresh` (default min(mean density, density_thresh), as upstream) with the box capped, vertex colours
        from the field at the vertices (latent mode: the linear latent->RGB preview; latent_tune: the model's decoder,
        decode_points), clamped to [0, 1].
        texture_resolution > 0: a textured mesh instead -- the per-triangle UV atlas, the field baked into it at that
        side (bake_texture, `gutter` dilation rounds), mesh.obj with v / vt / vn / f v/vt/vn, mesh.mtl, albedo.png
        (the RGB preview; latent_tune: the decoder's colours) and, in latent and latent_tune mode, latent_texture.pt
        ([4,R,R] f32, what Latent-Paint's guide.init_texture reads).
        target_faces > 0: the marching-cubes mesh is decimated on the GPU to that many faces or one fewer first
        (raymarching.decimate_mesh); the colours, the atlas and the bake are then the decimated mesh's.
        field_normals: `normals` / the `vn` lines are the FIELD's normals at the final vertices (self.normal: the exact
        gradient of the density, after the decimation when there is one) instead of the lattice's central differences
        or the decimated mesh's face sums; a textured export also bakes an object-space normal map, stored as
        (n + 1) / 2 -- `normal_map` [3,R,R] in the result and normal_object.png beside albedo.png (mesh.mtl unchanged).
        atlas: "triangle" (the per-triangle atlas) or "charts" (raymarching.chart_atlas at texture_resolution, of the
        decimated mesh when there is a decimation: connected patches share their texture vertices, and the result also
        carries face_chart, chart_rect and atlas_scale).
        min_component_faces / min_component_diameter / keep_largest (any > 0): the marching-cubes mesh is cleaned first
        (raymarching.clean_mesh): connected components with fewer faces, or a bounding-box diagonal below that fraction
        of the whole mesh's, go -- the floaters of a field trained by score distillation -- and keep_largest = k keeps
        the k largest of the rest.  The lattice normals follow the vertices that stay.
        smooth_iterations > 0: that many Taubin iterations (raymarching.smooth_mesh) take the lattice's stair steps
        out of the surface; without a decimation the normals are then the smoothed mesh's face sums.
        Order: marching cubes, clean, smooth, decimate, then colours / field normals / atlas / bake on the final mesh.
        bake_views = K > 0 (needs texture_resolution > 0): albedo.png is baked from K RENDERED views instead of per-point
        previews -- render_bake_views at `view_size`, `view_decoder` ([K,C,h,w] renders -> [K,3,H',W'] RGB in [0, 1] at
        any up-scaling that keeps the aspect ratio, e.g. the diffusion model's VAE decoder; None: the linear preview
        for latents, the identity for RGB renders), then bake_views with the point bake as the fallback for texels no
        view sees.  `view_erode` pixels are taken off every silhouette (default: 0 at the render size, else the
        up-scaling factor, about what a decoder smears the background over).  The point bake's image is kept as
        albedo_preview.png; the result gains view_rgb [3,R,R], view_weight and view_count [R,R]; rgb, texture and
        latent_texture.pt are what they are without the option.
        fill = "pullpush" (textured): every baked image -- albedo.png, albedo_preview.png, normal_object.png,
        latent_texture.pt -- is filled beyond the gutter over the whole atlas (bake_texture); "dilate" leaves the files
        byte for byte what they were.  unseen = "inpaint" (with bake_views): covered texels no view sees are filled from
        the seen ones instead of taking the point bake's colour.
        view_blend = "bands" (with bake_views): two-band blending -- the low band of a texel is the weighted mean of the
        views' low-passed images, everything finer comes from its best view alone, so the detail a decoder invents per
        view is not averaged into a blur; view_band_sigma is the Gaussian's sigma in decoded pixels (0: max(1, decoded
        side / render side), one render pixel, as view_erode's default); the result gains view_best [R,R] int32.
        view_exposure = True: one gain per view and channel, solved from what the views show where they overlap
        (view_bake.exposure_gains), takes the brightness steps between views out; the result gains view_gains [K,3].
        Both are off by default and every file is then byte for byte what it was.
        Returns dict(verts [V,3], faces [F,3] int32, normals [V,3], colors [V,3], iso, path, faces_before (the
        marching-cubes face count), components and components_kept (None without a cleaning), faces_cleaned (the face
        count after the cleaning)) with device tensors, plus vt, ft, texture, mask, rgb when textured."""
        from ...uv_atlas import check_atlas_choice
        from .mesh_io import write_obj
        from ...view_bake import BAKE_BLENDS, BAKE_UNSEEN, TEXTURE_FILLS, check_choice
        check_atlas_choice(atlas, "export_mesh: atlas")
        check_choice(fill, TEXTURE_FILLS, "export_mesh: fill")
        check_choice(unseen, BAKE_UNSEEN, "export_mesh: unseen")
        check_choice(view_blend, BAKE_BLENDS, "export_mesh: view_blend")
        if not float(view_band_sigma) >= 0.0:
            raise ValueError("export_mesh: view_band_sigma must be >= 0 (got %r)" % (view_band_sigma,))
        min_component_faces, min_component_diameter = int(min_component_faces), float(min_component_diameter)
        keep_largest, smooth_iterations = int(keep_largest), int(smooth_iterations)
        bake_views = int(bake_views)
        if bake_views < 0:
            raise ValueError("export_mesh: bake_views must be >= 0 (got %d)" % bake_views)
        if bake_views > 0 and int(texture_resolution) <= 0:
            raise ValueError("export_mesh: bake_views = %d needs texture_resolution > 0 (the views are baked into the "
                             "texture)" % bake_views)
        if bake_views == 0 and (view_blend != "mean" or view_exposure):
            raise ValueError("export_mesh: view_blend = %r / view_exposure = %r need bake_views > 0"
                             % (view_blend, view_exposure))
        if min_component_faces < 0 or keep_largest < 0:
            raise ValueError("export_mesh: min_component_faces (%d) and keep_largest (%d) must be >= 0"
                             % (min_component_faces, keep_largest))
        if not 0.0 <= min_component_diameter <= 1.0:
            raise ValueError("export_mesh: min_component_diameter %r outside [0, 1]" % min_component_diameter)
        if not 0 <= smooth_iterations <= _b.SMOOTH_MAX_ITER:
            raise ValueError("export_mesh: smooth_iterations %d outside [0, %d]" % (smooth_iterations, _b.SMOOTH_MAX_ITER))
        vol = self.density_lattice(resolution, S)
        if thresh is None:
            iso = float(torch.clamp(self.mean_density_dev.reshape(-1)[0], max=float(self.density_thresh)))
        else:
            iso = float(thresh)
        b = self.bound
        verts, faces, normals = rm.marching_cubes(vol, iso, (-b, -b, -b), (b, b, b), close_boundary=True)
        faces_before = int(faces.shape[0])
        del vol
        components = components_kept = None
        if min_component_faces > 0 or min_component_diameter > 0.0 or keep_largest > 0:
            st = {}
            verts, faces, vert_src = rm.clean_mesh(verts, faces, min_component_faces, min_component_diameter, keep_largest,
                                                   stats=st)
            normals = normals[vert_src]
            components, components_kept = st["components"], st["kept"]
        faces_cleaned = int(faces.shape[0])
        if smooth_iterations > 0:
            verts, normals = rm.smooth_mesh(verts, faces, smooth_iterations)
        if int(target_faces) > 0:
            verts, faces, normals = rm.decimate_mesh(verts, faces, int(target_faces))
        colors = torch.empty(verts.shape[0], 3, device=verts.device)
        chunk = S ** 3
        for s in range(0, verts.shape[0], chunk):
            pts = verts[s:s + chunk].contiguous()
            _, feats = self.field(pts, pts.shape[0])
            colors[s:s + chunk] = self._latent_preview(feats)
        if field_normals:
            normals = (torch.cat([self.normal(verts[s:s + chunk].contiguous()) for s in range(0, verts.shape[0], chunk)])
                       if verts.shape[0] > 0 else torch.zeros(0, 3, device=verts.device))
        out = os.path.join(str(path), "mesh.obj")
        result = {"verts": verts, "faces": faces, "normals": normals, "colors": colors, "iso": iso, "path": out,
                  "faces_before": faces_before, "components": components, "components_kept": components_kept,
                  "faces_cleaned": faces_cleaned}
        if int(texture_resolution) > 0:
            result.update(self._export_textured(str(path), verts, faces, normals, int(texture_resolution), gutter, S,
                                                bool(field_normals), atlas,
                                                views=(bake_views, view_size, view_decoder, view_erode), fill=fill,
                                                unseen=unseen,
                                                blend=(view_blend, bool(view_exposure), float(view_band_sigma))))
        else:
            write_obj(out, verts.cpu().numpy(), faces.cpu().numpy(), normals.cpu().numpy(), colors.cpu().numpy())
        return result

    def _export_textured(self, path, verts, faces, normals, R, gutter, S, normal_map=False, atlas="triangle",
                         views=(0, None, None, None), fill="dilate", unseen="fallback", blend=("mean", False, 0.0)):
        """The textured half of export_mesh: atlas, bake, mesh.obj + mesh.mtl + albedo.png (+ latent_texture.pt;
        normal_map: + normal_object.png, the field's normals over the same atlas; views = (K, size, decoder, erode)
        with K > 0: albedo.png from K rendered views, the point bake's image as albedo_preview.png; `fill` and `unseen`
        as export_mesh; blend = (view_blend, view_exposure, view_band_sigma))."""
        import warnings

        import numpy as np
        from PIL import Image

        from ...uv_atlas import MIN_TEXELS_PER_CELL, atlas_cells, atlas_min_resolution, per_triangle_atlas
        from .mesh_io import write_textured_obj
        F = faces.shape[0]
        extra = {}
        if atlas == "charts":
            vt, ft, info = rm.chart_atlas(verts, faces, R)
            extra = {"face_chart": info["face_chart"], "chart_rect": info["chart_rect"], "atlas_scale": info["scale"]}
        else:
            need = atlas_min_resolution(F)
            if F > 0 and R < need:
                warnings.warn("export_mesh: texture_resolution %d gives the per-triangle atlas of %d faces %.1f texels per "
                              "chart cell (fewer than %d): use texture_resolution >= %d, or target_faces <= %d"
                              % (R, F, R / atlas_cells(F), MIN_TEXELS_PER_CELL, need, 2 * (R // MIN_TEXELS_PER_CELL) ** 2),
                              stacklevel=3)
            vt, ft = per_triangle_atlas(F, verts.device)
        baked = self.bake_texture(verts, faces, vt, ft, resolution=R, gutter=gutter, S=S, fill=fill)
        os.makedirs(path, exist_ok=True)
        out = os.path.join(path, "mesh.obj")
        write_textured_obj(out, verts.cpu().numpy(), faces.cpu().numpy(), vt.cpu().numpy(), ft.cpu().numpy(),
                           normals.cpu().numpy(), material="mesh.mtl", texture="albedo.png")
        albedo = (baked["rgb"].permute(1, 2, 0).cpu().numpy() * 255).round().astype(np.uint8)
        if views[0] > 0:
            from ...view_bake import to_uint8
            Image.fromarray(albedo).save(os.path.join(path, "albedo_preview.png"))
            seen = self._bake_rendered_views(verts, faces, vt, ft, R, gutter, baked["rgb"], *views, fill=fill,
                                             unseen=unseen, blend=blend)
            baked = dict(baked, view_rgb=seen["rgb"], view_weight=seen["view_weight"], view_count=seen["view_count"],
                         **{k: seen[k] for k in ("view_gains", "view_best") if k in seen})
            albedo = to_uint8(seen["rgb"])
        Image.fromarray(albedo).save(os.path.join(path, "albedo.png"))
        if (self.latent_mode or self.tuned) and baked["texture"].shape[0] == 4:
            torch.save(baked["texture"].cpu(), os.path.join(path, "latent_texture.pt"))
        if normal_map:
            nmap = self.bake_texture(verts, faces, vt, ft, resolution=R, gutter=gutter, S=S,
                                     fn=lambda pts: (self.normal(pts) + 1.0) / 2.0, fill=fill)["texture"]
            img = (nmap.clamp(0, 1).permute(1, 2, 0).cpu().numpy() * 255).round().astype(np.uint8)
            Image.fromarray(img).save(os.path.join(path, "normal_object.png"))
            baked = dict(baked, normal_map=nmap)
        return dict(baked, vt=vt, ft=ft, **extra)

    def _bake_rendered_views(self, verts, faces, vt, ft, R, gutter, fallback, K, view_size, view_decoder, view_erode,
                             fill="dilate", unseen="fallback", blend=("mean", False, 0.0)):
        """export_mesh's view bake: K renders, decoded as images, projected into the atlas over `fallback`."""
        renders, cams = self.render_bake_views(K, view_size)
        h, w = renders.shape[-2:]
        if view_decoder is None:
            C = renders.shape[1]
            images = self._latent_preview(renders.permute(0, 2, 3, 1).reshape(-1, C)).reshape(K, h, w, 3).permute(0, 3, 1, 2)
        else:
            images = view_decoder(renders)
        if images.dim() != 4 or images.shape[0] != K or images.shape[1] != 3:
            raise ValueError("export_mesh: view_decoder must return [K,3,H,W] = [%d,3,...], not %s"
                             % (K, tuple(images.shape)))
        H, W = (int(v) for v in images.shape[-2:])
        if H * w != W * h:
            raise ValueError("export_mesh: view_decoder changed the aspect ratio (%d x %d -> %d x %d)" % (h, w, H, W))
        if view_erode is None:
            view_erode = 0 if (H, W) == (h, w) else max(1, -(-H // h))
        return self.bake_views(verts, faces, vt, ft, images.float().clamp(0, 1), cams, R, gutter=gutter, fallback=fallback,
                               erode=int(view_erode), fill=fill, unseen=unseen, blend=blend[0], exposure=blend[1],
                               band_sigma=blend[2] if blend[2] > 0 else max(1.0, H / h))

    def shadow_extra_state(self):
        """Context manager: inside it the occupancy state (density grid, bitfield, mean) is a SHADOW copy, so
        update_extra_state() does all of its work -- cell sampling, the density query, decayed maximum, mean, bitfield --
        without changing the scene the march sees.  bench.py times the refresh inside its timed steps this way while the
        analytic occupancy of its workload stays pinned."""
        return _ShadowExtraState(self)

    def occupancy_generator(self, seed=None):
        """The generator the occupancy refresh draws its cell samples and jitter from.  Replicas of a data-parallel run
        refresh their grids redundantly: with the same seed on every rank (the trainer passes `optim.seed`) and the
        order-independent update kernels they stay bit-identical without any exchange."""
        dev = self.density_grid.device
        if seed is not None or self._occ_gen is None or self._occ_gen.device != dev:
            self._occ_gen = torch.Generator(device=dev)
            self._occ_gen.manual_seed(0x0CC0 + (0 if seed is None else int(seed)))
            if seed is not None:
                self._occ_seed = 0x0CC0 + int(seed)     # the device-side sampler's seed (steady-state refreshes)
        return self._occ_gen

    @torch.no_grad()
    def update_extra_state(self, decay=0.95, S=128):
        """Occupancy-grid refresh (every `update_extra_interval` steps): evaluate the density at
        jittered cell centres (all cells for the first 16 refreshes, then G^3/4 random + G^3/4
        occupied cells), decayed-max into the grid, recompute the mean and repack the bitfield.
        Deterministic given the generator state and the weights (see occupancy_generator)."""
        if not self.cuda_ray:
            return
        if self.training:
            self.update_sample_budget()
        dev = self.density_grid.device
        gen = self.occupancy_generator()
        G, G3 = self.grid_size, self.grid_size ** 3
        chunk = 1 << 20
        if self._occ_cells is None or self._occ_cells.device != dev:
            self._occ_cells = torch.zeros(G3, device=dev, dtype=torch.int32)   # scratch of lnerf_occ_update, zero between calls
        fused_mean = False
        for cas in range(self.cascade):
            if self.iter_density >= 16 and getattr(self.cfg, "occ_device_sampling", True):
                # steady state: G^3/4 random + G^3/4 occupied cells, drawn on the device (lnerf_occ_sample): no
                # torch.nonzero, hence no host synchronisation, and 3 launches instead of 7; a function of
                # (grid, seed, refresh number) alone, so data-parallel replicas draw the same cells
                n_rand = G3 // 4
                if self._occ_sample_ws is None or self._occ_sample_ws[0].device != dev:
                    nb = _b.get_lib().lnerf_occ_sample_scratch_bytes(G3)
                    self._occ_sample_ws = (torch.empty(nb, device=dev, dtype=torch.uint8),
                                           torch.empty(2 * n_rand, device=dev, dtype=torch.int32),
                                           torch.empty(2 * n_rand, 3, device=dev))
                scratch, idx, xyzs = self._occ_sample_ws
                level = self.density_grid[cas]
                _b.call("lnerf_occ_sample", _p(level), G3, cas, G, self.bound, n_rand, self._occ_seed & 0xFFFFFFFF,
                        (self.iter_density * 8 + cas) & 0xFFFFFFFF, _p(scratch), _p(idx), _p(xyzs), _stream())
                sigmas, _ = self.field(xyzs, 2 * n_rand)
                sigmas = sigmas.contiguous() if self.density_scale == 1.0 else (sigmas * self.density_scale).contiguous()
                if self.cascade == 1:
                    # one cascade: update + mean together, the apply pass streaming over the cells
                    if self._occ_scratch is None or self._occ_scratch.device != dev:
                        self._occ_scratch = torch.zeros(256, device=dev)
                    _b.call("lnerf_occ_update_mean", _p(level), G3, _p(idx), 2 * n_rand, _p(sigmas), float(decay),
                            _p(self._occ_cells), _p(self.mean_density_dev), _p(self._occ_scratch), _stream())
                    fused_mean = True
                    continue
                _b.call("lnerf_occ_update", _p(level), _p(idx), 2 * n_rand, _p(sigmas), float(decay), _p(self._occ_cells),
                        _stream())
                continue
            if self.iter_density < 16:
                indices = None
                n = G3
            else:
                n_rand = G3 // 4
                rand_idx = torch.randint(0, G3, (n_rand,), device=dev, dtype=torch.int32, generator=gen)
                occ = torch.nonzero(self.density_grid[cas] > 0).squeeze(-1)
                if occ.numel() > 0:
                    pick = torch.randint(0, occ.numel(), (n_rand,), device=dev, generator=gen)
                    occ_idx = occ[pick].to(torch.int32)
                    indices = torch.cat([rand_idx, occ_idx])
                else:
                    indices = rand_idx
                n = indices.numel()
            level = self.density_grid[cas]
            for s in range(0, n, chunk):
                e = min(s + chunk, n)
                idx = None if indices is None else indices[s:e].contiguous()
                if idx is None:
                    idx = torch.arange(s, e, device=dev, dtype=torch.int32)
                noise = torch.rand(e - s, 3, device=dev, generator=gen)
                xyzs = torch.empty(e - s, 3, device=dev)
                _b.call("lnerf_occ_cell_points", _p(idx), e - s, cas, G, self.bound, _p(noise), _p(xyzs), _stream())
                sigmas, _ = self.field(xyzs, e - s)
                sigmas = (sigmas * self.density_scale).contiguous()
                _b.call("lnerf_occ_update", _p(level), _p(idx), e - s, _p(sigmas), float(decay), _p(self._occ_cells),
                        _stream())
        if not fused_mean:
            if self._occ_scratch is None or self._occ_scratch.device != dev:
                self._occ_scratch = torch.zeros(256, device=dev)
            _b.call("lnerf_occ_mean", _p(self.density_grid), self.density_grid.numel(), _p(self.mean_density_dev),
                    _p(self._occ_scratch), _stream())
        self.iter_density += 1
        rm.packbits(self.density_grid, self.density_thresh, self.density_bitfield, self.mean_density_dev)

    def render(self, rays_o, rays_d, staged=False, max_ray_batch=4096, **kwargs):
        """rays_o, rays_d [B,N,3] -> dict with 'image' [B,N,C], 'depth' [B,N], 'weights_sum' [B,N]."""
        _run = self.run_cuda if self.cuda_ray else self.run
        if not self.cuda_ray:   # the uniform sampler takes its sample counts from the config (render.num_steps / upsample_steps)
            kwargs.setdefault("num_steps", self.cfg.num_steps)
            kwargs.setdefault("upsample_steps", self.cfg.upsample_steps)
        if kwargs.get("prepared") is not None or (kwargs.get("camera") is not None and self.cuda_ray and self.training):
            # a PreparedRays, or camera=(poses, intrinsics, H, W): the rays are generated inside the march
            kwargs.pop("force_all_rays", None)
            return self.run_cuda(None, None, **kwargs)
        camera = kwargs.pop("camera", None)
        if camera is not None and rays_o is None:   # inference / uniform sampler: plain ray generation first
            poses, intr, him, wim = camera
            if torch.is_tensor(intr):               # (device intrinsics are the training form; one read-back here)
                intr = [float(v) for v in intr.reshape(-1)[:4].tolist()]
            rays_o, rays_d = rm.get_rays(poses, intr, int(him), int(wim))
        B, N = rays_o.shape[:2]
        if staged and not self.cuda_ray:
            dev = rays_o.device
            depth = torch.empty(B, N, device=dev)
            image = torch.empty(B, N, 3 if kwargs.get("shading", "albedo") == "normal" else self.img_dims, device=dev)
            wsum = torch.empty(B, N, device=dev)
            for b in range(B):
                for head in range(0, N, max_ray_batch):
                    tail = min(head + max_ray_batch, N)
                    r = _run(rays_o[b:b + 1, head:tail], rays_d[b:b + 1, head:tail], **kwargs)
                    depth[b:b + 1, head:tail] = r["depth"]
                    image[b:b + 1, head:tail] = r["image"]
                    wsum[b:b + 1, head:tail] = r["weights_sum"]
            return {"depth": depth, "image": image, "weights_sum": wsum}
        return _run(rays_o, rays_d, **kwargs)
