"""Python surface of the HIP ray-marching ops -- the counterpart of the `raymarching` CUDA
extension module that the reference's README lists under src/latent_nerf/raymarching
(README.md:152-156) but does not ship.  Names and argument meaning follow the upstream
torch-ngp / stable-dreamfusion module the reference says it is based on (README.md:163), as
enumerated in SURVEY.md §8(b); every op runs on liblnerf_hip.so through its C ABI.

Conventions that differ from a CUDA port, by design for MI355X:
  * `march_rays_train` is deterministic (per-ray count -> scan -> write) and never syncs with
    the host: it returns capacity-sized buffers plus a device counter; consumers take the
    counter (`m_dev`) instead of a Python int.
  * per-sample features are level-major ([L, capacity, 2]).
  * `deltas[:, 1]` is the absolute ray parameter t (depth = sum w_i t_i).
"""
import ctypes
import math
import typing

import torch

from . import backend as _b

_NULL = None


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current stream's handle.  torch.cuda.current_stream() builds a Stream object through four Python layers
    (~13 us; five calls per training step); the raw getter is what torch's own extension launchers use."""
    if _raw_stream is not None:
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t, name, dtype=torch.float32, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("%s: tensor is required" % name)
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (got %s); there is no CPU path" % (name, t.device))
    if t.dtype != dtype:
        raise TypeError("%s must be %s (got %s)" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    return ctypes.c_void_p(t.data_ptr())


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------ H1 / H2 / H3
def get_rays(poses, intrinsics, H, W):
    """poses [B,4,4] (camera-to-world, columns right/down/forward/eye), intrinsics (fx,fy,cx,cy)
    -> rays_o, rays_d [B, H*W, 3]."""
    if poses.dim() == 2:
        poses = poses[None]
    poses = poses.contiguous()
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    B = poses.shape[0]
    rays_o = torch.empty(B, H * W, 3, device=poses.device, dtype=torch.float32)
    rays_d = torch.empty_like(rays_o)
    _b.call("lnerf_get_rays", _chk(poses, "poses"), B, H, W, fx, fy, cx, cy, _p(rays_o), _p(rays_d), _stream())
    return rays_o, rays_d


def near_far_from_aabb(rays_o, rays_d, aabb, min_near=0.2):
    """rays [N,3]; aabb: 6 floats (list/tuple/CPU or GPU tensor) -> nears, fars [N]."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    N = rays_o.shape[0]
    a = [float(v) for v in (aabb.tolist() if isinstance(aabb, torch.Tensor) else aabb)]
    nears = torch.empty(N, device=rays_o.device, dtype=torch.float32)
    fars = torch.empty_like(nears)
    _b.call("lnerf_near_far_from_aabb", _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), N, a[0], a[1], a[2], a[3], a[4],
            a[5], float(min_near), _p(nears), _p(fars), _stream())
    return nears, fars


def morton3D(coords):
    """coords int32 [N,3] -> int32 [N] Morton index (x in bit 0)."""
    coords = coords.contiguous()
    N = coords.shape[0]
    out = torch.empty(N, device=coords.device, dtype=torch.int32)
    _b.call("lnerf_morton3d", _chk(coords, "coords", torch.int32), N, _p(out), _stream())
    return out


def morton3D_invert(indices):
    indices = indices.contiguous()
    N = indices.shape[0]
    out = torch.empty(N, 3, device=indices.device, dtype=torch.int32)
    _b.call("lnerf_morton3d_invert", _chk(indices, "indices", torch.int32), N, _p(out), _stream())
    return out


def packbits(grid, thresh, bitfield=None, mean_dev=None):
    """grid f32 [C, H^3] (Morton order) -> uint8 [C*H^3/8]; threshold = min(thresh, *mean_dev)."""
    grid = grid.contiguous()
    n = grid.numel()
    if bitfield is None:
        bitfield = torch.empty(n // 8, device=grid.device, dtype=torch.uint8)
    _b.call("lnerf_packbits", _chk(grid, "grid"), n, float(thresh), _chk(mean_dev, "mean_dev", allow_none=True),
            _chk(bitfield, "bitfield", torch.uint8), _stream())
    return bitfield


# ------------------------------------------------------------------------------ H4
class MarchResult:
    """Capacity-sized sample buffers of one training march.  `counter` (int32 [4 + scratch], device) holds
    [M, live rays, rays dropped for capacity, running peak of M | (dropped ? 2^30 : 0) over the marches into these
    buffers]; nothing here forces a host sync."""
    __slots__ = ("xyzs", "dirs", "deltas", "rays", "counter", "capacity")

    def __init__(self, xyzs, dirs, deltas, rays, counter, capacity):
        self.xyzs, self.dirs, self.deltas, self.rays, self.counter, self.capacity = (xyzs, dirs, deltas, rays, counter,
                                                                                   capacity)

    def take_peak(self):
        """(largest M, any ray dropped) of the marches into these buffers since the last call: ONE read-back
        (synchronises), then the word is cleared."""
        w = int(self.counter[3].item())
        self.counter[3:4].zero_()
        return w & ((1 << 30) - 1), bool(w >> 30)

    def num_samples(self) -> int:
        """Host read-back of M (synchronises)."""
        return int(self.counter[0].item())

    def trimmed(self):
        M = self.num_samples()
        return self.xyzs[:M], self.dirs[:M], self.deltas[:M], self.rays


def march_rays_train(rays_o, rays_d, bound, density_bitfield, C, H, nears, fars, perturb=False, dt_gamma=0.0,
                     max_steps=1024, capacity=None, noises=None, out=None, noise_state=None, aabb=None, min_near=0.0,
                     camera=None):
    """Occupancy-pruned march of N rays.  Returns a MarchResult.

    camera = (poses [B,4,4], (fx, fy, cx, cy), H_img, W_img) with rays_o / rays_d = PREALLOCATED [B*H*W, 3] outputs (and
    `aabb`): the rays are generated inside the march's count pass (lnerf_march_rays_train_pose: get_rays' arithmetic)
    and written to those tensors.

    nears / fars [N] from near_far_from_aabb -- or None with `aabb` = six host floats (+ `min_near`): the clip is
    then done inside the march passes (lnerf_march_rays_train_aabb: same arithmetic, one dispatch less).

    capacity: sample buffer size (default N * min(max_steps, 256)); rays that would overflow it
    are dropped and counted in counter[2].  `out` may pass a previous MarchResult to reuse its
    buffers.
    perturb: jitter of the march start.  `noises` [N] gives the values (upstream: torch.rand(N)); otherwise
    `noise_state` = (seed, int32 device counter [1]) selects the in-kernel counter-based generator (the call
    advances the counter; graph-capturable without host RNG state); with neither, torch.rand(N) is drawn here."""
    rays_o = rays_o.contiguous().view(-1, 3)
    rays_d = rays_d.contiguous().view(-1, 3)
    N = rays_o.shape[0]
    dev = rays_o.device
    if capacity is None:
        capacity = max(N * min(int(max_steps), 256), 64)
    seed, noise_counter = 0, None
    if perturb and noises is None:
        if noise_state is not None:
            seed, noise_counter = int(noise_state[0]) & 0xFFFFFFFF, noise_state[1]
        else:
            noises = torch.rand(N, device=dev, dtype=torch.float32)
    if out is not None and out.capacity == capacity and out.rays.shape[0] == N:
        xyzs, dirs, deltas, rays, counter = out.xyzs, out.dirs, out.deltas, out.rays, out.counter
        # The kernels write through raw pointers, which autograd cannot see: tell it that these buffers change, so
        # that a backward pass of an EARLIER render that saved them fails loudly ("modified by an inplace operation")
        # instead of silently using this march's samples.  Host-side bookkeeping only, no launch.
        for t in (xyzs, dirs, deltas, rays, counter):
            torch.autograd.graph.increment_version(t)
    else:
        xyzs = torch.empty(capacity, 3, device=dev, dtype=torch.float32)
        dirs = torch.empty(capacity, 3, device=dev, dtype=torch.float32)
        deltas = torch.empty(capacity, 2, device=dev, dtype=torch.float32)
        rays = torch.empty(N, 3, device=dev, dtype=torch.int32)
        # (four totals + the scratch the two-launch form of the march keeps its per-ray counts in; ZEROED: word 3 is a
        # running peak the library only ever raises -- MarchResult.take_peak() reads and clears it)
        counter = torch.zeros(int(_b.get_lib().lnerf_march_counter_len(N)), device=dev, dtype=torch.int32)
    # the four entry points differ in where the rays come from (their leading arguments) and end alike
    if camera is not None:
        if aabb is None or nears is not None:
            raise ValueError("march_rays_train(camera=...) needs aabb= and no nears/fars")
        poses, intr, him, wim = camera
        poses = poses.contiguous()
        if poses.shape[0] * him * wim != N:
            raise ValueError("camera describes %d rays, the ray buffers hold %d" % (poses.shape[0] * him * wim, N))
        if torch.is_tensor(intr):
            # intrinsics as a device tensor [B,4]: nothing of the camera is a launch argument (graph replays render
            # whatever the caller copied into `poses` / `intr`)
            intr = intr.view(-1, 4)
            if intr.shape[0] != poses.shape[0]:
                raise ValueError("intrinsics tensor must be [B,4]")
            entry = "lnerf_march_rays_train_camera"
            head = (_chk(poses, "poses"), _chk(intr, "intrinsics"), int(poses.shape[0]), int(him), int(wim))
        else:
            entry = "lnerf_march_rays_train_pose"
            fx, fy, cx, cy = [float(v) for v in intr]
            head = (_chk(poses, "poses"), int(poses.shape[0]), int(him), int(wim), fx, fy, cx, cy)
        head += (_chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), *[float(v) for v in aabb], float(min_near))
    elif nears is None and aabb is not None:
        entry = "lnerf_march_rays_train_aabb"
        head = (_chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), *[float(v) for v in aabb], float(min_near), N)
    else:
        entry = "lnerf_march_rays_train"
        head = (_chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(nears, "nears"), _chk(fars, "fars"), N)
    _b.call(entry, *head, _chk(density_bitfield, "density_bitfield", torch.uint8), float(bound), int(C), int(H),
            int(max_steps), float(dt_gamma), _chk(noises, "noises", allow_none=True), seed,
            _chk(noise_counter, "noise_counter", torch.int32, allow_none=True), int(capacity), _p(xyzs), _p(dirs),
            _p(deltas), _p(rays), _p(counter), _stream())
    return MarchResult(xyzs, dirs, deltas, rays, counter, capacity)


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, density_bitfield, C, H, fars,
               dt_gamma=0.0, max_steps=1024):
    """Inference march: up to n_step samples for each of the first n_alive entries of rays_alive."""
    dev = rays_o.device
    xyzs = torch.empty(n_alive * n_step, 3, device=dev, dtype=torch.float32)
    dirs = torch.empty(n_alive * n_step, 3, device=dev, dtype=torch.float32)
    deltas = torch.empty(n_alive * n_step, 2, device=dev, dtype=torch.float32)
    _b.call("lnerf_march_rays", int(n_alive), int(n_step), _chk(rays_alive, "rays_alive", torch.int32),
            _chk(rays_t, "rays_t"), _chk(rays_o, "rays_o"), _chk(rays_d, "rays_d"), _chk(fars, "fars"),
            _chk(density_bitfield, "density_bitfield", torch.uint8), float(bound), int(C), int(H), int(max_steps),
            float(dt_gamma), _p(xyzs), _p(dirs), _p(deltas), _stream())
    return xyzs, dirs, deltas


def composite_rays(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image,
                   transmittance, T_thresh=1e-4):
    C = image.shape[-1]
    _b.call("lnerf_composite_rays", int(n_alive), int(n_step), _chk(rays_alive, "rays_alive", torch.int32),
            _chk(rays_t, "rays_t"), _chk(sigmas, "sigmas"), _chk(rgbs, "rgbs"), _chk(deltas, "deltas"), int(C),
            float(T_thresh), _chk(weights_sum, "weights_sum"), _chk(depth, "depth"), _chk(image, "image"),
            _chk(transmittance, "transmittance"), _stream())


def compact_rays(rays_alive, n, out=None, n_alive_dev=None):
    """Keep entries >= 0 of rays_alive[:n] (order preserved).  Returns (compacted, count tensor)."""
    if out is None:
        out = torch.empty_like(rays_alive)
    if n_alive_dev is None:
        n_alive_dev = torch.empty(1, device=rays_alive.device, dtype=torch.int32)
    _b.call("lnerf_compact_rays", _chk(rays_alive, "rays_alive", torch.int32), int(n), _p(out), _p(n_alive_dev),
            _stream())
    return out, n_alive_dev


# ------------------------------------------------------------------------------ H8 / H9
class _CompositeRaysTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigmas, rgbs, deltas, rays, T_thresh, bg_color):
        sigmas = sigmas.contiguous()
        rgbs = rgbs.contiguous()
        N = rays.shape[0]
        C = rgbs.shape[1]
        dev = sigmas.device
        weights_sum = torch.empty(N, device=dev, dtype=torch.float32)
        depth = torch.empty(N, device=dev, dtype=torch.float32)
        image = torch.empty(N, C, device=dev, dtype=torch.float32)
        bg = None if bg_color is None else bg_color.contiguous()
        _b.call("lnerf_composite_rays_train_forward", _chk(sigmas, "sigmas"), _chk(rgbs, "rgbs"),
                _chk(deltas, "deltas"), _chk(rays, "rays", torch.int32), N, C, float(T_thresh),
                _chk(bg, "bg_color", allow_none=True), _p(weights_sum), _p(depth), _p(image), _stream())
        ctx.save_for_backward(sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg)
        ctx.set_materialize_grads(False)  # unused outputs (depth, weights_sum) arrive as None, not as zero fills
        ctx.T_thresh = float(T_thresh)
        ctx.bg_needs_grad = bg_color is not None and bg_color.requires_grad
        return weights_sum, depth, image

    @staticmethod
    def backward(ctx, g_ws, g_depth, g_image):
        sigmas, rgbs, deltas, rays, weights_sum, depth, image, bg = ctx.saved_tensors
        N, C = rays.shape[0], rgbs.shape[1]
        g_image = torch.zeros_like(image) if g_image is None else g_image.contiguous()
        g_ws = None if g_ws is None else g_ws.contiguous()
        g_depth = None if g_depth is None else g_depth.contiguous()
        d_sigmas = torch.empty_like(sigmas)
        d_rgbs = torch.empty_like(rgbs)
        d_bg = torch.empty_like(bg) if ctx.bg_needs_grad else None
        _b.call("lnerf_composite_rays_train_backward", _chk(g_ws, "grad_weights_sum", allow_none=True),
                _chk(g_depth, "grad_depth", allow_none=True), _chk(g_image, "grad_image"), _p(sigmas), _p(rgbs),
                _p(deltas), _p(rays), _p(weights_sum), _p(depth), _p(image), _p(bg), N, C, ctx.T_thresh, _p(d_sigmas),
                _p(d_rgbs), _p(d_bg), _stream())
        return d_sigmas, d_rgbs, None, None, None, d_bg


def composite_rays_train(sigmas, rgbs, deltas, rays, T_thresh=1e-4, bg_color=None):
    """sigmas [M], rgbs [M,C], deltas [M,2]=(dt,t), rays int32 [N,3]=(id,offset,count)
    -> weights_sum [N], depth [N], image [N,C] (+ (1-weights_sum)*bg_color)."""
    return _CompositeRaysTrain.apply(sigmas, rgbs, deltas, rays, T_thresh, bg_color)


class _CompositeRaysTrainDecode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sigmas, latents, deltas, rays, decoder, T_thresh, bg_color):
        sigmas = sigmas.contiguous()
        latents = latents.contiguous()
        decoder = decoder.contiguous()
        if latents.shape[1] != 4 or tuple(decoder.shape) != (3, 4):
            raise ValueError("composite_rays_train_decode: latents must be [M,4] and the decoder [3,4]")
        N = rays.shape[0]
        dev = sigmas.device
        weights_sum = torch.empty(N, device=dev, dtype=torch.float32)
        depth = torch.empty(N, device=dev, dtype=torch.float32)
        latent_image = torch.empty(N, 4, device=dev, dtype=torch.float32)
        image = torch.empty(N, 3, device=dev, dtype=torch.float32)
        bg = None if bg_color is None else bg_color.contiguous()
        _b.call("lnerf_composite_rays_train_decode_forward", _chk(sigmas, "sigmas"), _chk(latents, "latents"),
                _chk(deltas, "deltas"), _chk(rays, "rays", torch.int32), N, float(T_thresh), _chk(decoder, "decoder"),
                _chk(bg, "bg_color", allow_none=True), _p(weights_sum), _p(depth), _p(latent_image), _p(image), _stream())
        ctx.save_for_backward(sigmas, latents, deltas, rays, decoder, weights_sum, depth, latent_image, bg)
        ctx.set_materialize_grads(False)  # unused outputs (depth, weights_sum) arrive as None, not as zero fills
        ctx.mark_non_differentiable(latent_image)
        ctx.T_thresh = float(T_thresh)
        ctx.bg_needs_grad = bg_color is not None and bg_color.requires_grad
        return weights_sum, depth, image, latent_image

    @staticmethod
    def backward(ctx, g_ws, g_depth, g_image, _g_latent_image):
        sigmas, latents, deltas, rays, decoder, weights_sum, depth, latent_image, bg = ctx.saved_tensors
        N = rays.shape[0]
        g_image = torch.zeros(N, 3, device=sigmas.device) if g_image is None else g_image.contiguous()
        g_ws = None if g_ws is None else g_ws.contiguous()
        g_depth = None if g_depth is None else g_depth.contiguous()
        d_sigmas = torch.empty_like(sigmas)
        d_latents = torch.empty_like(latents)
        d_bg = torch.empty_like(bg) if ctx.bg_needs_grad else None
        # (N == 0: the library launches nothing, and the sum over no rays is zero)
        d_decoder = torch.empty_like(decoder) if N > 0 else torch.zeros_like(decoder)
        _b.call("lnerf_composite_rays_train_decode_backward", _chk(g_ws, "grad_weights_sum", allow_none=True),
                _chk(g_depth, "grad_depth", allow_none=True), _chk(g_image, "grad_image"), _p(sigmas), _p(latents),
                _p(deltas), _p(rays), _p(weights_sum), _p(depth), _p(latent_image), _p(decoder), _p(bg), N, ctx.T_thresh,
                _p(d_sigmas), _p(d_latents), _p(d_bg), _p(d_decoder), _stream())
        return d_sigmas, d_latents, None, None, d_decoder, None, d_bg


def composite_rays_train_decode(sigmas, latents, deltas, rays, decoder, T_thresh=1e-4, bg_color=None):
    """The RGB refinement stage's compositing: sigmas [M], latents [M,4], deltas [M,2], rays int32 [N,3], decoder [3,4]
    -> weights_sum [N], depth [N], image [N,3] = sum_k w_k (D z_k + 1) / 2 + (1 - weights_sum) * bg_color (RGB), and the
    composited latents latent_image [N,4] (no background; not differentiable).  sigmas, latents, decoder and bg_color
    receive gradients; the decoder's is the same bits on every run."""
    return _CompositeRaysTrainDecode.apply(sigmas, latents, deltas, rays, decoder, T_thresh, bg_color)


def decode_image(latent_image, weights_sum, decoder, bg_color=None):
    """latent_image [N,4], weights_sum [N], decoder [3,4] -> image [N,3] = (D L + ws) / 2 + (1 - ws) * bg_color: the
    epilogue of composite_rays_train_decode per pixel (lnerf_decode_image), for the inference loop.  Forward only."""
    latent_image = latent_image.contiguous()
    weights_sum = weights_sum.contiguous()
    decoder = decoder.detach().contiguous()
    N = latent_image.shape[0]
    if latent_image.shape[1] != 4 or tuple(decoder.shape) != (3, 4):
        raise ValueError("decode_image: latent_image must be [N,4] and the decoder [3,4]")
    bg = None if bg_color is None else bg_color.contiguous()
    image = torch.empty(N, 3, device=latent_image.device, dtype=torch.float32)
    _b.call("lnerf_decode_image", _chk(latent_image, "latent_image"), _chk(weights_sum, "weights_sum"),
            _chk(decoder, "decoder"), _chk(bg, "bg_color", allow_none=True), N, _p(image), _stream())
    return image


# ------------------------------------------------------------------------------ shaded renders
def fd_points(xyzs, bound, eps, m_host, m_dev=None, out=None):
    """The finite-difference stencil of the shaded renders (lnerf_fd_points): sample i < min(m_host, *m_dev) of xyzs
    [cap,3] -> rows 7 i .. 7 i + 6 of pts7 [7 cap, 3] (itself, then +x, -x, +y, -y, +z, -z at distance eps, clamped to
    [-bound, bound]) and the device counter m7_dev [1] = 7 m.  `out` = (pts7, m7_dev) of an earlier call re-uses its
    buffers.  -> (pts7, m7_dev); rows >= 7 m keep what they held."""
    _chk(xyzs, "xyzs")
    if xyzs.dim() != 2 or xyzs.shape[1] != 3:
        raise ValueError("fd_points: xyzs must be [cap,3]")
    cap, dev = xyzs.shape[0], xyzs.device
    if int(m_host) > cap:
        raise ValueError("fd_points: m_host %d exceeds the %d rows of xyzs" % (int(m_host), cap))
    if out is not None and out[0].shape[0] == 7 * cap and out[0].device == dev:
        pts7, m7 = out
        torch.autograd.graph.increment_version(pts7)   # rewritten through raw pointers (see march_rays_train)
        torch.autograd.graph.increment_version(m7)
    else:
        pts7 = torch.empty(7 * cap, 3, device=dev, dtype=torch.float32)
        # (the launch writes the counter; with no work there is no launch)
        m7 = (torch.empty if int(m_host) > 0 else torch.zeros)(1, device=dev, dtype=torch.int32)
    _b.call("lnerf_fd_points", _p(xyzs), float(bound), float(eps), int(m_host),
            _chk(m_dev, "m_dev", torch.int32, allow_none=True), _p(pts7), _p(m7), _stream())
    return pts7, m7


def shade_record(light_d, ambient_ratio, textureless, n_views, device):
    """The per-view record shade_fd reads, f32 [n_views, 5] = (l_x, l_y, l_z, ambient, textureless 0 / 1) on `device`.
    light_d: [3] (every view) or [n_views, 3], the direction toward the light (list or tensor; normalised here, in
    f32) -- or a record [n_views, 5] already, which is returned as it is (ambient_ratio and textureless are then its own)."""
    n_views = int(n_views)
    t = light_d if torch.is_tensor(light_d) else torch.tensor(light_d, dtype=torch.float32)
    if t.dim() == 2 and t.shape[1] == 5:
        if t.shape[0] != n_views or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError("a shade record must be f32 [%d, 5] on the GPU (got %s %s on %s)"
                             % (n_views, t.dtype, tuple(t.shape), t.device))
        return t.contiguous()
    t = t.detach().to(torch.float32).reshape(-1, 3)
    if t.shape[0] not in (1, n_views):
        raise ValueError("light_d must be [3] or [%d, 3] (got %s)" % (n_views, tuple(t.shape)))
    t = t.cpu()
    t = (t / t.norm(dim=-1, keepdim=True)).expand(n_views, 3)
    rec = torch.cat([t, torch.full((n_views, 1), float(ambient_ratio)),
                     torch.full((n_views, 1), 1.0 if textureless else 0.0)], -1)
    return rec.to(device).contiguous()


class _ShadeFD(torch.autograd.Function):
    """lnerf_shade_fd_forward / _backward; with `orient` (shade_fd's tuple, or None) lnerf_shade_fd_orient_*, which return
    the term as a third output: one forward launch, one backward launch either way."""

    @staticmethod
    def forward(ctx, sigmas7, rgbs7, rays, shade, rays_per_view, eps, orient):
        sigmas7 = sigmas7.contiguous()
        rgbs7 = rgbs7.contiguous()
        shade = shade.contiguous()
        if sigmas7.shape[0] % 7 != 0 or rgbs7.shape[0] != sigmas7.shape[0]:
            raise ValueError("shade_fd: sigmas7 [7 cap] and rgbs7 [7 cap, C] must hold seven rows per sample")
        if shade.dim() != 2 or shade.shape[1] != 5:
            raise ValueError("shade_fd: shade must be [B,5] = (l_x, l_y, l_z, ambient, textureless)")
        cap, C, N, B = sigmas7.shape[0] // 7, rgbs7.shape[1], rays.shape[0], shade.shape[0]
        if orient is not None:
            deltas, rays_d, density_scale, T_thresh, n_ids = orient
            n_ids = int(n_ids)
            if deltas.dim() != 2 or deltas.shape[1] != 2 or deltas.shape[0] < cap:
                raise ValueError("shade_fd: orient needs the march's deltas [>= cap, 2] (got %s for cap %d)"
                                 % (tuple(deltas.shape), cap))
            if rays_d.dim() != 2 or rays_d.shape[1] != 3 or rays_d.shape[0] != n_ids or N > n_ids:
                raise ValueError("shade_fd: orient needs rays_d [n_ids, 3] with n_ids = %d >= the %d rays (got %s)"
                                 % (n_ids, N, tuple(rays_d.shape)))
        dev = sigmas7.device
        inv_2eps = 1.0 / (2.0 * float(eps))
        # (rows outside every ray's span are not written, as with the field's own outputs: no fill launch in the step)
        sigma_c = torch.empty(cap, device=dev, dtype=torch.float32)
        colours = torch.empty(cap, C, device=dev, dtype=torch.float32)
        args = (_chk(sigmas7, "sigmas7"), _chk(rgbs7, "rgbs7"), C, _chk(rays, "rays", torch.int32), N, int(rays_per_view),
                _chk(shade, "shade"), B, inv_2eps)
        ctx.set_materialize_grads(False)
        if orient is None:
            _b.call("lnerf_shade_fd_forward", *args, _p(sigma_c), _p(colours), _stream())
            ctx.save_for_backward(sigmas7, rgbs7, rays, shade)
            ctx.meta = (int(rays_per_view), inv_2eps)
            return sigma_c, colours
        # every ray of the table writes its own element (0 for an empty span); with fewer rays than ids the rest is 0
        orient_ray = (torch.empty if N == n_ids else torch.zeros)(n_ids, device=dev, dtype=torch.float32)
        _b.call("lnerf_shade_fd_orient_forward", *args, _chk(deltas, "deltas"), _chk(rays_d, "rays_d"),
                float(density_scale), float(T_thresh), _p(sigma_c), _p(colours), _p(orient_ray), _stream())
        ctx.save_for_backward(sigmas7, rgbs7, rays, shade, deltas, rays_d)
        ctx.meta = (int(rays_per_view), inv_2eps, float(density_scale), float(T_thresh))
        return sigma_c, colours, orient_ray

    @staticmethod
    def backward(ctx, dsigma_c, dcolours, d_orient=None):
        sigmas7, rgbs7, rays, shade, *orient = ctx.saved_tensors
        rays_per_view, inv_2eps, *orient_meta = ctx.meta
        cap, C, N, B = sigmas7.shape[0] // 7, rgbs7.shape[1], rays.shape[0], shade.shape[0]
        dsigma_c = torch.zeros(cap, device=sigmas7.device) if dsigma_c is None else dsigma_c.contiguous()
        dcolours = torch.zeros(cap, C, device=sigmas7.device) if dcolours is None else dcolours.contiguous()
        # every row below 7 m lies in a ray's span and is written by the kernel; the rows above are read by nobody
        dsigmas7 = torch.empty_like(sigmas7)
        drgbs7 = torch.empty_like(rgbs7)
        args = (_p(sigmas7), _p(rgbs7), C, _p(rays), N, rays_per_view, _p(shade), B, inv_2eps,
                _chk(dsigma_c, "dsigma_c"), _chk(dcolours, "dcolours"))
        if orient:
            deltas, rays_d = orient
            d_orient = None if d_orient is None else d_orient.contiguous()   # (None: the library runs the plain backward)
            _b.call("lnerf_shade_fd_orient_backward", *args, _p(deltas), _p(rays_d), *orient_meta,
                    _chk(d_orient, "d_orient", allow_none=True), _p(dsigmas7), _p(drgbs7), _stream())
        else:
            _b.call("lnerf_shade_fd_backward", *args, _p(dsigmas7), _p(drgbs7), _stream())
        return (dsigmas7, drgbs7) + (None,) * 5


def shade_fd(sigmas7, rgbs7, rays, shade, rays_per_view, eps, orient=None):
    """Lambertian / textureless shading from the finite-difference normal (lnerf_shade_fd_forward / _backward, contract in
    include/lnerf_hip.h): sigmas7 [7 cap] (unscaled densities), rgbs7 [7 cap, C] of the field at fd_points' rows, rays
    int32 [N,3] = (id, offset, count), shade f32 [B,5] = (unit light direction, ambient, textureless 0 / 1) per view, the
    view of ray id being id // rays_per_view -> sigma_c [cap] (row 7 i), colours [cap, C] (albedo x lam, or lam alone).
    sigmas7 and rgbs7 receive gradients; there is no CPU path.
    orient = (deltas [cap,2], rays_d [n_ids,3], density_scale, T_thresh, n_ids): the orientation regulariser rides along
    (lnerf_shade_fd_orient_forward / _backward, ONE node, one launch each way) -> (sigma_c, colours, orient_ray [n_ids]),
    orient_ray[id] = sum_i w_i max(0, n_i . v)^2 with the compositing weights w (detached: its gradient reaches sigmas7
    through the normal alone) and v the unit direction of ray id; sigma_c and colours are the plain call's bits."""
    return _ShadeFD.apply(sigmas7, rgbs7, rays, shade, rays_per_view, eps, orient)


# ------------------------------------------------------------------------------ distortion loss
class _DistortionLoss(torch.autograd.Function):
    """lnerf_distortion_forward / _backward: one launch each way."""

    @staticmethod
    def forward(ctx, sigmas, deltas, rays, T_thresh, n_ids):
        sigmas = sigmas.contiguous()
        N, dev = rays.shape[0], sigmas.device
        if deltas.dim() != 2 or deltas.shape[1] != 2 or deltas.shape[0] < sigmas.shape[0]:
            raise ValueError("distortion_loss: deltas must be the march's [>= %d, 2] (got %s)"
                             % (sigmas.shape[0], tuple(deltas.shape)))
        if N > n_ids:
            raise ValueError("distortion_loss: n_ids = %d is less than the %d rays" % (n_ids, N))
        # every ray of the table writes its own element (0 for an empty span); with fewer rays than ids the rest is 0
        loss = (torch.empty if N == n_ids else torch.zeros)(n_ids, device=dev, dtype=torch.float32)
        ray_sums = torch.empty(n_ids, 2, device=dev, dtype=torch.float32)     # (read back by the rays that wrote them)
        _b.call("lnerf_distortion_forward", _chk(sigmas, "sigmas"), _chk(deltas, "deltas"),
                _chk(rays, "rays", torch.int32), N, float(T_thresh), _p(loss), _p(ray_sums), _stream())
        ctx.save_for_backward(sigmas, deltas, rays, loss, ray_sums)
        ctx.set_materialize_grads(False)
        ctx.T_thresh = float(T_thresh)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        if d_loss is None:
            return None, None, None, None, None
        sigmas, deltas, rays, loss, ray_sums = ctx.saved_tensors
        d_loss = d_loss.contiguous()
        # every row below the march's counter lies in a ray's span and is written; the rows above are read by nobody
        dsigmas = torch.empty_like(sigmas)
        _b.call("lnerf_distortion_backward", _p(sigmas), _p(deltas), _p(rays), rays.shape[0], ctx.T_thresh,
                _chk(d_loss, "d_loss"), _p(loss), _p(ray_sums), _p(dsigmas), _stream())
        return dsigmas, None, None, None, None


def distortion_loss(sigmas, deltas, rays, T_thresh=1e-4, n_ids=None):
    """The distortion loss of mip-NeRF 360 per ray (lnerf_distortion_forward / _backward, contract in include/lnerf_hip.h):
    sigmas [cap] (the densities the compositing gets, scaled already), deltas [cap,2] = (dt, t), rays int32 [N,3] =
    (id, offset, count) -> loss [n_ids] (n_ids defaults to N; ids of no ray hold 0),
    loss[id] = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i with the compositing weights w (NOT detached: sigmas
    receives the gradient) and the mid-points m = t + dt / 2, in world units of t.  One autograd node; there is no CPU path."""
    return _DistortionLoss.apply(sigmas, deltas, rays, T_thresh, rays.shape[0] if n_ids is None else int(n_ids))


# ------------------------------------------------------------------------------ composited normal image, 2D smoothness
class _NormalImage(torch.autograd.Function):
    """lnerf_normal_image_forward / _backward: one launch each way."""

    @staticmethod
    def forward(ctx, sigmas7, deltas, rays, n_ids, normal_eps, density_scale, T_thresh):
        sigmas7 = sigmas7.contiguous()
        N, dev = rays.shape[0], sigmas7.device
        if sigmas7.dim() != 1 or sigmas7.shape[0] % 7 != 0:
            raise ValueError("normal_image: sigmas7 [7 cap] must hold seven rows per sample (got %s)"
                             % (tuple(sigmas7.shape),))
        cap = sigmas7.shape[0] // 7
        if deltas.dim() != 2 or deltas.shape[1] != 2 or deltas.shape[0] < cap:
            raise ValueError("normal_image: deltas must be the march's [>= %d, 2] (got %s)" % (cap, tuple(deltas.shape)))
        if N > n_ids:
            raise ValueError("normal_image: n_ids = %d is less than the %d rays" % (n_ids, N))
        inv_2eps = 1.0 / (2.0 * float(normal_eps))
        # every ray of the table writes its own row (zeros for an empty span); with fewer rays than ids the rest is 0
        image = (torch.empty if N == n_ids else torch.zeros)(n_ids, 3, device=dev, dtype=torch.float32)
        _b.call("lnerf_normal_image_forward", _chk(sigmas7, "sigmas7"), _chk(deltas, "deltas"),
                _chk(rays, "rays", torch.int32), N, inv_2eps, float(density_scale), float(T_thresh), _p(image), _stream())
        ctx.save_for_backward(sigmas7, deltas, rays, image)
        ctx.set_materialize_grads(False)
        ctx.meta = (inv_2eps, float(density_scale), float(T_thresh))
        return image

    @staticmethod
    def backward(ctx, d_image):
        if d_image is None:
            return (None,) * 7
        sigmas7, deltas, rays, image = ctx.saved_tensors
        d_image = d_image.contiguous()
        # the kernel writes the seven rows of every span; the rows outside every span are zeros
        dsigmas7 = torch.zeros_like(sigmas7)
        _b.call("lnerf_normal_image_backward", _p(sigmas7), _p(deltas), _p(rays), rays.shape[0], *ctx.meta,
                _chk(d_image, "d_normal_image"), _p(image), _p(dsigmas7), _stream())
        return (dsigmas7,) + (None,) * 6


def normal_image(sigmas7, deltas, rays, n_ids=None, normal_eps=1e-2, density_scale=1.0, T_thresh=1e-4):
    """The composited normal of every ray (lnerf_normal_image_forward / _backward, contract in include/lnerf_hip.h):
    sigmas7 [7 cap] (the unscaled densities of the field at fd_points' rows: what shade_fd gets), deltas [cap,2] = (dt, t),
    rays int32 [N,3] = (id, offset, count) -> normal_image [n_ids, 3] (n_ids defaults to N; ids of no ray hold 0),
    normal_image[id] = sum_i w_i n_i with shade_fd's finite-difference normals n (distance normal_eps) and the compositing
    weights w on density_scale * sigma (NOT detached: sigmas7 receives the gradient through the weights and through the
    normals; rows outside every span get 0).  One autograd node; there is no CPU path."""
    return _NormalImage.apply(sigmas7, deltas, rays, rays.shape[0] if n_ids is None else int(n_ids), normal_eps,
                              density_scale, T_thresh)


class _ImageSmooth(torch.autograd.Function):
    """lnerf_image_smooth_forward / _backward: one launch each way."""

    @staticmethod
    def forward(ctx, img):
        if img.dim() != 4 or not 1 <= img.shape[3] <= 4:
            raise ValueError("image_smooth: img must be [B,H,W,C] with 1 <= C <= 4 (got %s)" % (tuple(img.shape),))
        img = img.contiguous()
        B, H, W, C = img.shape
        loss = torch.empty(B, H, W, 2, device=img.device, dtype=torch.float32)
        _b.call("lnerf_image_smooth_forward", _chk(img, "img"), B, H, W, C, _p(loss), _stream())
        ctx.save_for_backward(img)
        ctx.set_materialize_grads(False)
        return loss

    @staticmethod
    def backward(ctx, d_loss):
        if d_loss is None:
            return None
        img, = ctx.saved_tensors
        B, H, W, C = img.shape
        d_loss = d_loss.contiguous()
        d_img = torch.empty_like(img)          # (every element is written)
        _b.call("lnerf_image_smooth_backward", _p(img), B, H, W, C, _chk(d_loss, "d_loss"), _p(d_img), _stream())
        return d_img


def image_smooth(img):
    """Squared differences between neighbouring pixels (lnerf_image_smooth_forward / _backward, contract in
    include/lnerf_hip.h): img f32 [B,H,W,C], 1 <= C <= 4 -> loss [B,H,W,2], loss[b,y,x,0] = sum_c (img[b,y,x+1,c] -
    img[b,y,x,c])^2 (0 in the last column), loss[b,y,x,1] the same toward y + 1 (0 in the last row).  One autograd node;
    there is no CPU path."""
    return _ImageSmooth.apply(img)


# ------------------------------------------------------------------------------ mesh export
def marching_cubes(volume, iso, lo, hi, close_boundary=True):
    """Iso-surface of a dense f32 volume [nx, ny, nz] (z fastest) on the GPU (lnerf_marching_cubes, include/lnerf_hip.h).
    Lattice point (i, j, k) sits at lo + (hi - lo) * (i, j, k) / (n - 1); inside is value > iso.
    -> verts [V,3] f32, faces [F,3] int32 (normals from inside to outside), normals [V,3] f32, all on the device.
    One host synchronisation: a count pass sizes the outputs, the emit pass fills them from its scratch."""
    if not isinstance(volume, torch.Tensor) or volume.dim() != 3:
        raise ValueError("marching_cubes: volume must be a 3-d tensor [nx, ny, nz]")
    volume = volume.contiguous()
    _chk(volume, "volume")
    nx, ny, nz = (int(s) for s in volume.shape)
    lo = [float(v) for v in (lo.tolist() if isinstance(lo, torch.Tensor) else lo)]
    hi = [float(v) for v in (hi.tolist() if isinstance(hi, torch.Tensor) else hi)]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("marching_cubes: lo and hi take three coordinates each")
    flags = _b.MC_CLOSE_BOUNDARY if close_boundary else 0
    dev = volume.device
    nbytes = _b.get_lib().lnerf_marching_cubes_scratch_bytes(nx, ny, nz, flags)
    if nbytes == 0:
        raise ValueError("marching_cubes: lattice %d x %d x %d outside [2, 1024] per axis" % (nx, ny, nz))
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    args = (_p(volume), nx, ny, nz, float(iso), *lo, *hi)
    _b.call("lnerf_marching_cubes", *args, flags | _b.MC_COUNT_ONLY, _p(scratch), nbytes, None, None, 0, None, 0,
            _p(counts), _stream())
    V, F = (int(v) for v in counts.tolist())
    if V >= 2 ** 31:
        raise ValueError("marching_cubes: %d vertices do not fit int32 face indices" % V)
    verts = torch.empty(V, 3, device=dev, dtype=torch.float32)
    normals = torch.empty(V, 3, device=dev, dtype=torch.float32)
    faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
    if V > 0 or F > 0:
        _b.call("lnerf_marching_cubes", *args, flags | _b.MC_REUSE_COUNT, _p(scratch), nbytes, _p(verts), _p(normals), V,
                _p(faces), F, _p(counts), _stream())
    return verts, faces, normals


def _face_index(t, op, name, dev):
    """`t` as a contiguous int32 [F,3] index tensor on `dev`; `op` and `name` go into the messages."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
        raise ValueError("%s: %s must be a [F,3] index tensor" % (op, name))
    if t.dtype.is_floating_point:
        raise TypeError("%s: %s must hold integers" % (op, name))
    if t.dtype != torch.int32 and t.numel() and (int(t.min()) < -2 ** 31 or int(t.max()) >= 2 ** 31):
        raise ValueError("%s: %s has indices outside int32" % (op, name))   # (a wrapped index could be a valid one)
    return t.to(device=dev, dtype=torch.int32).contiguous()


def _mesh_inputs(verts, faces, op, max_faces, max_verts=None, order="%(V)d vertices / %(F)d faces"):
    """(verts contiguous f32 on the GPU, faces int32 [F,3] beside it, V, F) for the mesh ops; F <= max_faces and
    V <= max_verts (3 max_faces unless given), or ValueError with the counts in the op's `order`."""
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("%s: verts must be [V,3]" % op)
    faces = _face_index(faces, op, "faces", verts.device)
    verts = verts.contiguous()
    _chk(verts, "verts")
    V, F = int(verts.shape[0]), int(faces.shape[0])
    if F > max_faces or V > (3 * max_faces if max_verts is None else max_verts):
        raise ValueError("%s: %s out of range" % (op, order % dict(V=V, F=F)))
    return verts, faces, V, F


def _scratch(nbytes, dev):
    """`nbytes` of device scratch (never an empty tensor: its pointer would be NULL)."""
    return torch.empty(max(nbytes, 16), device=dev, dtype=torch.uint8)


def _settle_labels(entry, args, changed, max_rounds, op):
    """Label rounds (`entry`(*args, changed, stream)) until one changes nothing -> the number of rounds run."""
    rounds = 0
    while True:
        if rounds >= max_rounds:
            raise RuntimeError("%s: the labels have not settled after %d rounds" % (op, rounds))
        _b.call(entry, *args, _p(changed), _stream())
        rounds += 1
        if int(changed[0]) == 0:
            return rounds


def decimate_mesh(verts, faces, target_faces, max_error=float("inf"), max_rounds=_b.DECIMATE_DEFAULT_ROUNDS, stats=None):
    """Quadric-error decimation on the GPU (lnerf_decimate, include/lnerf_hip.h): rounds of independent edge collapses until
    at most `target_faces` faces are left -- target_faces or one fewer, unless a round finds no valid collapse, max_rounds
    runs out or `max_error` (a quadric-cost ceiling) blocks.  Open borders and non-manifold parts stay where they are.
    verts [V,3] f32, faces [F,3] (into verts), on the GPU -> verts [V',3] f32, faces [F',3] int32, normals [V',3] f32 on
    the device; the vertices still referenced and the faces left keep their order.  `stats` (a dict) receives rounds
    and collapses.  Synchronous: one host read of the counts per round."""
    target_faces, max_rounds, max_error = int(target_faces), int(max_rounds), float(max_error)
    if target_faces < 0 or max_rounds < 0:
        raise ValueError("decimate_mesh: target_faces (%d) and max_rounds (%d) must be >= 0" % (target_faces, max_rounds))
    if not max_error >= 0:
        raise ValueError("decimate_mesh: max_error must be >= 0 (inf: no ceiling)")
    verts, faces, V, F = _mesh_inputs(verts, faces, "decimate_mesh", _b.DECIMATE_MAX_FACES)
    dev = verts.device
    nbytes = _b.get_lib().lnerf_decimate_scratch_bytes(V, F)
    scratch = _scratch(nbytes, dev)
    counts = torch.zeros(4, device=dev, dtype=torch.int64)
    out_v = torch.empty(V, 3, device=dev, dtype=torch.float32)
    out_f = torch.empty(F, 3, device=dev, dtype=torch.int32)
    out_n = torch.empty(V, 3, device=dev, dtype=torch.float32)
    _b.call("lnerf_decimate", _p(verts), V, _p(faces), F, target_faces, max_error, max_rounds, _p(scratch), nbytes,
            _p(out_v), _p(out_f), _p(out_n), _p(counts), _stream())
    Vo, Fo, rounds, collapses = (int(c) for c in counts.tolist())
    if stats is not None:
        stats.update(rounds=rounds, collapses=collapses)
    return out_v[:Vo], out_f[:Fo], out_n[:Vo]


# ------------------------------------------------------------------------------ mesh cleaning
def mesh_components(verts, faces, stats=None):
    """Connected components of a mesh on the GPU (lnerf_mesh_components_*, include/lnerf_hip.h "mesh cleaning"): two
    vertices are connected iff a face holds both.  verts [V,3] f32, faces [F,3] (into verts), on the GPU ->
    dict(vert_comp [V] int32 (-1: in no face), face_comp [F] int32, comp_faces [C] int32, comp_box [C,6] f32 (x_lo, y_lo,
    z_lo, x_hi, y_hi, z_hi), components = C, referenced (vertices in a face), rounds); components are numbered by their
    smallest vertex.  A face indexing outside verts or a non-finite coordinate raises ValueError.  `stats` (a dict)
    receives the scalars.  Deterministic bit for bit.  Synchronous: one host read per label round."""
    verts, faces, V, F = _mesh_inputs(verts, faces, "mesh_components", _b.MESH_MAX_FACES)
    if V > 0 and not bool(torch.isfinite(verts).all()):
        raise ValueError("mesh_components: verts holds non-finite coordinates")
    dev = verts.device
    i32 = dict(device=dev, dtype=torch.int32)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    label = torch.empty(V, **i32)
    _b.call("lnerf_mesh_components_begin", _p(faces), V, F, _p(label), _p(counts), _stream())
    bad = int(counts[0])
    if bad:
        raise ValueError("mesh_components: %d faces index outside verts (%d)" % (bad, V))
    rounds = _settle_labels("lnerf_mesh_components_round", (_p(faces), V, F, _p(label)), torch.zeros(1, **i32),
                            _b.MESH_MAX_ROUNDS, "mesh_components")
    nbytes = _b.get_lib().lnerf_mesh_components_scratch_bytes(V, F)
    scratch = _scratch(nbytes, dev)
    cap = min(V, F)
    vert_comp, face_comp, comp_faces = torch.empty(V, **i32), torch.empty(F, **i32), torch.empty(cap, **i32)
    comp_box = torch.empty(cap, 6, device=dev, dtype=torch.float32)
    _b.call("lnerf_mesh_components_finish", _p(verts), V, _p(faces), F, _p(label), _p(scratch), nbytes, _p(vert_comp),
            _p(face_comp), _p(comp_faces), _p(comp_box), _p(counts), _stream())
    C, referenced = (int(c) for c in counts.tolist())
    if stats is not None:
        stats.update(components=C, referenced=referenced, rounds=rounds)
    return dict(vert_comp=vert_comp, face_comp=face_comp, comp_faces=comp_faces[:C], comp_box=comp_box[:C], components=C,
                referenced=referenced, rounds=rounds)


def mesh_filter(verts, faces, face_keep):
    """The faces with a non-zero flag and the vertices they reference, both in their old order (lnerf_mesh_filter).
    verts [V,3] f32, faces [F,3], face_keep [F] (bool / uint8), on the GPU -> verts [V',3], faces [F',3] int32
    (re-indexed), vert_src [V'] long with verts_out = verts[vert_src]: gather any per-vertex attribute through it."""
    verts, faces, V, F = _mesh_inputs(verts, faces, "mesh_filter", _b.MESH_MAX_FACES)
    if not isinstance(face_keep, torch.Tensor) or face_keep.shape != (F,) or face_keep.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mesh_filter: face_keep must be a bool / uint8 tensor [%d]" % F)
    dev = verts.device
    keep = face_keep.to(device=dev, dtype=torch.uint8).contiguous()
    nbytes = _b.get_lib().lnerf_mesh_filter_scratch_bytes(V, F)
    scratch = _scratch(nbytes, dev)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    faces_out = torch.empty(F, 3, device=dev, dtype=torch.int32)
    vert_src = torch.empty(V, device=dev, dtype=torch.int32)
    _b.call("lnerf_mesh_filter", _p(faces), V, F, _p(keep), _p(scratch), nbytes, _p(faces_out), _p(vert_src), _p(counts),
            _stream())
    Vo, Fo = (int(c) for c in counts.tolist())
    vert_src = vert_src[:Vo].long()
    return verts[vert_src], faces_out[:Fo], vert_src


def component_keep(comp_faces, comp_box, min_faces=0, min_diameter=0.0, keep_largest=0):
    """clean_mesh's keep rule (include/lnerf_hip.h "mesh cleaning"), on the host in f64: comp_faces [C], comp_box [C,6]
    numpy -> bool [C]."""
    import numpy as np
    n = np.asarray(comp_faces, np.int64)
    box = np.asarray(comp_box, np.float64).reshape(-1, 6)
    C = len(n)
    if C == 0:
        return np.zeros(0, bool)
    d = box[:, 3:] - box[:, :3]
    diag2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    D = box[:, 3:].max(0) - box[:, :3].min(0)
    diag2_mesh = (D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]
    md = float(min_diameter)
    ok = (n >= int(min_faces)) & (diag2 >= (md * md) * diag2_mesh)
    k = int(keep_largest)
    if k > 0:
        order = sorted(np.nonzero(ok)[0].tolist(), key=lambda c: (-int(n[c]), c))[:k]
        ok = np.zeros(C, bool)
        ok[order] = True
    return ok


def clean_mesh(verts, faces, min_faces=0, min_diameter=0.0, keep_largest=0, stats=None):
    """Drop the small connected components of a mesh on the GPU: a component stays iff it has at least `min_faces` faces
    and its bounding-box diagonal is at least `min_diameter` (a fraction in [0, 1]) of the whole mesh's; keep_largest =
    k > 0 then keeps only the k such components with the most faces.  The rule itself runs on the host from the
    components' boxes and counts (mesh_components); the compaction is lnerf_mesh_filter.
    -> verts [V',3] f32, faces [F',3] int32, vert_src [V'] long (verts' = verts[vert_src]); faces and vertices keep their
    order.  With everything at 0 only the vertices in no face go.  `stats` (a dict) receives components, kept, rounds,
    faces_before, faces_after."""
    min_faces, keep_largest, min_diameter = int(min_faces), int(keep_largest), float(min_diameter)
    if min_faces < 0 or keep_largest < 0:
        raise ValueError("clean_mesh: min_faces (%d) and keep_largest (%d) must be >= 0" % (min_faces, keep_largest))
    if not 0.0 <= min_diameter <= 1.0:
        raise ValueError("clean_mesh: min_diameter %r outside [0, 1]" % min_diameter)
    verts, faces, V, F = _mesh_inputs(verts, faces, "clean_mesh", _b.MESH_MAX_FACES)
    comp = mesh_components(verts, faces)
    ok = component_keep(comp["comp_faces"].cpu().numpy(), comp["comp_box"].cpu().numpy(), min_faces, min_diameter,
                        keep_largest)
    ok_dev = torch.as_tensor(ok, device=verts.device)
    keep = ok_dev[comp["face_comp"].long()] if F > 0 else torch.zeros(0, device=verts.device, dtype=torch.bool)
    out_v, out_f, vert_src = mesh_filter(verts, faces, keep)
    if stats is not None:
        stats.update(components=comp["components"], kept=int(ok.sum()), rounds=comp["rounds"], faces_before=F,
                     faces_after=int(out_f.shape[0]))
    return out_v, out_f, vert_src


def smooth_mesh(verts, faces, iterations=10, lam=_b.SMOOTH_LAMBDA, mu=_b.SMOOTH_MU):
    """Taubin smoothing on the GPU (lnerf_mesh_smooth): `iterations` times a step of weight `lam` towards the mean of the
    incident faces' other corners, then a step of weight `mu` (negative: it undoes the shrinkage; mu = 0 is plain
    Laplacian smoothing).  verts [V,3] f32, faces [F,3] (into verts), on the GPU -> verts [V,3] f32, normals [V,3] f32
    (area-weighted face sums of the result, as decimate_mesh's).  The connectivity does not change.  iterations = 0
    gives the vertices back with their normals.  Deterministic bit for bit."""
    iterations, lam, mu = int(iterations), float(lam), float(mu)
    if not 0 <= iterations <= _b.SMOOTH_MAX_ITER:
        raise ValueError("smooth_mesh: %d iterations outside [0, %d]" % (iterations, _b.SMOOTH_MAX_ITER))
    if not 0.0 < lam <= 1.0:
        raise ValueError("smooth_mesh: lam %r outside (0, 1]" % lam)
    if not -1.5 <= mu <= 0.0:
        raise ValueError("smooth_mesh: mu %r outside [-1.5, 0]" % mu)
    verts, faces, V, F = _mesh_inputs(verts, faces, "smooth_mesh", _b.MESH_MAX_FACES)
    dev = verts.device
    nbytes = _b.get_lib().lnerf_mesh_smooth_scratch_bytes(V, F)
    scratch = _scratch(nbytes, dev)
    out_v = torch.empty(V, 3, device=dev, dtype=torch.float32)
    out_n = torch.empty(V, 3, device=dev, dtype=torch.float32)
    try:
        _b.call("lnerf_mesh_smooth", _p(verts), V, _p(faces), F, iterations, lam, mu, _p(scratch), nbytes, _p(out_v),
                _p(out_n), _stream())
    except _b.LnerfError as e:
        if "index outside" in str(e):
            raise ValueError("smooth_mesh: %s" % e) from e
        raise
    return out_v, out_n


# ------------------------------------------------------------------------------ chart atlas
def _half_edge_twins(faces, V):
    """twin [3F] int32 of the half-edges 3 f + k = faces[f][k] -> faces[f][(k+1)%3]: the one half-edge the other way round
    when the undirected edge occurs in exactly two half-edges, one each way, and its ends differ; else -1."""
    F = faces.shape[0]
    a = faces.reshape(-1).long()
    b = faces[:, [1, 2, 0]].reshape(-1).long()
    key = torch.minimum(a, b) * max(V, 1) + torch.maximum(a, b)
    key, order = torch.sort(key, stable=True)
    _, counts = torch.unique_consecutive(key, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    first = start[counts == 2]
    e0, e1 = order[first], order[first + 1]
    ok = ((a[e0] < b[e0]) != (a[e1] < b[e1])) & (a[e0] != b[e0])
    e0, e1 = e0[ok], e1[ok]
    twin = torch.full((3 * F,), -1, device=faces.device, dtype=torch.int32)
    twin[e0] = e1.int()
    twin[e1] = e0.int()
    return twin


def chart_atlas(verts, faces, resolution, pad=2, stats=None):
    """Chart UV atlas of a mesh on the GPU (lnerf_atlas_*, include/lnerf_hip.h "chart atlas"): faces bucketed by the axis
    nearest their normal, connected same-bucket patches projected along it, their boxes shelf-packed into the square at
    one scale, and faces that fold over their own chart evicted into charts of their own.
    verts [V,3] f32, faces [F,3] (into verts), on the GPU -> vt [n_vt,2] f32 (one row per (chart, vertex) pair), ft [F,3]
    long, and a dict: face_chart [F] int32, chart_rect [C,4] int32 (ox, oy, w, h in texels), chart_axis [C] int32, scale,
    k, evicted (count), evicted_faces [E] long, rounds.  `stats` (a dict) receives the scalars.  Deterministic bit
    for bit.  Synchronous: one host read per label round and a few around the packing, which is host code."""
    import numpy as np
    from ...uv_atlas import ATLAS_MAX_SHRINKS, atlas_pack_error, chart_rect_sizes, pack_charts, shelf_pack
    R, pad = int(resolution), int(pad)
    if not 1 <= R <= _b.UV_MAX_RES:
        raise ValueError("chart_atlas: resolution %d outside [1, %d]" % (R, _b.UV_MAX_RES))
    if pad < 0 or 2 * pad + 2 > R:
        raise ValueError("chart_atlas: pad %d needs 2 pad + 2 <= resolution (%d)" % (pad, R))
    verts, faces, V, F = _mesh_inputs(verts, faces, "chart_atlas", _b.ATLAS_MAX_FACES, max_verts=2 ** 31 - 1,
                                      order="%(F)d faces / %(V)d vertices")
    dev = verts.device
    lib = _b.get_lib()
    i32 = dict(device=dev, dtype=torch.int32)
    counts = torch.zeros(1, device=dev, dtype=torch.int64)
    bucket, label = torch.empty(F, **i32), torch.empty(F, **i32)
    _b.call("lnerf_atlas_buckets", _p(verts), V, _p(faces), F, _p(bucket), _p(label), _p(counts), _stream())
    bad = int(counts[0])
    if bad:
        raise ValueError("chart_atlas: %d faces index outside verts (%d)" % (bad, V))
    # charts: rounds of hook + pointer jumping until a round changes nothing
    twin = _half_edge_twins(faces, V)
    rounds = _settle_labels("lnerf_atlas_round", (_p(bucket), _p(twin), F, _p(label)), torch.zeros(1, **i32),
                            _b.ATLAS_MAX_ROUNDS, "chart_atlas")
    nbytes = lib.lnerf_atlas_compact_scratch_bytes(F)
    scratch = _scratch(nbytes, dev)
    face_chart, chart_axis = torch.empty(F, **i32), torch.empty(F, **i32)
    _b.call("lnerf_atlas_compact", _p(bucket), _p(label), F, _p(scratch), nbytes, _p(face_chart), _p(chart_axis),
            _p(counts), _stream())
    C = int(counts[0])
    chart_axis = chart_axis[:C].clone()

    def boxes(fc, n, sub=None):
        f, b = (faces, bucket) if sub is None else (faces[sub].contiguous(), bucket[sub].contiguous())
        nb = lib.lnerf_atlas_boxes_scratch_bytes(n)
        sc = _scratch(nb, dev)
        out = torch.empty(n, 4, device=dev, dtype=torch.float32)
        _b.call("lnerf_atlas_boxes", _p(verts), V, _p(f), _p(b), _p(fc), int(f.shape[0]), n, _p(sc), nb, _p(out), _stream())
        return out

    def emit(fc, axis, rect, box, s):
        """vt, ft (int32) of the layout: texture vertices = the distinct (chart, vertex) pairs, ascending."""
        key = (fc.long()[:, None] * max(V, 1) + faces.long()).reshape(-1)
        uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
        ft = inv.reshape(F, 3).int().contiguous()
        vt = torch.zeros(int(uniq.shape[0]), 2, device=dev, dtype=torch.float32)
        org = torch.as_tensor(rect[:, :2].astype("int32"), device=dev).contiguous()
        _b.call("lnerf_atlas_uv", _p(verts), V, _p(faces), _p(ft), F, _p(fc), _p(axis), _p(org), _p(box), int(axis.shape[0]),
                pad, s, R, _p(vt), int(vt.shape[0]), _stream())
        return vt, ft

    def folded(vt, ft):
        """evicted [F] bool: faces that strictly cover a texel centre a face with a larger index covers too."""
        nb = lib.lnerf_atlas_fold_scratch_bytes(F, R)
        sc = _scratch(nb, dev)
        owner = torch.empty(R * R, **i32)
        ev = torch.zeros(F, **i32)
        args = (_p(vt), int(vt.shape[0]), _p(ft), F, R)
        _b.call("lnerf_atlas_fold", *args, _b.UV_ITEMS, 0, _p(sc), nb, None, None, _p(counts), _stream())
        _b.call("lnerf_atlas_fold", *args, _b.UV_COVER, int(counts[0]), _p(sc), nb, _p(owner), _p(ev), _p(counts), _stream())
        return ev != 0

    box = boxes(face_chart, C)
    box_np = box.cpu().numpy()
    k = 0
    while True:
        k, s, rect, state = pack_charts(box_np, R, pad, k)
        vt, ft = emit(face_chart, chart_axis, rect, box, s)
        ev = folded(vt, ft) if F > 0 else torch.zeros(0, device=dev, dtype=torch.bool)
        ev_faces = torch.nonzero(ev).reshape(-1)
        E = int(ev_faces.shape[0])
        fc, axis = face_chart, chart_axis
        if E > 0:
            # every evicted face becomes a chart of its own, numbered after the others in face order
            ev_box = boxes(torch.arange(E, **i32), E, ev_faces)
            eb = ev_box.cpu().numpy().astype("float64")
            w, h = chart_rect_sizes(eb[:, 1] - eb[:, 0], eb[:, 3] - eb[:, 2], s, pad)
            placed = shelf_pack(w, h, R, state)
            if placed is None:
                k += 1
                if k > ATLAS_MAX_SHRINKS:
                    raise atlas_pack_error(R, C + E, pad)
                continue
            rect = np.concatenate([rect, np.stack([placed[0], placed[1], w, h], 1)], 0)
            fc = face_chart.clone()
            fc[ev_faces] = torch.arange(C, C + E, **i32)
            axis = torch.cat([chart_axis, bucket[ev_faces]])
            vt, ft = emit(fc, axis, rect, torch.cat([box, ev_box]).contiguous(), s)
        break
    info = dict(face_chart=fc, chart_rect=torch.as_tensor(rect.astype("int32"), device=dev).reshape(-1, 4), chart_axis=axis,
                scale=s, k=k, evicted=E, evicted_faces=ev_faces, rounds=rounds)
    if stats is not None:
        stats.update(scale=s, k=k, evicted=E, rounds=rounds, charts=int(axis.shape[0]))
    return vt, ft.long(), info


# ------------------------------------------------------------------------------ texture baking
def uv_raster(verts, faces, vt, ft, R):
    """Which texel of an R x R texture each face of a UV-mapped mesh covers (lnerf_uv_raster, include/lnerf_hip.h).
    verts [V,3], faces [F,3] (into verts), vt [T,2], ft [F,3] (into vt), all on the GPU.
    -> texel_face [R,R] int32 (covering face with the largest index, -1 = none), texel_idx [P] int32 (the covered
    texels' linear indices i * R + j, ascending) and pos [P,3] f32 (the surface point at each covered texel's centre).
    Texel (i, j) has its centre at u = (j + 0.5) / R, v = 1 - (i + 0.5) / R, the convention texture_map samples with.
    Two host synchronisations: the candidate count sizes the cover launch, the covered count sizes the outputs."""
    R = int(R)
    if not 1 <= R <= _b.UV_MAX_RES:
        raise ValueError("uv_raster: resolution %d outside [1, %d]" % (R, _b.UV_MAX_RES))
    if not isinstance(verts, torch.Tensor) or verts.dim() != 2 or verts.shape[1] != 3:
        raise ValueError("uv_raster: verts must be [V,3]")
    if not isinstance(vt, torch.Tensor) or vt.dim() != 2 or vt.shape[1] != 2:
        raise ValueError("uv_raster: vt must be [T,2]")
    dev = verts.device
    verts = verts.to(torch.float32).contiguous()
    vt = vt.to(device=dev, dtype=torch.float32).contiguous()
    faces, ft = _face_index(faces, "uv_raster", "faces", dev), _face_index(ft, "uv_raster", "ft", dev)
    if faces.shape[0] != ft.shape[0]:
        raise ValueError("uv_raster: faces has %d rows, ft %d" % (faces.shape[0], ft.shape[0]))
    _chk(verts, "verts")
    _chk(vt, "vt")
    F, V, T = faces.shape[0], verts.shape[0], vt.shape[0]
    if max(F, V, T) >= 2 ** 31:
        raise ValueError("uv_raster: %d faces / %d vertices / %d texture vertices exceed int32" % (F, V, T))
    nbytes = _b.get_lib().lnerf_uv_raster_scratch_bytes(F, R)
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    counts = torch.zeros(3, device=dev, dtype=torch.int64)
    texel_face = torch.empty(R, R, device=dev, dtype=torch.int32)
    mesh = (_p(verts), V, _p(faces), _p(vt), T, _p(ft), F, R)
    _b.call("lnerf_uv_raster", *mesh, _b.UV_ITEMS, 0, _p(scratch), nbytes, None, None, None, 0, _p(counts), _stream())
    items, bad = (int(v) for v in counts[:2].tolist())
    if bad:
        raise ValueError("uv_raster: %d faces index outside verts (%d) or vt (%d)" % (bad, V, T))
    _b.call("lnerf_uv_raster", *mesh, _b.UV_COVER, items, _p(scratch), nbytes, _p(texel_face), None, None, 0,
            _p(counts), _stream())
    P = int(counts[2])
    texel_idx = torch.empty(P, device=dev, dtype=torch.int32)
    pos = torch.empty(P, 3, device=dev, dtype=torch.float32)
    if P > 0:
        _b.call("lnerf_uv_raster", *mesh, _b.UV_EMIT, 0, _p(scratch), nbytes, _p(texel_face), _p(texel_idx), _p(pos),
                P, _p(counts), _stream())
    return texel_face, texel_idx, pos


def uv_dilate(texture, mask, passes):
    """`passes` gutter rounds, in place, over texture [C,R,R] f32 and mask [R,R] uint8 (2 covered, 1 filled, 0 empty)
    on the GPU (lnerf_uv_dilate): a texel that is empty before a round takes the mean of its 8-neighbours that were
    non-empty before it.  Returns (texture, mask)."""
    if not isinstance(texture, torch.Tensor) or texture.dim() != 3 or texture.shape[1] != texture.shape[2]:
        raise ValueError("uv_dilate: texture must be [C,R,R]")
    C, R = int(texture.shape[0]), int(texture.shape[1])
    if not isinstance(mask, torch.Tensor) or tuple(mask.shape) != (R, R):
        raise ValueError("uv_dilate: mask must be [R,R] = [%d,%d]" % (R, R))
    _chk(texture, "texture")
    _chk(mask, "mask", dtype=torch.uint8)
    passes = int(passes)
    if passes < 0:
        raise ValueError("uv_dilate: passes must be >= 0")
    if passes > 0:
        tmp, tmp_mask = torch.empty_like(texture), torch.empty_like(mask)
        _b.call("lnerf_uv_dilate", _p(texture), _p(mask), C, R, passes, _p(tmp), _p(tmp_mask), _stream())
    return texture, mask


# ------------------------------------------------------------------------------ texture pyramids, plain and weighted
def mip_levels(R, max_mip_level=-1):
    """Levels 1..L of an R x R texture: L_full = the trailing zero bits of R (a level's side may be odd only at the last
    level), capped by `max_mip_level` when that is >= 0.  R = 1 or odd R gives 0: plain bilinear."""
    R = int(R)
    full = (R & -R).bit_length() - 1 if R > 0 else 0
    return full if max_mip_level < 0 else min(int(max_mip_level), full)


def mip_texels(R, L):
    """Texels per channel of the packed levels 1..L."""
    return sum((R >> l) ** 2 for l in range(1, L + 1))


def _pyramid_shape(op, texture, weight, L):
    """(R, L) of a call on texture [C,R,R] (None: the weights alone) and weight [R,R] (None: the plain pyramid)."""
    square = lambda t, dim: isinstance(t, torch.Tensor) and t.dim() == dim and t.shape[-2] == t.shape[-1]
    if weight is not None and not square(weight, 2):
        raise ValueError("%s: weight must be [R,R]" % op)
    if texture is not None and not (square(texture, 3) and (weight is None or texture.shape[-1] == weight.shape[-1])):
        raise ValueError("%s: texture must be [C,R,R]" % op
                         + ("" if weight is None else " with the weight's R = %d" % weight.shape[-1]))
    R = int((texture if weight is None else weight).shape[-1])
    L = mip_levels(R) if L is None else int(L)
    if L < 0 or L > mip_levels(R):
        raise ValueError("%s: L = %d outside [0, %d], the levels a side of %d allows" % (op, L, mip_levels(R), R))
    return R, L


def pyramid_build(texture, L=None, weight=None, wpyr=None):
    """texture [C,R,R] -> levels 1..L packed [C,S] (None when L = 0; L = None: every level the side allows): the 2 x 2
    box averages (lnerf_mip_build) or, given weight [R,R] and its levels wpyr [S], the coverage-weighted means
    (lnerf_mipcov_pull)."""
    R, L = _pyramid_shape("mip_build" if weight is None else "mipcov_pull", texture, weight, L)
    if L == 0:
        return None
    C = int(texture.shape[0])
    pyr = torch.empty(C, mip_texels(R, L), device=texture.device)
    if weight is None:
        _b.call("lnerf_mip_build", _chk(texture, "texture"), C, R, L, _p(pyr), _stream())
    else:
        _b.call("lnerf_mipcov_pull", _chk(texture, "texture"), _chk(weight, "weight"), _chk(wpyr, "wpyr"), C, R, L,
                _p(pyr), _stream())
    return pyr


def pyramid_fold(dpyr, dtexture, L=None, weight=None, wpyr=None):
    """The transpose of pyramid_build: folds the gradient pyramid dpyr [C,S] (which it changes) into dtexture [C,R,R],
    which it adds to (lnerf_mip_build_backward, or lnerf_mipcov_pull_backward given the weights).  Returns dtexture."""
    R, L = _pyramid_shape("mip_build_backward" if weight is None else "mipcov_pull_backward", dtexture, weight, L)
    C = int(dtexture.shape[0])
    if weight is None:
        _b.call("lnerf_mip_build_backward", _chk(dpyr, "dpyr", allow_none=L == 0), C, R, L, _chk(dtexture, "dtexture"),
                _stream())
    else:
        _b.call("lnerf_mipcov_pull_backward", _chk(dpyr, "dpyr", allow_none=L == 0), _chk(weight, "weight"),
                _chk(wpyr, "wpyr", allow_none=L == 0), C, R, L, _chk(dtexture, "dtexture"), _stream())
    return dtexture


def mip_build(tex, L):
    """tex [C,R,R] -> levels 1..L packed [C,S] (None when L = 0)."""
    return pyramid_build(tex, L)


def mipcov_weights(weight, L=None):
    """weight [R,R] f32 in [0,1] -> the weights of levels 1..L packed [S] (lnerf_mipcov_weights; None when L = 0).
    L = None: every level the side allows."""
    R, L = _pyramid_shape("mipcov_weights", None, weight, L)
    if L == 0:
        return None
    wpyr = torch.empty(mip_texels(R, L), device=weight.device)
    _b.call("lnerf_mipcov_weights", _chk(weight, "weight"), R, L, _p(wpyr), _stream())
    return wpyr


def mipcov_pull(texture, weight, wpyr, L=None):
    """texture [C,R,R] -> the coverage-weighted means of levels 1..L packed [C,S] (None when L = 0)."""
    return pyramid_build(texture, L, weight, wpyr)


def mipcov_pull_backward(dpyr, weight, wpyr, dtexture, L=None):
    """Folds dpyr [C,S] (which it changes) into dtexture [C,R,R], which it adds to and returns."""
    return pyramid_fold(dpyr, dtexture, L, weight, wpyr)


def mipcov_push(texture, weight, wpyr, pyr, L=None):
    """The push of the pull-push fill, in place over texture [C,R,R] and the pulled pyr [C,S] (lnerf_mipcov_push).
    -> (texture, filled [R,R] uint8: 1 where a texel with weight != 1 was given a value)."""
    R, L = _pyramid_shape("mipcov_push", texture, weight, L)
    filled = torch.empty(R, R, device=texture.device, dtype=torch.uint8)
    _b.call("lnerf_mipcov_push", _chk(texture, "texture"), _chk(weight, "weight"), _chk(wpyr, "wpyr", allow_none=L == 0),
            _chk(pyr, "pyr", allow_none=L == 0), int(texture.shape[0]), R, L, _p(filled), _stream())
    return texture, filled


def pull_push_fill(texture, weight):
    """Fill the texels of texture [C,R,R] that `weight` [R,R] (f32 in [0,1]; 1 = known) does not cover from the ones it
    does: the coverage-weighted pyramid pulled up to a single texel and pushed back down (include/lnerf_hip.h), so that
    one known texel anywhere fills the whole texture.  A side that is not a power of two is padded to the next one with
    weight 0 for the fill and cropped again: the padding adds no value, it only lets the pyramid reach one texel.
    Texels of weight 1 keep their bits.  -> (a new filled texture, filled [R,R] uint8)."""
    R, _ = _pyramid_shape("pull_push_fill", texture, weight, None)
    side = 1 << max(R - 1, 0).bit_length()
    weight = weight.to(torch.float32)
    out = texture.to(torch.float32)
    if side != R:
        weight = torch.nn.functional.pad(weight, (0, side - R, 0, side - R))
        out = torch.nn.functional.pad(out, (0, side - R, 0, side - R))
    weight, out = weight.contiguous(), out.clone().contiguous()
    wpyr = mipcov_weights(weight)
    out, filled = mipcov_push(out, weight, wpyr, mipcov_pull(out, weight, wpyr))
    if side != R:
        out, filled = out[:, :R, :R].contiguous(), filled[:R, :R].contiguous()
    return out, filled


# ------------------------------------------------------------------------------ view projection
GOLDEN_ANGLE = math.pi * (3.0 - math.sqrt(5.0))


def bake_view_poses(K, theta_range=(math.radians(15.0), math.radians(150.0))):
    """K view directions for a view bake: a spherical Fibonacci lattice restricted to the polar band `theta_range`
    (radians from +y, the convention of pose_from_angles and Latent-Paint's Renderer).  The polar cosine is stratified
    over the band -- view k sits at the mid-point of the k-th of K equal strata, so the views share the band's area
    evenly -- and the azimuth is k x the golden angle.  -> [(theta, phi)] * K, host floats; deterministic."""
    K = int(K)
    t0, t1 = float(theta_range[0]), float(theta_range[1])
    if K < 1:
        raise ValueError("bake_view_poses: K must be >= 1 (got %d)" % K)
    if not 0.0 <= t0 <= t1 <= math.pi:
        raise ValueError("bake_view_poses: theta_range %r is not an interval of [0, pi]" % (theta_range,))
    c0, c1 = math.cos(t0), math.cos(t1)
    poses = []
    for k in range(K):
        c = c0 + (k + 0.5) / K * (c1 - c0)
        poses.append((math.acos(max(-1.0, min(1.0, c))), (k * GOLDEN_ANGLE) % (2.0 * math.pi)))
    return poses


def nerf_camera_record(c2w, fx, fy, cx, cy, H, W):
    """The NeRF camera (camera-to-world `c2w` [4,4] with the columns right, down, forward, eye of lnerf_get_rays, and
    pixel intrinsics) as the rasteriser's 14-float record (rotation rows, eye, fx, fy; camera z negative in front): the
    rows are right, -down, -forward and the focal lengths 2 fx / W, 2 fy / H, so the centre of pixel (row i, column j)
    of get_rays lands on the rasteriser's pixel (i, j).  The record has no principal point: cx = W / 2 and cy = H / 2
    (what intrinsics_from_fov gives) or ValueError.  -> list of 14 floats."""
    m = c2w.detach().cpu().double().tolist() if isinstance(c2w, torch.Tensor) else [[float(v) for v in r] for r in c2w]
    if len(m) < 3 or any(len(r) != 4 for r in m[:3]):
        raise ValueError("nerf_camera_record: c2w must be [4,4] (or [3,4])")
    H, W = int(H), int(W)
    if abs(float(cx) - W / 2.0) > 1e-6 * W or abs(float(cy) - H / 2.0) > 1e-6 * H:
        raise ValueError("nerf_camera_record: the rasteriser's camera has its principal point at the image centre "
                         "(%g, %g), not (%g, %g)" % (W / 2.0, H / 2.0, cx, cy))
    right, down, fwd, eye = ([m[r][c] for r in range(3)] for c in range(4))
    return right + [-v for v in down] + [-v for v in fwd] + eye + [2.0 * float(fx) / W, 2.0 * float(fy) / H]


def _cams(cams, op, dev):
    if not isinstance(cams, torch.Tensor) or cams.dim() != 2 or cams.shape[1] != 14 or cams.shape[0] < 1:
        raise ValueError("%s: cams must be [K,14] with K >= 1" % op)
    cams = cams.to(device=dev, dtype=torch.float32).contiguous()
    _chk(cams, "cams")
    return cams


class RasterState(typing.NamedTuple):
    """B views of one mesh, rasterised: per pixel the winning face (-1: background) and its barycentrics; the projected faces."""
    face_idx: torch.Tensor   # [B*H*W] int32
    bary: torch.Tensor       # [B*H*W,3]
    B: int
    H: int
    W: int
    face_xy: torch.Tensor    # [B,F,3,2]
    face_z: torch.Tensor     # [B,F,3]


def raster_project(verts, faces32, cams, H, W):
    """lnerf_raster_prepare_batch: verts [V,3], faces32 [F,3] int32, cams [B,14] -> (face_z, face_xy, face_box [B,F,4])."""
    B, F, dev = cams.shape[0], faces32.shape[0], verts.device
    face_z, face_xy = torch.empty(B, F, 3, device=dev), torch.empty(B, F, 3, 2, device=dev)
    face_box = torch.empty(B, F, 4, device=dev, dtype=torch.int16)
    _b.call("lnerf_raster_prepare_batch", _chk(verts, "verts"), verts.shape[0], _chk(faces32, "faces", torch.int32), F,
            _chk(cams, "cams"), B, H, W, _p(face_z), _p(face_xy), _p(face_box), _stream())
    return face_z, face_xy, face_box


def raster_cover(face_z, face_xy, face_box, H, W):
    """lnerf_rasterize_batch on raster_project's result -> (face_idx [B*H*W], bary [B*H*W,3])."""
    B, F = face_z.shape[0], face_z.shape[1]
    face_idx = torch.empty(B * H * W, device=face_z.device, dtype=torch.int32)
    bary = torch.empty(B * H * W, 3, device=face_z.device)
    _b.call("lnerf_rasterize_batch", B, H, W, _p(face_z), _p(face_xy), _p(face_box), F, _p(face_idx), _p(bary), _stream())
    return face_idx, bary


def rasterize_views(verts, faces32, cams, H, W, project=raster_project, cover=raster_cover):
    """The batched tile-culled rasteriser, both launches -> RasterState (`project`, `cover`: the steps as autograd nodes)."""
    face_z, face_xy, face_box = project(verts, faces32, cams, H, W)
    face_idx, bary = cover(face_z, face_xy, face_box, H, W)
    return RasterState(face_idx, bary, cams.shape[0], H, W, face_xy, face_z)


def view_zbuffer(verts, faces, cams, H, W, erode=0):
    """Camera z of the visible surface of a mesh at every pixel centre of K views -> zbuf [K,H,W] f32: the batched
    rasteriser (lnerf_raster_prepare_batch, lnerf_rasterize_batch) and, per view, its perspective-correct barycentrics
    over the corners' camera z (lnerf_interpolate_attributes).  Foreground is negative; background pixels hold +1, and
    with `erode` > 0 so does every pixel within `erode` pixels (Chebyshev distance) of a background pixel: a decoder
    that up-scales smears the background over about its factor.  cams: [K,14] records."""
    H, W, erode = int(H), int(W), int(erode)
    if erode < 0:
        raise ValueError("view_zbuffer: erode must be >= 0")
    verts, faces, _, _ = _mesh_inputs(verts, faces, "view_zbuffer", 2 ** 31 - 1)
    dev = verts.device
    cams = _cams(cams, "view_zbuffer", dev)
    K = cams.shape[0]
    st = rasterize_views(verts, faces, cams, H, W)
    face_idx, bary, face_z = st.face_idx.view(K, H * W), st.bary.view(K, H * W, 3), st.face_z
    zbuf = torch.empty(K, H * W, device=dev)
    for k in range(K):   # face indices are per view: one D = 1 interpolation over each view's own corner depths
        _b.call("lnerf_interpolate_attributes", _p(face_idx[k]), _p(bary[k]), _p(face_z[k]), H * W, 1, _p(zbuf[k]),
                _stream())
    bg = (face_idx < 0).view(K, 1, H, W)
    if erode > 0:
        bg = torch.nn.functional.max_pool2d(bg.float(), 2 * erode + 1, stride=1, padding=erode) > 0
    return torch.where(bg.view(K, H, W), torch.ones((), device=dev), zbuf.view(K, H, W)).contiguous()


def project_views(pos, nrm, cams, zbuf, images, cos_min=0.2, power=4.0, slack=2.0):
    """Colour surface points from K images of the surface (lnerf_uv_project_views, include/lnerf_hip.h: the rule).
    pos, nrm [P,3] (point, unit outward normal), cams [K,14], zbuf [K,H,W] (view_zbuffer), images [K,C,H,W], 1 <= C <= 4.
    A view counts for a point where the point faces it (cosine >= cos_min), projects with all four bilinear taps on
    foreground pixels and passes the depth test (`slack` pixel footprints of bias); its colour is weighted by
    cosine^power.  -> out [P,C] (the weighted mean, 0 where no view counted), weight [P], count [P] int32."""
    pos, nrm = _points("project_views", pos, nrm)
    dev = pos.device
    cams, zbuf, images, K, C, H, W = _view_stack("project_views", cams, zbuf, images, dev)
    P = pos.shape[0]
    out = torch.zeros(P, C, device=dev)
    weight = torch.zeros(P, device=dev)
    count = torch.zeros(P, device=dev, dtype=torch.int32)
    _b.call("lnerf_uv_project_views", _chk(pos, "pos") if P else None, _chk(nrm, "nrm") if P else None, P, _p(cams), K, H,
            W, _chk(zbuf, "zbuf"), _chk(images, "images"), C, float(cos_min), float(power), float(slack),
            _p(out) if P else None, _p(weight) if P else None, _p(count) if P else None, _stream())
    return out, weight, count


# ------------------------------------------------------------------------------ exposure matching, two-band blending
LOWPASS_MAX_R = 64      # LNERF_LOWPASS_MAX_R
STATS_MAX_K = 64        # LNERF_STATS_MAX_K


def gaussian_taps(sigma):
    """The 2r + 1 taps of view_lowpass: exp(-t^2 / (2 sigma^2)) for t = -r .. r in float64, normalised to sum 1,
    r = ceil(3 sigma); sigma = 0 is the identity (r = 0, one tap of 1).  -> list of host floats (float64)."""
    sigma = float(sigma)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError("gaussian_taps: sigma must be finite and >= 0 (got %r)" % (sigma,))
    r = int(math.ceil(3.0 * sigma))
    if r > LOWPASS_MAX_R:
        raise ValueError("gaussian_taps: sigma = %g needs r = %d taps a side, more than %d" % (sigma, r, LOWPASS_MAX_R))
    g = [math.exp(-(t * t) / (2.0 * sigma * sigma)) if sigma > 0 else 1.0 for t in range(-r, r + 1)]
    total = math.fsum(g)
    return [v / total for v in g]


def _view_stack(op, cams, zbuf, images, dev, name="images"):
    """The checks project_views makes of its image stack and z-buffer -> (cams, zbuf, images, K, C, H, W)."""
    cams = _cams(cams, op, dev)
    K = cams.shape[0]
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[0] != K or not 1 <= images.shape[1] <= 4:
        raise ValueError("%s: %s must be [K,C,H,W] with K = %d and 1 <= C <= 4" % (op, name, K))
    C, H, W = (int(v) for v in images.shape[1:])
    if not isinstance(zbuf, torch.Tensor) or tuple(zbuf.shape) != (K, H, W):
        raise ValueError("%s: zbuf must be [K,H,W] = [%d,%d,%d]" % (op, K, H, W))
    return cams, zbuf.to(dev).float().contiguous(), images.to(dev).float().contiguous(), K, C, H, W


def _points(op, pos, nrm):
    for t, name in ((pos, "pos"), (nrm, "nrm")):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != 3:
            raise ValueError("%s: %s must be [P,3]" % (op, name))
    if pos.shape != nrm.shape:
        raise ValueError("%s: pos %s and nrm %s differ" % (op, tuple(pos.shape), tuple(nrm.shape)))
    return pos.float().contiguous(), nrm.to(pos.device).float().contiguous()


def view_lowpass(images, zbuf, sigma):
    """Masked, normalised Gaussian low-pass of K view images (lnerf_view_lowpass, include/lnerf_hip.h: the rule).
    images [K,C,H,W], 1 <= C <= 4; zbuf [K,H,W] (view_zbuffer): a pixel is usable iff zbuf < 0; sigma in pixels, the
    taps those of gaussian_taps.  Unusable pixels are left out of every sum (a NaN there reaches nothing); a pixel
    with no usable pixel in reach gets 0.  -> low [K,C,H,W], written at every pixel."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4 or not 1 <= images.shape[1] <= 4 or images.shape[0] < 1:
        raise ValueError("view_lowpass: images must be [K,C,H,W] with K >= 1 and 1 <= C <= 4")
    K, C, H, W = (int(v) for v in images.shape)
    if not isinstance(zbuf, torch.Tensor) or tuple(zbuf.shape) != (K, H, W):
        raise ValueError("view_lowpass: zbuf must be [K,H,W] = [%d,%d,%d]" % (K, H, W))
    taps = gaussian_taps(sigma)
    r = len(taps) // 2
    dev = images.device
    images, zbuf = images.float().contiguous(), zbuf.to(dev).float().contiguous()
    nbytes = int(_b.get_lib().lnerf_view_lowpass_scratch_bytes(K, C, H, W))
    if nbytes == 0:
        raise ValueError("view_lowpass: [%d,%d,%d,%d] is out of range (K C H W must stay below 2^31)" % (K, C, H, W))
    scratch = _scratch(nbytes, dev)
    low = torch.empty_like(images)
    taps_host = (ctypes.c_float * len(taps))(*taps)
    _b.call("lnerf_view_lowpass", _chk(images, "images"), _chk(zbuf, "zbuf"), K, C, H, W, taps_host, r, _p(scratch), nbytes,
            _p(low), _stream())
    return low


def view_overlap_stats(pos, nrm, cams, zbuf, low, cos_min=0.2, slack=2.0):
    """For every ordered pair of views, the number of points both accept and the sum of what the first shows there
    (lnerf_view_overlap_stats, include/lnerf_hip.h: the rule): the input of view_bake.exposure_gains.  pos, nrm [P,3],
    cams [K,14] with K <= 64, zbuf [K,H,W], low [K,C,H,W] (view_lowpass; finite, |value| <= 64); a point accepts a view
    exactly where project_views does.  -> (N [K,K] int64, S [K,K,C] int64: sums of round(sample * 2^24)); integer sums,
    so two calls give the same bits."""
    pos, nrm = _points("view_overlap_stats", pos, nrm)
    dev = pos.device
    cams, zbuf, low, K, C, H, W = _view_stack("view_overlap_stats", cams, zbuf, low, dev, "low")
    if K > STATS_MAX_K:
        raise ValueError("view_overlap_stats: K = %d views, more than %d" % (K, STATS_MAX_K))
    P = pos.shape[0]
    N = torch.zeros(K, K, device=dev, dtype=torch.int64)
    S = torch.zeros(K, K, C, device=dev, dtype=torch.int64)
    _b.call("lnerf_view_overlap_stats", _chk(pos, "pos") if P else None, _chk(nrm, "nrm") if P else None, P, _p(cams), K, H,
            W, _chk(zbuf, "zbuf"), _chk(low, "low"), C, float(cos_min), float(slack), _p(N), _p(S), _stream())
    return N, S


def project_views_bands(pos, nrm, cams, zbuf, images, low, gains=None, cos_min=0.2, power=4.0, slack=2.0):
    """Two-band projection of K images onto surface points (lnerf_uv_project_views_bands, include/lnerf_hip.h: the rule).
    Arguments as project_views, plus low [K,C,H,W] (view_lowpass of the images) and gains [K,C] or None (per view and
    channel, applied to both bands; None multiplies nothing).  The low band of a point is the cosine^power-weighted mean
    of the accepted views' low bands; everything above it comes from the one accepted view with the largest weight.
    -> out [P,C], weight [P], count [P] int32 (both exactly project_views'), best [P] int32 (-1: no view)."""
    pos, nrm = _points("project_views_bands", pos, nrm)
    dev = pos.device
    cams, zbuf, images, K, C, H, W = _view_stack("project_views_bands", cams, zbuf, images, dev)
    if not isinstance(low, torch.Tensor) or tuple(low.shape) != (K, C, H, W):
        raise ValueError("project_views_bands: low must be [K,C,H,W] = [%d,%d,%d,%d]" % (K, C, H, W))
    low = low.to(dev).float().contiguous()
    if gains is not None:
        if not isinstance(gains, torch.Tensor) or tuple(gains.shape) != (K, C):
            raise ValueError("project_views_bands: gains must be [K,C] = [%d,%d]" % (K, C))
        gains = gains.to(dev).float().contiguous()
    P = pos.shape[0]
    out = torch.zeros(P, C, device=dev)
    weight = torch.zeros(P, device=dev)
    count = torch.zeros(P, device=dev, dtype=torch.int32)
    best = torch.full((P,), -1, device=dev, dtype=torch.int32)
    _b.call("lnerf_uv_project_views_bands", _chk(pos, "pos") if P else None, _chk(nrm, "nrm") if P else None, P, _p(cams),
            K, H, W, _chk(zbuf, "zbuf"), _chk(images, "images"), _chk(low, "low"),
            _chk(gains, "gains", allow_none=True), C, float(cos_min), float(power), float(slack),
            _p(out) if P else None, _p(weight) if P else None, _p(count) if P else None, _p(best) if P else None, _stream())
    return out, weight, count, best
