"""NeRFNetwork: hash-grid encoder + fused sigma/latent MLP (+ background net), HIP-backed.
Counterpart of src/latent_nerf/models/network_grid.py of the absent package (SURVEY.md
Appendix A: sigma_net = MLP(32, 1+C, hidden 64, 3 layers, bias), density blob, bg_net)."""
import math

import torch
import torch.nn as nn

from ..raymarching import backend as _b
from ..raymarching.raymarching import _chk, _p, _stream
from . import encoding as E
from .encoding import GridEncoder
from .nerf_utils import NeRFType
from .renderer import NeRFRenderer

_PREC = {"f32": _b.F32, "bf16": _b.BF16}
_W = ("w1", "b1", "w2", "b2", "w3", "b3")


def _mlp_forward(ctx, feat, xyzs, W, m_host, m_dev, level_stride, blob_scale, blob_std, precision, workspace,
                 frag_ready=False):
    """lnerf_mlp_forward -> sigmas [level_stride], rgbs [level_stride, out_dim - 1] (f32); saves ctx for the backward."""
    out_dim = W[4].shape[0]
    sigmas = torch.empty(level_stride, device=xyzs.device, dtype=torch.float32)
    rgbs = torch.empty(level_stride, out_dim - 1, device=xyzs.device, dtype=torch.float32)
    _b.call("lnerf_mlp_forward", _chk(feat, "feat", feat.dtype), _b.F32 if feat.dtype == torch.float32 else _b.BF16,
            int(level_stride), _chk(xyzs, "xyzs"), *[_chk(t, n) for t, n in zip(W, _W)], out_dim, float(blob_scale),
            float(blob_std), int(m_host), _chk(m_dev, "m_dev", torch.int32, allow_none=True), _p(sigmas), _p(rgbs),
            precision | (_b.MLP_FRAGMENTS_READY if (frag_ready and precision == _b.BF16) else 0), _p(workspace),
            0 if workspace is None else workspace.numel(), _stream())
    ctx.save_for_backward(feat, xyzs, *W, sigmas, m_dev if m_dev is not None else torch.empty(0))
    ctx.meta = (m_host, m_dev is not None, level_stride, blob_scale, blob_std, precision, workspace)
    ctx.set_materialize_grads(False)
    return sigmas, rgbs


def _mlp_backward_workspace(workspace, precision, out_dim, device):
    """(workspace, precision tag, own): the node's own workspace when it is large enough, else a fresh one."""
    need = _b.get_lib().lnerf_mlp_backward_workspace_bytes(out_dim)
    if workspace is None or workspace.numel() < need:
        return torch.empty(need, device=device, dtype=torch.uint8), precision, False
    if precision == _b.BF16:
        # this node's forward left the weight fragments at the head of the same workspace, and autograd's version check
        # on the saved weights guarantees they have not changed since
        precision |= _b.MLP_FRAGMENTS_READY
    return workspace, precision, True


def _mlp_backward(feat, xyzs, W, sigmas, m_host, m_dev, level_stride, blob_scale, blob_std, dsigmas, drgbs, grads,
                  workspace, precision, clear_ptr=None, clear_bytes=0):
    """lnerf_mlp_backward -> dfeat (f32); writes the weight gradients into `grads` (Nones: the step's tail sums them)."""
    out_dim = W[4].shape[0]
    dev = xyzs.device
    dsigmas = torch.zeros_like(sigmas) if dsigmas is None else dsigmas.contiguous()
    drgbs = torch.zeros(level_stride, out_dim - 1, device=dev) if drgbs is None else drgbs.contiguous()
    dfeat = torch.empty(feat.shape, device=dev, dtype=torch.float32)
    _b.call("lnerf_mlp_backward", _p(feat), _b.F32 if feat.dtype == torch.float32 else _b.BF16, int(level_stride),
            _p(xyzs), *[_p(t) for t in W], out_dim, float(blob_scale), float(blob_std), int(m_host), _p(m_dev),
            _p(sigmas), _chk(dsigmas, "dsigmas"), _chk(drgbs, "drgbs"), _p(dfeat), *[_p(g) for g in grads], 0,
            _p(workspace), workspace.numel(), precision, clear_ptr, clear_bytes, _stream())
    return dfeat


class _SigmaLatentMLP(torch.autograd.Function):
    """sigmas, rgbs = MLP(feat) of given level-major features."""

    @staticmethod
    def forward(ctx, feat, xyzs, w1, b1, w2, b2, w3, b3, m_host, m_dev, level_stride, blob_scale, blob_std,
                precision, workspace):
        return _mlp_forward(ctx, feat, xyzs, (w1, b1, w2, b2, w3, b3), m_host, m_dev, level_stride, blob_scale,
                            blob_std, precision, workspace)

    @staticmethod
    def backward(ctx, dsigmas, drgbs):
        feat, xyzs, *W, sigmas, m_dev = ctx.saved_tensors
        m_host, has_mdev, level_stride, blob_scale, blob_std, precision, workspace = ctx.meta
        grads = [torch.empty_like(t) for t in W]
        workspace, precision, _own = _mlp_backward_workspace(workspace, precision, W[4].shape[0], xyzs.device)
        dfeat = _mlp_backward(feat, xyzs, W, sigmas, m_host, m_dev if has_mdev else None, level_stride, blob_scale,
                              blob_std, dsigmas, drgbs, grads, workspace, precision)
        return (dfeat, None, *grads, None, None, None, None, None, None, None)


class _HashMLPField(torch.autograd.Function):
    """sigma, latent = MLP(hash_encode(xyzs)) as ONE autograd node: the level-major feature tensor (f32 or
    bf16) and its f32 gradient stay internal, so autograd never re-casts or copies them.
    forward : gather (lnerf_grid_encode_forward) -> MLP (lnerf_mlp_forward)
    backward: MLP backward (-> dfeat f32, weight grads) -> scatter, as the route of encoding.plan_backward says."""

    @staticmethod
    def forward(ctx, xyzs, table, shadow, w1, b1, w2, b2, w3, b3, encoder, bound, m_host, m_dev, level_stride,
                blob_scale, blob_std, precision, workspace, frag_ready):
        src = table if shadow is None else shadow
        feat_dtype = torch.bfloat16 if precision == _b.BF16 else torch.float32
        feat = E.grid_encode_forward(xyzs, bound, src.detach(), encoder.levels, m_host, m_dev, level_stride, None,
                                     feat_dtype, encoder.variant)
        ctx.field = (encoder, bound)
        return _mlp_forward(ctx, feat, xyzs, (w1, b1, w2, b2, w3, b3), m_host, m_dev, level_stride, blob_scale,
                            blob_std, precision, workspace, frag_ready)

    @staticmethod
    def backward(ctx, dsigmas, drgbs):
        feat, xyzs, *W, sigmas, m_dev = ctx.saved_tensors
        m_host, has_mdev, level_stride, blob_scale, blob_std, precision, workspace = ctx.meta
        encoder, bound = ctx.field
        m_dev = m_dev if has_mdev else None
        dev, out_dim = xyzs.device, W[4].shape[0]
        workspace, tag, own_ws = _mlp_backward_workspace(workspace, precision, out_dim, dev)
        route = E.plan_backward(encoder, m_host, dev, W, own_ws)
        grads = route.views or [None if route.tail else torch.empty_like(t) for t in W]
        flags, clear_ptr, clear_bytes = route.mlp_args(encoder.levels, m_host)
        dfeat = _mlp_backward(feat, xyzs, W, sigmas, m_host, m_dev, level_stride, blob_scale, blob_std, dsigmas, drgbs,
                              grads, workspace, tag | flags, clear_ptr, clear_bytes)
        dtable = E.run_backward(route, xyzs, bound, dfeat, encoder, m_host, m_dev, level_stride, workspace, precision,
                                out_dim)
        grads = grads if route.views is None else [None] * 6       # (views: in the exchange bucket already)
        return (None, dtable, None, *grads, None, None, None, None, None, None, None, None, None, None)


class NeRFNetwork(NeRFRenderer):
    def __init__(self, cfg, num_levels=16, level_dim=2, base_resolution=16, log2_hashmap_size=19,
                 hidden_dim=64, blob_scale=5.0, blob_std=0.2):
        super().__init__(cfg, latent_mode=cfg.nerf_type == NeRFType.latent)
        if hidden_dim != 64 or num_levels * level_dim != 32:
            raise ValueError("the fused HIP MLP is built for 32 -> 64 -> 64 -> 1+C")
        # latent_tune: the RGB refinement stage -- the latent field (4 latents per sample, no sigmoid) with a linear
        # latent -> RGB decoder behind the compositing; the renders are RGB
        self.tuned = cfg.nerf_type == NeRFType.latent_tune
        self.img_dims = 3 + 1 if self.latent_mode else 3
        self.field_dims = 4 if self.tuned else self.img_dims      # channels field() returns per sample
        self.blob_scale, self.blob_std = blob_scale, blob_std
        self.precision = cfg.precision("mlp_precision")
        table_dtype = torch.bfloat16 if cfg.precision("table_dtype") == "bf16" else torch.float32
        self.encoder = GridEncoder(num_levels, level_dim, base_resolution, 2048 * self.bound, log2_hashmap_size,
                                   table_dtype=table_dtype, variant=cfg.gather_variant,
                                   scatter_variant=(cfg.scatter_variant if cfg.scatter_variant >= 0
                                                    else (3 if self.precision == "bf16" else 2)),
                                   gridtype=cfg.layout() if hasattr(cfg, "layout") else getattr(cfg, "gridtype", "hash"))
        in_dim, out_dim = self.encoder.out_dim, 1 + self.field_dims
        # nn.Linear default init, kept as bare parameters: the fused kernel takes all six at once
        self.w1 = nn.Parameter(torch.empty(hidden_dim, in_dim))
        self.b1 = nn.Parameter(torch.empty(hidden_dim))
        self.w2 = nn.Parameter(torch.empty(hidden_dim, hidden_dim))
        self.b2 = nn.Parameter(torch.empty(hidden_dim))
        self.w3 = nn.Parameter(torch.empty(out_dim, hidden_dim))
        self.b3 = nn.Parameter(torch.empty(out_dim))
        for w, b in ((self.w1, self.b1), (self.w2, self.b2), (self.w3, self.b3)):
            bound = 1.0 / math.sqrt(w.shape[1])
            nn.init.uniform_(w, -bound, bound)
            nn.init.uniform_(b, -bound, bound)
        if self.tuned:
            from ..training.guidance import LATENT_TO_RGB
            # D [3,4], no bias: starts as the known linear latent -> RGB estimate, so a latent checkpoint renders as its
            # preview did
            self.decoder = nn.Parameter(torch.tensor(LATENT_TO_RGB, dtype=torch.float32).T.contiguous())
        self.bg_radius = cfg.bg_radius
        if self.bg_radius > 0:
            self.bg_w1 = nn.Parameter(torch.empty(64, 39))
            self.bg_b1 = nn.Parameter(torch.empty(64))
            self.bg_w2 = nn.Parameter(torch.empty(self.img_dims, 64))
            self.bg_b2 = nn.Parameter(torch.empty(self.img_dims))
            for w, b in ((self.bg_w1, self.bg_b1), (self.bg_w2, self.bg_b2)):
                bound = 1.0 / math.sqrt(w.shape[1])
                nn.init.uniform_(w, -bound, bound)
                nn.init.uniform_(b, -bound, bound)
        self._mlp_ws = None
        self._normal_ws = None        # MLP workspace of the normal queries (density_gradient / normal): their own
        # bf16 weight fragments at the head of the MLP workspace: which weights they were built from, in which buffer the
        # full image (constants included) was last built, and the optimiser that keeps them current (FusedAdam(mlp=...))
        self._frag_versions = None
        self._frag_built_in = None
        self._frag_owner = None

    def mlp_workspace(self, device):
        if self._mlp_ws is None or self._mlp_ws.device != device:
            need = _b.get_lib().lnerf_mlp_backward_workspace_bytes(self.w3.shape[0])
            self._mlp_ws = torch.empty(need, device=device, dtype=torch.uint8)
            self._frag_built_in = None
        return self._mlp_ws

    def weight_versions(self):
        return (self.w1._version, self.w2._version, self.w3._version,
                self.w1.data_ptr(), self.w2.data_ptr(), self.w3.data_ptr())

    def fragments_current(self):
        """True when the weight fragments in the workspace equal the weights: only claimed under an optimiser that
        mirrors its updates into them (a replayed hipGraph changes the weights without touching torch's version
        counters; with the mirroring optimiser inside the graph the fragments move with them) and while nothing else
        has modified the weights since (version counters: FusedAdam bumps them, torch's in-place ops do)."""
        return (self.precision == "bf16" and self._frag_owner is not None and self._mlp_ws is not None
                and self._frag_built_in == self._mlp_ws.data_ptr() and self._frag_versions == self.weight_versions())

    MAX_BF16_STRIDE = 1 << 24

    # ---- per-sample field -------------------------------------------------------------
    def field(self, xyzs, m_host, m_dev=None, level_stride=None):
        """xyzs [cap,3] -> sigmas [cap], latents [cap,C] for the first min(m_host, *m_dev) rows (C = 4 latents in the
        latent and latent_tune types, 3 sigmoid colours in the rgb type)."""
        if level_stride is None:
            level_stride = xyzs.shape[0]
        if self.precision == "bf16" and level_stride > self.MAX_BF16_STRIDE and m_dev is None \
                and not torch.is_grad_enabled():
            # the bf16 kernels address features with 32-bit byte offsets (include/lnerf_hip.h: level_stride <= 2^24):
            # an inference batch beyond that is evaluated in pieces (training batches never get near it)
            outs = [self.field(xyzs[s:s + self.MAX_BF16_STRIDE], min(self.MAX_BF16_STRIDE, int(m_host) - s))
                    for s in range(0, int(m_host), self.MAX_BF16_STRIDE)]
            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
        ws = self.mlp_workspace(xyzs.device)
        enc = self.encoder
        ready = self.fragments_current()
        sigmas, rgbs = _HashMLPField.apply(xyzs, enc.embeddings, enc.shadow(), self.w1, self.b1, self.w2, self.b2,
                                           self.w3, self.b3, enc, self.bound, m_host, m_dev, level_stride,
                                           self.blob_scale, self.blob_std, _PREC[self.precision], ws, ready)
        if not ready and self.precision == "bf16" and int(m_host) > 0:   # that forward built the whole image
            self._frag_built_in = ws.data_ptr()
            self._frag_versions = self.weight_versions()
        if not (self.latent_mode or self.tuned):
            rgbs = torch.sigmoid(rgbs)
        return sigmas, rgbs

    def decode_points(self, latents):
        """latents [M,4] -> RGB [M,3] = (z D^T + 1) / 2 clamped to [0, 1]: the decoder for per-point uses (vertex
        colours, baked textures).  latent_tune only."""
        if not self.tuned:
            raise RuntimeError("decode_points needs render.nerf_type = latent_tune (this model has no decoder)")
        return ((latents.float() @ self.decoder.detach().T + 1.0) / 2.0).clamp(0, 1)

    def forward(self, x, d=None):
        x = x.reshape(-1, 3).contiguous().float()
        return self.field(x, x.shape[0])

    def density(self, x):
        sigmas, rgbs = self.forward(x)
        return {"sigma": sigmas, "albedo": rgbs}

    # ---- surface normals ----------------------------------------------------------------
    def _density_query(self, x, want_grad, want_normals):
        """sigma, grad sigma and / or the normal at x [M,3] (contiguous f32), analytically, in five launches:
        gather -> lnerf_mlp_forward -> lnerf_mlp_backward with dsigmas == 1, drgbs == 0 (its dfeat is d sigma / d feat;
        LNERF_MLP_DEFER_REDUCE: no weight gradient is reduced or written) -> lnerf_grid_encode_backward_input ->
        lnerf_density_normals.  Everything runs in a workspace of its own and through no autograd node: the fragment
        image at the head of the training workspace, the scatter workspace and every `.grad` stay as they are."""
        dev, M = x.device, x.shape[0]
        enc, prec = self.encoder, _PREC[self.precision]
        out_dim = self.w3.shape[0]
        W = [t.detach() for t in (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)]
        need = _b.get_lib().lnerf_mlp_backward_workspace_bytes(out_dim)
        if self._normal_ws is None or self._normal_ws.device != dev or self._normal_ws.numel() < need:
            self._normal_ws = torch.empty(need, device=dev, dtype=torch.uint8)
        ws = self._normal_ws
        shadow = enc.shadow()
        src = enc.embeddings.detach() if shadow is None else shadow
        feat = E.grid_encode_forward(x, self.bound, src, enc.levels, M, None, M, None,
                                     torch.bfloat16 if prec == _b.BF16 else torch.float32, enc.variant)
        fdt = _b.BF16 if prec == _b.BF16 else _b.F32
        sigmas = torch.empty(M, device=dev)
        rgbs = torch.empty(M, out_dim - 1, device=dev)
        _b.call("lnerf_mlp_forward", _p(feat), fdt, M, _p(x), *[_p(t) for t in W], out_dim, float(self.blob_scale),
                float(self.blob_std), M, None, _p(sigmas), _p(rgbs), prec, _p(ws), ws.numel(), _stream())
        ones = torch.ones(M, device=dev)
        rgbs.zero_()                                    # (re-used as drgbs == 0)
        dfeat = torch.empty(feat.shape, device=dev, dtype=torch.float32)
        # (bf16: the forward above left the fragments of these very weights at the head of `ws`)
        tag = prec | _b.MLP_DEFER_REDUCE | (_b.MLP_FRAGMENTS_READY if prec == _b.BF16 else 0)
        _b.call("lnerf_mlp_backward", _p(feat), fdt, M, _p(x), *[_p(t) for t in W], out_dim, float(self.blob_scale),
                float(self.blob_std), M, None, _p(sigmas), _p(ones), _p(rgbs), _p(dfeat), None, None, None, None, None,
                None, 0, _p(ws), ws.numel(), tag, None, 0, _stream())
        dxyz = E.grid_encode_backward_input(x, self.bound, src, enc.levels, dfeat, M, None, M, out=ones.new_empty(M, 3))
        grad = torch.empty(M, 3, device=dev) if want_grad else None
        normals = torch.empty(M, 3, device=dev) if want_normals else None
        _b.call("lnerf_density_normals", _p(dxyz), _p(x), _p(sigmas), float(self.blob_scale), float(self.blob_std), M,
                None, _p(grad), _p(normals), _stream())
        if self.density_scale != 1.0:
            sigmas = self.density_scale * sigmas
        return sigmas, grad, normals

    def _density_query_chunked(self, x, want_grad, want_normals):
        x = x.reshape(-1, 3).contiguous().float()
        M, step = x.shape[0], self.MAX_BF16_STRIDE      # (the bf16 MLP kernels' limit; field() cuts there too)
        if M == 0:
            z = torch.zeros(0, 3, device=x.device)
            return torch.zeros(0, device=x.device), (z if want_grad else None), (z.clone() if want_normals else None)
        if M <= step:
            return self._density_query(x, want_grad, want_normals)
        outs = [self._density_query(x[s:s + step], want_grad, want_normals) for s in range(0, M, step)]
        return tuple(None if outs[0][k] is None else torch.cat([o[k] for o in outs]) for k in range(3))

    @torch.no_grad()
    def density_normals(self, xyzs):
        sigmas, _, normals = self._density_query_chunked(xyzs, False, True)
        return sigmas, normals

    @torch.no_grad()
    def density_gradient(self, x):
        """x [..., 3] -> (sigmas [M] (x density_scale), grad sigma [M, 3]): the exact gradient of the trilinear field
        (one-sided on lattice planes), the density blob included.  Outside the training graph: nothing here is
        differentiable and no training state is touched."""
        sigmas, grad, _ = self._density_query_chunked(x, True, False)
        return sigmas, grad

    @torch.no_grad()
    def normal(self, x):
        """x [..., 3] -> unit surface normals [M, 3] = -grad sigma / |grad sigma| (the zero vector where the gradient
        vanishes): the upstream renderer's `normal()`, analytic instead of six finite-difference queries."""
        return self._density_query_chunked(x, False, True)[2]

    def background(self, d):
        from .bg import background_net
        return background_net(d, self.bg_w1, self.bg_b1, self.bg_w2, self.bg_b2)

    def get_params(self, lr):
        params = [{"params": [self.encoder.embeddings], "lr": lr * 10},
                  {"params": [self.w1, self.b1, self.w2, self.b2, self.w3, self.b3], "lr": lr}]
        if self.tuned:
            params.append({"params": [self.decoder], "lr": lr})
        if self.bg_radius > 0:
            params.append({"params": [self.bg_w1, self.bg_b1, self.bg_w2, self.bg_b2], "lr": lr})
        return params
