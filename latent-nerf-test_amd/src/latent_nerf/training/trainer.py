"""Trainer of the latent-NeRF path: the counterpart of the `src.latent_nerf.training.trainer.Trainer`
the reference's script imports (scripts/train_latent_nerf.py:3-4,8-14) but does not ship.  Structure,
checkpoint schema and evaluation follow the reference's present Latent-Paint trainer
(src/latent_paint/training/trainer.py: __init__ :25-54, train :113-144, evaluate :146-174,
train_render :190-209, load_checkpoint :235-286, save_checkpoint :288-310) with its one known defect
fixed the way its own fork does: the SDS gradient returned by `train_step` is injected with
`pred.backward(gradient=grad)` (src/latent_paint_mesh/training/trainer.py:657-658).

Every render/backward/optimiser op runs on the HIP library; this file is plumbing."""
import json
import math
import os
import time
from pathlib import Path

import numpy as np
import torch

from ...utils import make_path, seed_everything, tensor2numpy, write_video
from ..configs.train_config import TrainConfig
from ..models.network_grid import NeRFNetwork
from . import distributed as D
from . import shading as SH
from .guidance import (LATENT_TO_RGB, StableDiffusionGuidance, SyntheticGuidance, decode_with, sparsity_loss,
                       sparsity_loss_grad)
from .nerf_dataset import NeRFDataset
from .optimizer import FusedAdam

# approximate linear latent -> RGB map used for quick previews (src/latent_paint/models/textured_mesh.py:34-40)
_LATENT_TO_RGB = torch.tensor(LATENT_TO_RGB)


class Trainer:
    def __init__(self, cfg: TrainConfig, device=None, guidance=None):
        """Data parallel: launch one process per GPU (`python -m torch.distributed.run --nproc-per-node N -m
        scripts.train_latent_nerf ...`); scripts/train_latent_nerf.py calls distributed.init_distributed() before
        anything touches the GPU.  Every rank holds a full replica, renders `optim.views_per_step / N` views per
        step and exchanges gradients once per step (GradSync); replicas stay bit-identical (identical initial
        weights, identical reduced gradients, identical Adam step, identically seeded occupancy refresh)."""
        self.cfg = cfg
        self.train_step = 0
        self.rank, self.world = D.world_info()
        self.lambda_tv = float(getattr(cfg.optim, "lambda_tv", 0.0))
        if self.lambda_tv > 0 and D.exchange_active():
            raise ValueError("optim.lambda_tv > 0 is single-process only: the float atomics of the term on the hashed "
                             "levels would let the replicas of a data-parallel run drift apart bit by bit")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
        seed_everything(cfg.optim.seed)   # model initialisation: the same stream on every rank
        self.exp_path = make_path(cfg.log.exp_dir)
        self.ckpt_path = make_path(self.exp_path / "checkpoints")
        self.train_renders_path = make_path(self.exp_path / "vis" / "train")
        self.eval_renders_path = make_path(self.exp_path / "vis" / "eval")
        self.final_renders_path = make_path(self.exp_path / "results")
        if self.rank == 0:
            with open(self.exp_path / "config.json", "w") as f:
                json.dump(_cfg_to_dict(cfg), f, indent=1, default=str)
        if self.world > 1 and cfg.render.noise_seed is not None:
            # march jitter: a different counter-based stream per rank (poses come from pose_generator(seed, step, view),
            # which every rank can reproduce; jitter and guidance noise must NOT be correlated across ranks)
            cfg.render.noise_seed = (int(cfg.render.noise_seed) + 0x9E3779B1 * self.rank) & 0x7FFFFFFF
        self.nerf = NeRFNetwork(cfg.render).to(self.device)
        D.broadcast_parameters(list(self.nerf.parameters()))          # replicas start from rank 0's weights
        self.nerf.occupancy_generator(seed=cfg.optim.seed)            # the same refresh samples on every rank
        if self.world > 1:                                            # guidance noise / timesteps: per-rank streams
            torch.manual_seed(cfg.optim.seed + 7919 * (self.rank + 1))
            torch.cuda.manual_seed(cfg.optim.seed + 7919 * (self.rank + 1))
        self.diffusion = guidance if guidance is not None else self.init_diffusion()
        self.text_z = self.calc_text_embeddings()
        # the views of a step that this rank renders -- as ONE batch (render.batch_size of the reference's fork,
        # src/latent_paint_mesh/configs/train_config.py:32, src/latent_paint_mesh/training/views_dataset.py:98): one
        # march / gather / MLP / composite / backward over all of their rays, one optimiser step
        self.views = D.views_for_rank(max(cfg.optim.views_per_step, self.world), self.rank, self.world)
        n_views = len(self.views)
        self.exchange = D.exchange_active()     # more than one rank, or LNERF_FORCE_DIST on one
        fuse = bool(cfg.optim.fuse_table_update) and not self.exchange
        # optim.lambda_tv: the total-variation term of the table is added to its dense f32 gradient right before the
        # optimiser step, so the table's Adam step cannot run inside the scatter
        if self.lambda_tv > 0:
            if fuse:
                self.log("optim.lambda_tv = %g: the table's Adam step runs outside the scatter (plain route, dense f32 "
                         "gradient), as with optim.fuse_table_update = false" % self.lambda_tv)
            fuse = False
        # capturable: the step counter lives on the device, so that the captured step (optim.graph_step) and the eager
        # step run the very same kernels with the very same bias corrections
        self.optimizer = FusedAdam(self.nerf.get_params(cfg.optim.lr), betas=(0.9, 0.99), eps=1e-15,
                                   encoder=self.nerf.encoder, fuse_table_update=fuse, mlp=self.nerf, capturable=True)
        self.optimizer.grad_scale = 1.0 / (n_views * self.world)   # the step's gradient is the MEAN over its views
        # the whole loop (eager steps, captures, replays, collectives) runs on ONE non-default stream: autograd pins a
        # parameter's gradient accumulation to the stream it first ran on, and the legacy default stream cannot capture.
        # Code that back-propagates through `self.nerf` outside train() must do so under
        # `torch.cuda.stream(trainer.stream)` (or set optim.graph_step = false).
        self.stream = torch.cuda.Stream(device=self.device)
        self._gstep, self._gstep_capacity, self._static, self._whole = None, None, None, False
        # optim.start_shading_iter: up to TWO captured steps per sample capacity, the plain one (`_gstep`) and the shaded
        # one; `_shaded` says which form the current step takes (training/shading.py draws it)
        self._gstep_shaded, self._gstep_ws, self._shaded = None, None, False
        # (host_s: host time spent enqueueing replayed steps -- pose, upload, graph launch; refreshes not included;
        # shaded_steps: steps rendered lambertian / textureless, eager or replayed)
        self.graph_stats = {"captures": 0, "replayed_steps": 0, "eager_steps": 0, "host_s": 0.0, "shaded_steps": 0}
        small = [p for p in self.nerf.parameters() if p is not self.nerf.encoder.embeddings]
        # exchange: bf16 on the wire with the bf16 configuration (f32 otherwise); with one view per rank and step the
        # backward pass writes the wire buffer itself and the table travels in level groups (pipelined with the sums)
        bf16 = cfg.render.precision("mlp_precision") == "bf16"
        self.pipelined = self.exchange and bf16
        # optim.shard_table_optimizer: reduce-scatter / owner steps its rows / all-gather of the shadow (GradSync)
        self.sharded = bool(getattr(cfg.optim, "shard_table_optimizer", False)) and self.pipelined
        self.grad_sync = D.GradSync([self.nerf.encoder.embeddings], small,
                                    transport=torch.bfloat16 if bf16 else torch.float32, shard_optimizer=self.sharded)
        # The exchange goes into the captured step where the collectives can be captured (RCCL; not gloo's host staging)
        # AND the form has been seen to reproduce the eager exchange: optim.graph_collectives = "auto" (default) takes it
        # for a communicator of ONE rank (LNERF_FORCE_DIST; tests/test_gpu_distributed.py pins captured == eager bit for
        # bit there) and leaves it OFF for world > 1, where no recorded multi-rank run has shown that yet -- PARITY
        # UNPINNED AT N > 1; "true" / LNERF_GRAPH_COLLECTIVES=1 opt in (bench.py does, after a supervised pre-flight of
        # exactly that comparison on the job's own ranks), "false" / LNERF_GRAPH_COLLECTIVES=0 opt out.
        gc = getattr(cfg.optim, "graph_collectives", "auto")
        gc = {True: "true", False: "false"}.get(gc, str(gc).lower())
        env = os.environ.get("LNERF_GRAPH_COLLECTIVES", "")
        want = env == "1" or (env != "0" and (gc == "true" or (gc == "auto" and self.world == 1)))
        self.capture_exchange = bool(self.exchange and want and D.backend_name() == "nccl")
        if self.pipelined:
            self.grad_sync.attach_sink(self.nerf.encoder, pipeline_groups=max(1, cfg.optim.exchange_groups))
        self.dataloaders = self.init_dataloaders()
        self.shape_loss = self.init_shape_guidance()
        # optim.lambda_orient: the term's gradient w.r.t. the per-ray loss_orient of a shaded render is a CONSTANT,
        # lambda / (rays of the render) -- allocated here, before any capture, one tensor per render shape
        self._orient_const = {}
        if self._lambda_orient() > 0:
            self._orient_grad((n_views, cfg.render.train_h * cfg.render.train_w))
        # optim.lambda_distortion: the same pattern for the per-ray loss_distortion of every training render
        self._distortion_const = {}
        if self._lambda_distortion() > 0:
            self._distortion_grad((n_views, cfg.render.train_h * cfg.render.train_w))
        # optim.lambda_normal_smooth: the gradient w.r.t. image_smooth's [B,H,W,2] pair sums of a shaded render's normal
        # image is a constant too, one value per channel
        self._normal_smooth_const = {}
        if self._lambda_normal_smooth() > 0:
            self._normal_smooth_grad((n_views, cfg.render.train_h, cfg.render.train_w, 2))
        self.past_checkpoints = []
        if cfg.optim.ckpt is not None:
            self.load_checkpoint(cfg.optim.ckpt, model_only=True)
        if cfg.optim.resume:
            self.load_checkpoint(model_only=False)
        self.log("trainer ready: %d parameters, exp dir %s" % (sum(p.numel() for p in self.nerf.parameters()),
                                                              self.exp_path))

    # ------------------------------------------------------------------ set-up
    def log(self, msg):
        if self.rank == 0:
            if not getattr(self.cfg.log, "quiet", False):
                print("[trainer] " + msg, flush=True)
            with open(self.exp_path / "log.txt", "a") as f:
                f.write(msg + "\n")

    def init_diffusion(self):
        g = self.cfg.guide
        if g.guidance == "synthetic":
            return SyntheticGuidance(self.device, channels=self.nerf.img_dims, size=self.cfg.render.train_h,
                                     seed=self.cfg.optim.seed)
        return StableDiffusionGuidance(self.device, g.diffusion_name)

    def init_shape_guidance(self):
        """`guide.shape_path` -> mesh occupancy grids + shape loss (sketch-shape guidance)."""
        g = self.cfg.guide
        if not g.shape_path:
            return None
        from .shape import MeshOccupancy, ShapeLoss, load_obj, normalize_mesh
        verts, faces = load_obj(g.shape_path)
        verts = normalize_mesh(verts, target_scale=g.mesh_scale, dy=0.0)
        self.mesh_occ = MeshOccupancy(verts, faces, self.device, bound=self.nerf.bound,
                                      resolution=self.cfg.render.grid_size)
        self.mesh_occ.init_density_grid(self.nerf)
        self.log("shape guidance: %d faces from %s" % (faces.shape[0], g.shape_path))
        return ShapeLoss(self.mesh_occ, proximal_surface=g.proximal_surface)

    def calc_text_embeddings(self):
        """One embedding, or six direction-specific ones (src/latent_paint/training/trainer.py:82-91)."""
        ref_text = self.cfg.guide.text
        if not self.cfg.guide.append_direction:
            return self.diffusion.get_text_embeds(ref_text)
        return [self.diffusion.get_text_embeds("%s, %s view" % (ref_text, d))
                for d in ("front", "side", "back", "side", "overhead", "bottom")]

    def init_dataloaders(self):
        r = self.cfg.render
        return {
            "train": NeRFDataset(r, self.device, "train", r.train_h, r.train_w, 100, seed=self.cfg.optim.seed),
            "val": NeRFDataset(r, self.device, "val", r.eval_h, r.eval_w, self.cfg.log.eval_size),
            "val_large": NeRFDataset(r, self.device, "val", r.eval_h, r.eval_w, self.cfg.log.full_eval_size),
        }

    # ------------------------------------------------------------------ one optimisation step
    def _render_train(self, camera):
        """camera = (poses [B,4,4], intrinsics, H, W): B views as one batch -> (render dict, latents [B,C,H,W])."""
        out = self.nerf.render(None, None, staged=False, perturb=True, bg_color=None, force_all_rays=True, camera=camera,
                               **self._shading_args())
        H, W = int(camera[2]), int(camera[3])
        pred = out["image"].reshape(-1, H, W, out["image"].shape[-1]).permute(0, 3, 1, 2).contiguous()
        return out, pred

    def _guidance_grad(self, pred, dirs):
        """dirs: the views' direction buckets (host ints).  Direction-specific prompts: one guidance call per view."""
        if isinstance(self.diffusion, SyntheticGuidance):
            return self.diffusion.train_step(self.text_z, pred, dirs=torch.as_tensor(dirs, dtype=torch.long))
        step = self.diffusion.train_step
        if not self.nerf.latent_mode and hasattr(self.diffusion, "train_step_rgb"):
            step = self.diffusion.train_step_rgb      # an RGB prediction: the gradient comes back through the encoder
        if not isinstance(self.text_z, list):
            return step(self.text_z, pred)
        if pred.shape[0] == 1:
            return step(self.text_z[int(dirs[0])], pred)
        return torch.cat([step(self.text_z[int(d)], pred[i:i + 1]) for i, d in enumerate(dirs)])

    def _lambda_orient(self):
        return float(getattr(self.cfg.optim, "lambda_orient", 0.0))

    def _orient_grad(self, shape):
        """d(lambda_orient * mean(loss_orient)) / d(loss_orient): lambda / (number of rays of the render) on every ray, the
        normalisation of the sparsity term (sparsity_loss_grad).  One cached tensor per shape, read-only."""
        key = tuple(int(v) for v in shape)
        g = self._orient_const.get(key)
        if g is None:
            g = torch.full(key, self._lambda_orient() / max(math.prod(key), 1), device=self.device, dtype=torch.float32)
            self._orient_const[key] = g
        return g

    def _lambda_distortion(self):
        return float(getattr(self.cfg.optim, "lambda_distortion", 0.0))

    def _distortion_grad(self, shape):
        """d(lambda_distortion * mean(loss_distortion)) / d(loss_distortion): lambda / (number of rays of the render) on
        every ray, as _orient_grad.  One cached tensor per shape, read-only."""
        key = tuple(int(v) for v in shape)
        g = self._distortion_const.get(key)
        if g is None:
            g = torch.full(key, self._lambda_distortion() / max(math.prod(key), 1), device=self.device,
                           dtype=torch.float32)
            self._distortion_const[key] = g
        return g

    def _lambda_normal_smooth(self):
        return float(getattr(self.cfg.optim, "lambda_normal_smooth", 0.0))

    def _normal_smooth_grad(self, shape):
        """d(lambda_normal_smooth * (sum_h / (B H (W - 1) 3) + sum_v / (B (H - 1) W 3))) / d(the [B,H,W,2] pair sums of
        image_smooth): lambda / (B H (W - 1) 3) on channel 0, lambda / (B (H - 1) W 3) on channel 1, 0 where an image has
        no such pair (W = 1 / H = 1).  One cached tensor per shape, read-only."""
        key = tuple(int(v) for v in shape)
        g = self._normal_smooth_const.get(key)
        if g is None:
            B, H, W, _ = key
            lam, n_h, n_v = self._lambda_normal_smooth(), B * H * (W - 1) * 3, B * (H - 1) * W * 3
            g = torch.empty(key, device=self.device, dtype=torch.float32)
            g[..., 0] = lam / n_h if n_h > 0 else 0.0
            g[..., 1] = lam / n_v if n_v > 0 else 0.0
            self._normal_smooth_const[key] = g
        return g

    def _normal_smooth(self, out):
        """The [B,H,W,2] pair sums of a shaded render's normal image (raymarching.image_smooth), built once per render's
        dict; None for a render without 'normal_image'."""
        if "normal_image" not in out:
            return None
        if "loss_normal_smooth" not in out:
            from ..raymarching import image_smooth
            r = self.cfg.render
            out["loss_normal_smooth"] = image_smooth(out["normal_image"].reshape(-1, r.train_h, r.train_w, 3))
        return out["loss_normal_smooth"]

    def _backward(self, out, pred, grad, grad_ws=None):
        """SDS: d(loss)/d(pred) = grad (src/latent_paint_mesh/training/trainer.py:657-658).  The sparsity term's gradient
        w.r.t. weights_sum comes from one HIP launch (`grad_ws` when the caller already has it) and enters the
        compositing backward beside it; the orientation term of a shaded step enters the shade backward as a constant
        per-ray gradient, and so does the distortion term into its own node (its gradient joins the compositing's on the
        densities); the 2D normal-smoothness term of a shaded step enters image_smooth's node with its constant gradient
        and reaches the densities through the normal image; the shape term (a function of the samples) goes through
        autograd."""
        tensors, grads = [pred], [grad]
        if "loss_orient" in out:
            tensors.append(out["loss_orient"])
            grads.append(self._orient_grad(out["loss_orient"].shape))
        if "loss_distortion" in out:
            tensors.append(out["loss_distortion"])
            grads.append(self._distortion_grad(out["loss_distortion"].shape))
        pairs = self._normal_smooth(out)
        if pairs is not None:
            tensors.append(pairs)
            grads.append(self._normal_smooth_grad(pairs.shape))
        if self.cfg.optim.lambda_sparsity > 0:
            tensors.append(out["weights_sum"])
            grads.append(grad_ws if grad_ws is not None
                         else sparsity_loss_grad(out["weights_sum"], self.cfg.optim.lambda_sparsity))
        if self.shape_loss is not None and self.cfg.optim.lambda_shape > 0:
            loss = self.cfg.optim.lambda_shape * self.shape_loss(out["xyzs"], out["sigmas"], out["counter"])
            tensors.append(loss)
            grads.append(torch.ones_like(loss))
        torch.autograd.backward(tensors, grads)

    def step_loss(self, out):
        """Value of the auxiliary terms of one render (logging only; the step itself never needs it)."""
        loss = torch.zeros((), device=self.device)
        if self.cfg.optim.lambda_sparsity > 0:
            loss = loss + self.cfg.optim.lambda_sparsity * sparsity_loss(out["weights_sum"].detach())
        if "loss_orient" in out:
            loss = loss + self._lambda_orient() * out["loss_orient"].detach().mean()
        if "loss_distortion" in out:
            loss = loss + self._lambda_distortion() * out["loss_distortion"].detach().mean()
        pairs = self._normal_smooth(out)
        if pairs is not None:
            loss = loss + (pairs.detach() * self._normal_smooth_grad(pairs.shape)).sum()
        return loss

    def train_render(self, data):
        """Render one view and inject the guidance gradient.  Returns (pred latents [1,C,H,W], the render's dict)."""
        if data["rays_o"] is None:
            out, pred = self._render_train(data["camera"])
        else:
            H, W = data["H"], data["W"]
            out = self.nerf.render(data["rays_o"], data["rays_d"], staged=False, perturb=True, bg_color=None,
                                   force_all_rays=True, **self._distortion_args())
            pred = out["image"].reshape(1, H, W, -1).permute(0, 3, 1, 2).contiguous()
        grad = self._guidance_grad(pred, [int(d) for d in data["dir"]])
        self._backward(out, pred, grad)
        return pred, out

    def _exchange_and_step(self, n_views):
        scale = 1.0 / (n_views * self.world)
        if self.pipelined:
            ex = self.grad_sync.allreduce_pipelined()
            ex.finish_small()
            self.optimizer.step(grad_scale=scale, grads=self.grad_sync.reduced(),
                                row_groups={self.nerf.encoder.embeddings: ex.table_groups})
            ex.finish_gathers()     # (sharded optimiser: the new shadow rows of every owner; no-op otherwise)
        else:
            self.grad_sync.allreduce()
            if self.lambda_tv > 0:
                # the optimiser multiplies the whole gradient by `scale`: the term's weight is lambda_tv for any number
                # of views.  Lines: (seed, the optimiser's device step counter) -- fresh ones on every replay
                o = self.cfg.optim
                self.nerf.encoder.grad_total_variation(self.lambda_tv / scale, o.tv_vertices, seed=o.seed,
                                                       step=self.optimizer.step_no + 1, step_dev=self.optimizer.step_dev)
            self.optimizer.step(grad_scale=scale)

    # ---- shading schedule (optim.start_shading_iter)
    def shading_kind(self, step=None):
        """'albedo', 'textureless' or 'lambertian': the shading of training step `step` (default: the current one).  The
        schedule and the light distribution are the upstream trainers' (training/shading.py)."""
        return SH.shading_kind(self.cfg.optim.seed, self.train_step if step is None else step,
                               getattr(self.cfg.optim, "start_shading_iter", None))

    def _shading_args(self):
        """Keywords of the step's render: a shaded step reads its per-view record (light, ambient, textureless flag) from
        the static buffers, so the kind inside the shaded form is DATA -- one captured graph serves both kinds."""
        if not self._shaded:
            return self._distortion_args()
        args = {"shading": "lambertian", "light_d": self._static_buffers()["shade"], **self._distortion_args()}
        if self._lambda_orient() > 0:
            args["orient"] = True       # (loss_orient in the render's dict: _backward picks it up)
        if self._lambda_normal_smooth() > 0:
            args["normal_image"] = True     # (normal_image in the render's dict: _backward builds the term on it)
        return args

    def _distortion_args(self):
        """Keyword of EVERY training render, plain or shaded, when optim.lambda_distortion > 0 (loss_distortion in the
        render's dict: _backward picks it up); nothing otherwise."""
        return {"distortion": True} if self._lambda_distortion() > 0 else {}

    # ---- one step on this rank's views: camera upload -> batched render -> guidance -> backward -> exchange -> optimiser
    def _graph_ready(self):
        r = self.cfg.render
        return (bool(getattr(self.cfg.optim, "graph_step", True)) and self.nerf.cuda_ray and r.noise_seed is not None
                and self.nerf.bg_radius <= 0)

    RING = 64

    def _static_buffers(self):
        """Static device buffers the step reads its views from (eager and captured steps alike), and the ring of pinned
        upload slots: the host runs steps ahead of the GPU, a slot is rewritten only after the copy that read it has
        executed (event per slot).  Layout of a slot / of `cam`, k views: [k x 16 pose | k x 4 intrinsics | k view
        buckets (int32 bit patterns) | k x 5 shade record (unit light direction, ambient, textureless flag)]."""
        if self._static is None:
            k = len(self.views)
            r = self.cfg.render
            host = torch.zeros(self.RING, 26 * k, dtype=torch.float32).pin_memory()
            cam = torch.zeros(26 * k, device=self.device)
            self._static = {"k": k, "host": host, "host_np": host.numpy(), "host_i32": host.view(torch.int32).numpy(),
                            "events": [None] * self.RING, "cam": cam,
                            "poses": cam[:16 * k].view(k, 4, 4), "intr": cam[16 * k:20 * k].view(k, 4),
                            "dirs": cam[20 * k:21 * k].view(torch.int32), "shade": cam[21 * k:26 * k].view(k, 5),
                            "grad": torch.zeros(k, self.nerf.img_dims, r.train_h, r.train_w, device=self.device)}
        return self._static

    def _upload_views(self):
        """This step's views -- poses from the counter-based per-(step, view) stream every rank can reproduce,
        distribution of src/latent_paint/training/views_dataset.py:9-22 -- written into the next pinned slot with plain
        Python arithmetic (no torch op per view) and sent to the static buffers with ONE asynchronous copy; a shaded
        step's lights (training/shading.py) travel in the same slot.  Returns the views' direction buckets (host ints)."""
        from ..models.nerf_utils import intrinsics_from_fov, pose_values
        st = self._static_buffers()
        k, ds = st["k"], self.dataloaders["train"]
        slot = self.train_step % self.RING
        if st["events"][slot] is not None:
            st["events"][slot].synchronize()
        row, row_i = st["host_np"][slot], st["host_i32"][slot]
        dirs = []
        kind = self.shading_kind() if self._shaded else None
        for j, v in enumerate(self.views):
            p = ds.sample_pose(0, uniforms=D.pose_uniforms(self.cfg.optim.seed, self.train_step, v))
            pose = pose_values(p["theta"], p["phi"], p["radius"])
            row[16 * j:16 * j + 16] = pose
            if kind is not None:
                row[21 * k + 5 * j:21 * k + 5 * j + 5] = SH.shade_row(self.cfg.optim.seed, self.train_step, v,
                                                                      (pose[3], pose[7], pose[11]), kind)
            row[16 * k + 4 * j:16 * k + 4 * j + 4] = intrinsics_from_fov(p["fov"], ds.H, ds.W)
            row_i[20 * k + j] = p["dir_index"]
            dirs.append(p["dir_index"])
        st["cam"].copy_(st["host"][slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        st["events"][slot] = ev
        return dirs

    def _camera(self):
        st, r = self._static, self.cfg.render
        return (st["poses"], st["intr"], r.train_h, r.train_w)

    def _device_guidance(self):
        """The guidance runs as ONE HIP launch on the render's own image layout, together with the sparsity gradient
        (SyntheticGuidance.train_step_image): eager and captured steps alike, so that the two stay bit-identical.
        optim.graph_guidance = false keeps the `train_step(text_z, latents [B,C,H,W])` call shape of the reference."""
        return (hasattr(self.diffusion, "train_step_image") and bool(getattr(self.cfg.optim, "graph_guidance", True))
                and self.optimizer.step_dev is not None)

    def _device_guided_backward(self):
        """render -> fused guidance + sparsity gradient -> backward (+ exchange + optimiser) on the static views."""
        st, r = self._static, self.cfg.render
        out = self.nerf.render(None, None, staged=False, perturb=True, bg_color=None, force_all_rays=True,
                               camera=self._camera(), **self._shading_args())
        gi, gws = self.diffusion.train_step_image(out["image"], st["dirs"], r.train_h, r.train_w, self.optimizer.step_dev,
                                                  out["weights_sum"], float(self.cfg.optim.lambda_sparsity))
        self.optimizer.arm()          # no exchange: the scatter applies the table's Adam step (no-op otherwise)
        self._backward(out, out["image"], gi, gws)
        return out

    def _eager_step(self):
        dirs = self._upload_views()
        if self._device_guidance():
            out = self._device_guided_backward()
            self._exchange_and_step(len(self.views))
            return None, out
        out, pred = self._render_train(self._camera())
        grad = self._guidance_grad(pred, dirs)
        self.optimizer.arm()          # no exchange: the scatter applies the table's Adam step (no-op otherwise)
        self._backward(out, pred, grad)
        self._exchange_and_step(len(self.views))
        return pred, out

    def _all_ranks(self, failed):
        """True on every rank when `failed` is true on ANY rank (a collective decision: ranks must not end up on
        different step forms).  Eager, outside any capture."""
        if not (self.exchange and self.world > 1):
            return bool(failed)
        import torch.distributed as dist
        flag = torch.tensor([1 if failed else 0], device=self.device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MAX)
        return bool(int(flag.item()))

    def _capture(self):
        """Capture the step for the current sample capacity, in the form `self._shaded` says (plain or shaded): graph F
        (render) / eager guidance / graph B (backward, exchange where it can be captured, optimiser) -- or ONE graph when
        the guidance is capturable too.  Runs no kernel: the training state does not advance."""
        from .graph_step import GraphedRenderStep
        st = self._static_buffers()
        solo = not self.exchange
        inline = self.capture_exchange
        opt = self.optimizer
        keep = (opt.step_no, self.nerf.local_step)
        n_views = len(self.views)

        def forward():
            return self._render_train(self._camera())

        def backward(out, pred):
            if solo:
                opt.arm()                 # one process: the scatter applies the table's Adam step
            self._backward(out, pred, st["grad"])
            if solo or inline:
                self._exchange_and_step(n_views)   # (inline: collectives and the optimiser's waits on them are captured)

        # a guidance that runs on the device (the synthetic one: one HIP launch) goes INSIDE the graph: one graph launch
        # per step
        self._whole = self._device_guidance()
        if self._whole:
            from .graph_step import GraphedWholeStep

            def whole():
                out = self._device_guided_backward()
                if solo or inline:
                    self._exchange_and_step(n_views)
                return out, out["image"]

            build = lambda: GraphedWholeStep(whole, list(self.nerf.parameters()), self.stream)
        else:
            build = lambda: GraphedRenderStep(forward, backward, list(self.nerf.parameters()), self.stream)
        err = None
        try:
            gstep = build()
        except RuntimeError as e:
            err, gstep = e, None
            torch.cuda.synchronize()
        opt.step_no, self.nerf.local_step = keep   # host-side counters the captured Python advanced
        # a collective the backend cannot capture: the ranks decide TOGETHER (a capture runs nothing, so a failure is
        # local and synchronous; the all-reduce below is an ordinary eager collective every rank reaches)
        if inline and self._all_ranks(err is not None):
            self.log("capture with collectives failed on some rank (%s): the exchange stays outside the graphs on all"
                     % (str(err).splitlines()[0] if err is not None else "another rank"))
            self.capture_exchange = False
            return self._capture()
        if err is not None:
            raise err
        if self._shaded:
            self._gstep_shaded = gstep
        else:
            self._gstep = gstep
        self._gstep_capacity = self.nerf._march.capacity
        self.graph_stats["captures"] += 1

    def _have_gstep(self):
        return self._gstep is not None or self._gstep_shaded is not None

    def _scatter_ws_state(self):
        from ..models import encoding as E
        return E.scatter_workspace_epoch(self.device)

    def _graphed_step(self):
        st, g = self._static, (self._gstep_shaded if self._shaded else self._gstep)
        dirs = self._upload_views()
        if self._whole:
            grads = g.replay()
        else:
            out, pred = g.forward()
            st["grad"].copy_(self._guidance_grad(pred, dirs))
            grads = g.backward()
        self.nerf.local_step += 1
        if not self.exchange or self.capture_exchange:
            self.optimizer.note_replayed_step()
        else:   # exchange outside the graphs: the captured backward left this rank's gradients; the rest is eager
            for p, gr in zip(g.params, grads):
                p.grad = gr
            self._exchange_and_step(len(self.views))
            for p in g.params:
                p.grad = None
        self.graph_stats["replayed_steps"] += 1

    def train(self, iters=None):
        iters = self.cfg.optim.iters if iters is None else iters
        self.nerf.train()
        use_graph = self._graph_ready()
        # eager steps before the first capture of each form, plain (False) and shaded (True): lazy allocations, workspace
        # sizes (the shaded form's are its own: 7 x the samples), autograd streams
        eager_left = {False: 2, True: 2}
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            while self.train_step < iters:
                self.train_step += 1
                if self.nerf.cuda_ray and (self.train_step - 1) % self.cfg.render.update_extra_interval == 0:
                    self.nerf.update_extra_state()
                    if self._have_gstep() and self.nerf._capacity(*self.nerf._march_key) != self._gstep_capacity:
                        # the sample budget moved: new buffers, capture again (both forms)
                        self._gstep, self._gstep_shaded, eager_left = None, None, {False: 1, True: 1}
                if self._have_gstep() and self._scatter_ws_state() != self._gstep_ws:
                    # somebody else scattered through this device's shared workspace since this trainer's last step (a
                    # second model, a backward through this net outside train()): the captured steps assume the level
                    # maxima they left clean -- capture again (the new captures start from a cleared header)
                    self._gstep, self._gstep_shaded, eager_left = None, None, {False: 1, True: 1}
                sh = self._shaded = self.shading_kind() != "albedo"
                self.graph_stats["shaded_steps"] += int(sh)
                if use_graph and (self._gstep_shaded if sh else self._gstep) is None and eager_left[sh] <= 0:
                    self._capture()
                if use_graph and (self._gstep_shaded if sh else self._gstep) is not None:
                    t0 = time.perf_counter()
                    self._graphed_step()
                    self.graph_stats["host_s"] += time.perf_counter() - t0
                else:
                    eager_left[sh] -= 1
                    self.graph_stats["eager_steps"] += 1
                    self.optimizer.zero_grad()
                    self._eager_step()
                # The epoch moves with every scatter issued from Python: this trainer's own eager steps and captures, not
                # only a foreign call.  Neither disturbs what a captured step relies on -- a capture runs no kernel, and an
                # eager step of either form ends as a replay of it does (its closing scatter leaves the header of the
                # workspace it used clean; the plain and the shaded form may use different buffers of the device's list,
                # each then only ever touched by its own form) -- so the note is taken again here, after the trainer's
                # own step: alternating between the two forms triggers no recapture, a foreign scatter still does.
                self._gstep_ws = self._scatter_ws_state()
                if self.train_step % self.cfg.log.save_interval == 0:
                    self.save_checkpoint(full=True)
                    self.evaluate(self.dataloaders["val"], self.eval_renders_path)
                    self.nerf.train()
        self._shaded = False    # (renders outside the loop -- train_render, evaluation -- are plain)
        torch.cuda.current_stream().wait_stream(self.stream)
        self.log("finished training at step %d (%s)" % (self.train_step, self.graph_stats))
        # the reference's trainers close with the full evaluation pass of the last model
        # (src/latent_paint/training/trainer.py:141-144)
        self.log("evaluating the last model...")
        self.full_eval()
        self.nerf.train()

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def eval_render(self, data):
        H, W = data["H"], data["W"]
        out = self.nerf.render(data["rays_o"], data["rays_d"], staged=True, perturb=False, bg_color=None)
        pred = out["image"].reshape(1, H, W, -1).permute(0, 3, 1, 2).contiguous()
        depth = out["depth"].reshape(1, H, W)
        return pred, depth

    @torch.no_grad()
    def eval_normals_render(self, data):
        """uint8 [H,W,3]: the view rendered with shading='normal' ((n + 1) / 2 composited, no background)."""
        H, W = data["H"], data["W"]
        out = self.nerf.render(data["rays_o"], data["rays_d"], staged=True, perturb=False, bg_color=None,
                               shading="normal")
        img = out["image"].reshape(H, W, 3).float().clamp(0, 1)
        return (img * 255).round().to(torch.uint8).cpu().numpy()

    @torch.no_grad()
    def evaluate(self, dataset, save_path: Path, save_as_video=False):
        """One render per evaluation pose: PNG files during training, one video for the final pass (file names of
        src/latent_paint/training/trainer.py:146-172)."""
        from PIL import Image
        self.nerf.eval()
        frames, normal_frames = [], []
        with_normals = bool(getattr(self.cfg.log, "eval_normals", False))
        for i, data in enumerate(dataset):
            pred, depth = self.eval_render(data)
            rgb = self.preview_rgb(pred)
            frames.append(rgb)
            if self.rank == 0 and not save_as_video:
                Image.fromarray(rgb).save(save_path / ("step_%05d_%04d_rgb.png" % (self.train_step, i)))
            if with_normals:
                # the normal-shaded render the upstream trainers write beside the colour (shading='normal', no
                # background): it tells a solid from a billboard where the latent preview cannot
                nrm = self.eval_normals_render(data)
                normal_frames.append(nrm)
                if self.rank == 0 and not save_as_video:
                    Image.fromarray(nrm).save(save_path / ("step_%05d_%04d_normals.png" % (self.train_step, i)))
        if self.rank == 0 and save_as_video and frames:
            write_video(save_path / ("step_%05d_rgb" % self.train_step), frames)
            if normal_frames:
                write_video(save_path / ("step_%05d_normals" % self.train_step), normal_frames)
        return frames

    def full_eval(self):
        frames = self.evaluate(self.dataloaders["val_large"], self.final_renders_path, save_as_video=True)
        if getattr(self.cfg.log, "save_mesh", False) and self.rank == 0:
            # the density field as a triangle mesh (NeRFRenderer.export_mesh) -> <exp_dir>/mesh/mesh.obj
            tex = int(getattr(self.cfg.log, "mesh_texture_resolution", 0))
            target = int(getattr(self.cfg.log, "mesh_target_faces", 0))
            # the view bake decodes its renders the way the evaluation renders are decoded (preview_rgb)
            decoded = getattr(self.cfg.log, "decode_eval", False) and self.nerf.latent_mode
            mesh = self.nerf.export_mesh(self.exp_path / "mesh", texture_resolution=tex, target_faces=target,
                                         bake_views=int(getattr(self.cfg.log, "mesh_bake_views", 0)),
                                         view_size=int(getattr(self.cfg.log, "mesh_bake_view_size", 0)) or None,
                                         view_decoder=(lambda z: decode_with(self.diffusion, z.float())) if decoded else None,
                                         field_normals=bool(getattr(self.cfg.log, "mesh_field_normals", False)),
                                         atlas=getattr(self.cfg.log, "mesh_atlas", "triangle"),
                                         min_component_faces=int(getattr(self.cfg.log, "mesh_min_component_faces", 0)),
                                         min_component_diameter=float(getattr(self.cfg.log, "mesh_min_component_diameter", 0.0)),
                                         keep_largest=int(getattr(self.cfg.log, "mesh_keep_largest", 0)),
                                         smooth_iterations=int(getattr(self.cfg.log, "mesh_smooth_iterations", 0)),
                                         fill=getattr(self.cfg.log, "mesh_texture_fill", "dilate"),
                                         unseen=getattr(self.cfg.log, "mesh_bake_unseen", "fallback"),
                                         view_blend=getattr(self.cfg.log, "mesh_bake_blend", "mean"),
                                         view_exposure=bool(getattr(self.cfg.log, "mesh_bake_exposure", False)),
                                         view_band_sigma=float(getattr(self.cfg.log, "mesh_bake_band_sigma", 0.0)))
            self.log("exported %s (%d vertices, %d triangles; %d before decimation; iso %.4g)"
                     % (mesh["path"], mesh["verts"].shape[0], mesh["faces"].shape[0], mesh["faces_before"], mesh["iso"]))
            if mesh["components"] is not None:
                self.log("mesh cleaning kept %d of %d components (%d of %d triangles)"
                         % (mesh["components_kept"], mesh["components"], mesh["faces_cleaned"], mesh["faces_before"]))
        return frames

    def preview_rgb(self, latents):
        """[1,C,H,W] latents (latent_tune: the decoded RGB prediction) -> uint8 [H',W',3].  With `log.decode_eval` the guidance model's decoder turns the latents
        into the image (vae.decode, src/stable_diffusion.py:462-470; a guidance object without a decoder gives the
        linear preview at 8x); default: the linear latent->RGB estimate at the render resolution (no VAE offline)."""
        if getattr(self.cfg.log, "decode_eval", False) and self.nerf.latent_mode:
            rgb = decode_with(self.diffusion, latents.float())[0].permute(1, 2, 0).cpu()
            return tensor2numpy(rgb)
        x = latents[0].permute(1, 2, 0).float().cpu()
        if self.nerf.tuned and x.shape[-1] == 3:
            # a decoded prediction is RGB in [0, 1] already (unclamped): tensor2numpy takes a non-negative array as that
            # and would read one negative value as "this image is in [-1, 1]"
            return tensor2numpy(x.clamp(0, 1))
        rgb = x @ _LATENT_TO_RGB if x.shape[-1] == 4 else x[..., :3]
        return tensor2numpy(rgb.clamp(-1, 1))

    # ------------------------------------------------------------------ checkpoints
    # schema of src/latent_paint/training/trainer.py:288-310: {'train_step', 'checkpoints', 'model'[, 'optimizer']}
    def save_checkpoint(self, full=False):
        if self.sharded:   # (collective: every rank calls save_checkpoint) master table and moments whole again
            big = self.optimizer.big[0]
            self.grad_sync.gather_rows([self.nerf.encoder.embeddings.data, big[1], big[2]])
        if self.rank != 0:
            return None
        name = "step_%06d" % self.train_step
        state = {"train_step": self.train_step, "checkpoints": self.past_checkpoints,
                 "model": self.nerf.state_dict(), "table_layout": self._table_layout()}
        if full:
            state["optimizer"] = self.optimizer.state_dict()
        file_path = "%s.pth" % name
        self.past_checkpoints.append(file_path)
        if len(self.past_checkpoints) > self.cfg.log.max_keep_ckpts:
            old = self.ckpt_path / self.past_checkpoints.pop(0)
            old.unlink(missing_ok=True)
        torch.save(state, self.ckpt_path / file_path)
        return self.ckpt_path / file_path

    def _table_layout(self):
        lv = self.nerf.encoder.levels
        return {"gridtype": str(lv.gridtype), "offsets": [int(o) for o in lv.offsets],
                "resolutions": [int(r) for r in lv.resolutions]}

    def load_checkpoint(self, checkpoint=None, model_only=False):
        if checkpoint is None:
            found = sorted(self.ckpt_path.glob("*.pth"))
            if not found:
                self.log("no checkpoint found, model randomly initialized")
                return
            checkpoint = found[-1]
        state = torch.load(checkpoint, map_location=self.device, weights_only=True)
        if "model" not in state:
            self.nerf.load_state_dict(state)
            return
        # the row layout of the hashed levels is part of what the table MEANS: a `blocked` table loaded into a `hash`
        # model has the right shape and renders scrambled features (the Adam moments likewise)
        have, want = state.get("table_layout"), self._table_layout()
        if have is not None and have != want:
            raise ValueError("checkpoint %s holds a hash table laid out as %s; this model reads %s (render.gridtype / "
                             "level table differ): tables are not interchangeable" % (checkpoint, have, want))
        if have is None and want["gridtype"] != "hash":
            self.log("WARNING: checkpoint %s does not record its table layout (written before round 4: Instant-NGP "
                     "hash); loading it into a %r model scrambles the hashed levels" % (checkpoint, want["gridtype"]))
        missing, unexpected = self.nerf.load_state_dict(state["model"], strict=False)
        if missing or unexpected:
            self.log("checkpoint: missing %s unexpected %s" % (missing, unexpected))
        if model_only:
            return
        self.past_checkpoints = list(state["checkpoints"])
        self.train_step = int(state["train_step"]) + 1
        if "optimizer" in state:
            self.optimizer.load_state_dict(state["optimizer"])


def _cfg_to_dict(cfg):
    import dataclasses
    return dataclasses.asdict(cfg)
