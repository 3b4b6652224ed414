"""Training configuration tree `log / render / optim / guide`, the surface the reference's CLI drives
(`python -m scripts.train_latent_nerf --config_path demo_configs/latent_nerf/lego_man.yaml`, or dotted flags
such as `--log.exp_name x --guide.text "..." --render.nerf_type latent`, README.md:64-69,92-97).

Field names and defaults follow the reference's present Latent-Paint config
(src/latent_paint/configs/train_config.py:7-97) and the NeRF flags its demo configs and README still
advertise for the absent package (demo_configs/latent_nerf/lego_man.yaml:1-10, README.md:140-142:
guide.shape_path, guide.mesh_scale, guide.proximal_surface, optim.lambda_shape, optim.seed, optim.iters).
pyrallis is not installed here, so `load_config()` implements the same two input forms on top of
argparse + yaml; when pyrallis is importable the dataclasses work with `pyrallis.wrap()` unchanged."""
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

from ... import config_cli as _cli
from .render_config import RenderConfig


@dataclass
class GuideConfig:
    # Guiding text prompt
    text: str = ""
    # A mesh to be used as a shape prior (sketch-shape guidance)
    shape_path: Optional[str] = None
    # Append direction to text prompts
    append_direction: bool = True
    # A Textual-Inversion concept to use
    concept_name: Optional[str] = None
    # A huggingface diffusion model to use
    diffusion_name: str = "CompVis/stable-diffusion-v1-4"
    # "synthetic": seeded stand-in for the diffusion model (offline); "stable-diffusion": diffusers adapter
    guidance: str = "synthetic"
    # Scale of the mesh that is used as the shape prior
    mesh_scale: float = 0.7
    # Strictness of the shape guidance near the surface
    proximal_surface: float = 0.3


@dataclass
class OptimConfig:
    seed: int = 0
    iters: int = 5000
    lr: float = 1e-3
    # Use amp-style mixed precision (bf16 table shadow + bf16 MFMA MLP)
    fp16: bool = True
    # Start from a checkpoint
    resume: bool = False
    ckpt: Optional[str] = None
    lambda_sparsity: float = 5e-4
    lambda_shape: float = 5e-6
    # views per optimisation step (sharded one-per-GPU in data-parallel runs)
    views_per_step: int = 1
    # single process and one view per step: the hash table's Adam step runs inside the scatter of the backward pass
    fuse_table_update: bool = True
    # data parallel, bf16: level groups the table gradient is exchanged in (each group's all-reduce is launched behind
    # its own sums while the next group is still being summed); 1 = one collective for the whole table
    exchange_groups: int = 4
    # data parallel, bf16: shard the hash table's optimiser by rows -- reduce-scatter of the bf16 gradient, the owning rank
    # runs Adam on its 1/N of the rows, all-gather of the bf16 shadow the gather reads (same wire bytes as the all-reduce,
    # 1/N of the Adam traffic per rank); the f32 master and the moments are gathered for checkpoints only
    shard_table_optimizer: bool = False
    # replay the step from captured hipGraphs (graph F: render / eager guidance / graph B: backward + optimiser); the
    # first steps, and the step after every change of the sample budget, run eagerly.  Any number of views per rank (a
    # step's views are rendered as one batch).
    graph_step: bool = True
    # a guidance object that runs on the device in the renderer's own layout (train_step_image: the synthetic one, ONE HIP
    # launch, counter-based noise) is called that way -- eager steps and captured steps alike -- and sits INSIDE the step
    # graph: one graph launch per step.  False: the reference's call shape `train_step(text_z, latents [B,C,H,W])`
    # (what a real diffusion model gets): graph F / eager guidance / graph B
    graph_guidance: bool = True
    # data parallel on RCCL: the gradient exchange (per-group sums + all-reduces, flat bucket) and the optimiser are
    # captured INTO the step graph (RCCL's collectives are capturable; one graph launch per step on every rank, no eager
    # launches between the ranks' graphs).  "false", or a backend that stages through the host (gloo): graph / eager
    # exchange + optimiser.  "auto" (default): captured on a communicator of ONE rank (LNERF_FORCE_DIST, where tests pin
    # captured == eager bit for bit), NOT with more than one rank -- no recorded multi-rank run has shown the two forms
    # equal yet (parity unpinned at N > 1); "true" / LNERF_GRAPH_COLLECTIVES=1 opt in (bench.py does so after a
    # supervised pre-flight of exactly that comparison on the job's own ranks)
    graph_collectives: str = "auto"
    # from this step on (1-based) most training renders are SHADED, as in the upstream trainers: per step, 40 % lambertian
    # (albedo x a diffuse term from the density's finite-difference normal), 40 % textureless (the diffuse term alone),
    # 20 % plain albedo, under a random light near the camera (ambient 0.1) -- the defence against flat, "painted-on"
    # geometry.  A shaded step evaluates the field at 7 points per sample.  None: every step renders the plain albedo
    start_shading_iter: Optional[int] = None
    # weight of the orientation regulariser on SHADED steps (needs start_shading_iter; the plain albedo steps of a shaded
    # schedule do not have the term, as upstream): mean over the rays of sum_i w_i max(0, n_i . v)^2, the compositing
    # weight times the squared share of the finite-difference normal that faces away from the camera -- against
    # inside-out shells and foggy fronts.  Fused into the shade kernels.  The upstream trainers use about 1e-2.  0: off
    lambda_orient: float = 0.0
    # weight of the total-variation regulariser of the hash table (the upstream trainers' lambda_tv): per level, 1 / (2 N)
    # times the sum over the lattice edges of the squared feature difference, estimated per step on whole x-lines of
    # the vertex lattice (GridEncoder.grad_total_variation) -- the training-time answer to noisy coarse geometry and
    # floaters.  Single process only; > 0 takes the table's Adam step out of the scatter (the term needs the dense f32
    # gradient), as optim.fuse_table_update = false does.  0: off, nothing changes
    lambda_tv: float = 0.0
    # lattice vertices the term samples per level and step (levels with fewer vertices are swept whole)
    tv_vertices: int = 65536
    # weight of the distortion loss of mip-NeRF 360 on every training render (albedo and shaded, latent and latent_tune):
    # mean over the rays of sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 dt_i, the compositing weights w at the samples'
    # mid-points m, in world units of the ray parameter -- it pulls a ray's weight into one compact interval, the
    # training-time answer to semi-transparent fog in front of the object and floaters between camera and surface.  The
    # gradient reaches the densities through the weights.  Any number of views and ranks (the term is local to a ray).
    # mip-NeRF 360 uses 1e-2.  0: off, nothing changes
    lambda_distortion: float = 0.0
    # weight of the 2D normal-smoothness term on the shaded steps of optim.start_shading_iter (the upstream DreamFusion-style
    # trainers' lambda_2d_normal_smooth): the finite-difference normals of a shaded render are composited into a per-pixel
    # normal image [B,H,W,3] (compositing weights NOT detached) and the squared differences between neighbouring pixels
    # are penalised,
    #   lambda * ( sum_h / (B * H * (W - 1) * 3) + sum_v / (B * (H - 1) * W * 3) ),
    # sum_h / sum_v over the horizontal / vertical pixel pairs and the three components -- against the high-frequency
    # bumps ("orange peel") that textureless shading brings out.  The plain-albedo steps of a shaded schedule do not have
    # it (they compute no normal).  Any number of views and ranks (the term is local to a view's image).  Upstream's
    # weight was not available to copy: no value is recommended here.  0: off, nothing changes
    lambda_normal_smooth: float = 0.0

MESH_ATLASES = ("triangle", "charts")   # log.mesh_atlas (src/uv_atlas.py ATLAS_CHOICES)
TEXTURE_FILLS = ("dilate", "pullpush")   # log.mesh_texture_fill (src/view_bake.py TEXTURE_FILLS)
BAKE_UNSEEN = ("fallback", "inpaint")    # log.mesh_bake_unseen (src/view_bake.py BAKE_UNSEEN)
BAKE_BLENDS = ("mean", "bands")          # log.mesh_bake_blend (src/view_bake.py BAKE_BLENDS)


@dataclass
class LogConfig:
    exp_name: str = "default"
    exp_root: Path = Path("experiments/")
    save_interval: int = 100
    eval_only: bool = False
    eval_size: int = 10
    full_eval_size: int = 100
    save_mesh: bool = False
    # with save_mesh: > 0 exports a textured mesh (per-triangle UV atlas, the field baked at this texture side) instead
    # of per-vertex colours; its latent_texture.pt starts Latent-Paint (guide.init_texture)
    mesh_texture_resolution: int = 0
    # with save_mesh: > 0 decimates the marching-cubes mesh to this many faces (or one fewer) before the colours / bake
    mesh_target_faces: int = 0
    # with save_mesh: the exported normals (and, textured, an object-space normal map normal_object.png) come from the
    # field's density gradient at the final vertices instead of the lattice / the decimated faces
    mesh_field_normals: bool = False
    # with save_mesh and mesh_texture_resolution: the UV atlas the texture lives in, "triangle" (every face a chart of its
    # own) or "charts" (connected patches projected along the axis nearest their normals, raymarching.chart_atlas)
    mesh_atlas: str = "triangle"
    # with save_mesh: the marching-cubes mesh is cleaned before anything else (raymarching.clean_mesh): connected components
    # with fewer faces than mesh_min_component_faces, or a bounding-box diagonal below mesh_min_component_diameter (a
    # fraction in [0, 1]) of the whole mesh's, are dropped; mesh_keep_largest = k > 0 keeps the k largest of the rest.
    # The upstream exporter cleans with 8 faces and 0.05 of the diagonal.  0: off
    mesh_min_component_faces: int = 0
    mesh_min_component_diameter: float = 0.0
    mesh_keep_largest: int = 0
    # with save_mesh: > 0 runs this many Taubin smoothing iterations (raymarching.smooth_mesh) before the decimation
    mesh_smooth_iterations: int = 0
    # with save_mesh and mesh_texture_resolution: > 0 bakes albedo.png from this many RENDERED views (a Fibonacci lattice
    # of directions at the evaluation camera), decoded as images -- through the guidance model's decoder with
    # log.decode_eval -- and projected into the atlas with a visibility test and an angle weight; the per-point preview
    # is kept as albedo_preview.png.  mesh_bake_view_size: side of those renders (0 = render.eval_h x render.eval_w)
    mesh_bake_views: int = 0
    mesh_bake_view_size: int = 0
    # with mesh_texture_resolution: what the exported images hold outside the charts.  "dilate": the gutter rounds only;
    # "pullpush": the whole atlas is filled from the charts (raymarching.pull_push_fill), so that the mip levels a viewer
    # builds from albedo.png / normal_object.png / latent_texture.pt do not average the empty colour in at chart borders
    mesh_texture_fill: str = "dilate"
    # with mesh_bake_views: covered texels no view sees take the point bake's colour ("fallback") or are filled from the
    # seen texels ("inpaint")
    mesh_bake_unseen: str = "fallback"
    # with mesh_bake_views: how the views that see a texel are combined.  "mean": their angle-weighted mean; "bands":
    # two-band blending -- the weighted mean of the views' low-passed images plus the detail of the best view alone, so
    # what a decoder invents per view is not averaged into a blur.  mesh_bake_band_sigma: the low-pass's sigma in
    # decoded pixels (0 = one pixel of the render, the finest scale at which decoded views agree).  mesh_bake_exposure:
    # one gain per view and channel, solved from the overlaps, takes brightness steps between views out
    mesh_bake_blend: str = "mean"
    mesh_bake_exposure: bool = False
    mesh_bake_band_sigma: float = 0.0
    # evaluation also writes a normal-shaded render (*_normals.png / *_normals video) beside every *_rgb one
    eval_normals: bool = False
    max_keep_ckpts: int = 2
    # no progress lines on stdout (log.txt in the experiment directory is still written)
    quiet: bool = False
    # evaluation renders go through the guidance model's decoder (vae.decode) instead of the linear latent->RGB preview
    decode_eval: bool = False

    @property
    def exp_dir(self) -> Path:
        return Path(self.exp_root) / self.exp_name


@dataclass
class TrainConfig:
    log: LogConfig = field(default_factory=LogConfig)
    render: RenderConfig = field(default_factory=RenderConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)
    guide: GuideConfig = field(default_factory=GuideConfig)

    def __post_init__(self):
        if self.log.eval_only and (self.optim.ckpt is None and not self.optim.resume):
            self.optim.resume = True  # same rule as src/latent_paint/configs/train_config.py:94-97
        # Precision follows optim.fp16 ONLY where the user left render.mlp_precision / render.table_dtype on "auto":
        # the set of such fields is fixed the first time (and edited by note_explicit), so that re-running this after
        # `--optim.fp16 false` or after an explicit `--render.mlp_precision f32` gives the f32 parity path.
        if not hasattr(self, "_auto_precision"):
            self._auto_precision = {n for n in ("mlp_precision", "table_dtype") if getattr(self.render, n) == "auto"}
        for n in self._auto_precision:
            setattr(self.render, n, "bf16" if self.optim.fp16 else "f32")
        for n in ("mlp_precision", "table_dtype"):
            self.render.precision(n)  # validates
        # the table layout follows the table's dtype where the user left render.gridtype on "auto": the blocked layout
        # with the bf16 shadow (a block = one 64-byte line of 4-byte rows), Instant-NGP's vertex hash with the f32 table
        if not hasattr(self, "_auto_layout"):
            self._auto_layout = self.render.gridtype == "auto"
        if self._auto_layout:
            self.render.gridtype = "blocked" if self.render.table_dtype == "bf16" else "hash"
        self.render.layout()  # validates
        if not self.optim.lambda_orient >= 0:
            raise ValueError("optim.lambda_orient must be >= 0, not %r" % (self.optim.lambda_orient,))
        if self.optim.lambda_orient > 0 and self.optim.start_shading_iter is None:
            raise ValueError("optim.lambda_orient = %r needs optim.start_shading_iter: the orientation term exists only on "
                             "shaded steps (it reads their finite-difference normal)" % (self.optim.lambda_orient,))
        if not self.optim.lambda_normal_smooth >= 0:
            raise ValueError("optim.lambda_normal_smooth must be >= 0, not %r" % (self.optim.lambda_normal_smooth,))
        if self.optim.lambda_normal_smooth > 0 and self.optim.start_shading_iter is None:
            raise ValueError("optim.lambda_normal_smooth = %r needs optim.start_shading_iter: the term acts on the "
                             "shaded steps (it composites their finite-difference normal)"
                             % (self.optim.lambda_normal_smooth,))
        if not self.optim.lambda_tv >= 0:
            raise ValueError("optim.lambda_tv must be >= 0, not %r" % (self.optim.lambda_tv,))
        if not self.optim.lambda_distortion >= 0:
            raise ValueError("optim.lambda_distortion must be >= 0, not %r" % (self.optim.lambda_distortion,))
        if not self.optim.tv_vertices >= 1:
            raise ValueError("optim.tv_vertices must be >= 1, not %r" % (self.optim.tv_vertices,))
        if self.log.mesh_atlas not in MESH_ATLASES:
            raise ValueError("log.mesh_atlas must be one of %s, not %r" % (" | ".join(MESH_ATLASES), self.log.mesh_atlas))
        if self.log.mesh_texture_fill not in TEXTURE_FILLS:
            raise ValueError("log.mesh_texture_fill must be one of %s, not %r"
                             % (" | ".join(TEXTURE_FILLS), self.log.mesh_texture_fill))
        if self.log.mesh_bake_unseen not in BAKE_UNSEEN:
            raise ValueError("log.mesh_bake_unseen must be one of %s, not %r"
                             % (" | ".join(BAKE_UNSEEN), self.log.mesh_bake_unseen))
        for n in ("mesh_min_component_faces", "mesh_min_component_diameter", "mesh_keep_largest", "mesh_smooth_iterations"):
            if not getattr(self.log, n) >= 0:
                raise ValueError("log.%s must be >= 0, not %r" % (n, getattr(self.log, n)))
        if self.log.mesh_bake_blend not in BAKE_BLENDS:
            raise ValueError("log.mesh_bake_blend must be one of %s, not %r"
                             % (" | ".join(BAKE_BLENDS), self.log.mesh_bake_blend))
        if (self.log.mesh_bake_blend != "mean" or self.log.mesh_bake_exposure) and not self.log.mesh_bake_views > 0:
            raise ValueError("log.mesh_bake_blend = %r / log.mesh_bake_exposure = %r need log.mesh_bake_views > 0"
                             % (self.log.mesh_bake_blend, self.log.mesh_bake_exposure))
        for n in ("mesh_bake_views", "mesh_bake_view_size", "mesh_bake_band_sigma"):
            if not getattr(self.log, n) >= 0:
                raise ValueError("log.%s must be >= 0, not %r" % (n, getattr(self.log, n)))
        if self.log.mesh_bake_views > 0 and not self.log.mesh_texture_resolution > 0:
            raise ValueError("log.mesh_bake_views = %r needs log.mesh_texture_resolution > 0: the views are baked into "
                             "the exported texture" % (self.log.mesh_bake_views,))
        if self.log.mesh_min_component_diameter > 1:
            raise ValueError("log.mesh_min_component_diameter is a fraction of the mesh's diagonal in [0, 1], not %r"
                             % self.log.mesh_min_component_diameter)

    def note_explicit(self, key, value):
        """config_cli.apply_overrides tells us which fields the user set."""
        section, _, name = key.partition(".")
        if section == "render" and name == "gridtype":
            self._auto_layout = value == "auto"
        if section == "render" and name in ("mlp_precision", "table_dtype"):
            if not hasattr(self, "_auto_precision"):
                self._auto_precision = set()
            (self._auto_precision.add if value == "auto" else self._auto_precision.discard)(name)


def apply_overrides(cfg: TrainConfig, flat: dict) -> TrainConfig:
    """flat: {'log.exp_name': 'x', 'render.nerf_type': 'latent', ...}"""
    return _cli.apply_overrides(cfg, flat)


def load_config(argv=None) -> TrainConfig:
    """`--config_path file.yaml` and/or dotted flags `--section.field value`."""
    return _cli.load_config(TrainConfig, argv)
