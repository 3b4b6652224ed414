"""Config tree of the Latent-Paint path.  The field names, types and defaults are the reference's CLI / YAML contract
(src/latent_paint/configs/train_config.py:7-97; demo_configs/latent_paint/goldfish.yaml); here every section is a
table of (field, type, default, help) rows turned into a dataclass by `config_cli.make_section`.  Differences from the
reference, all deliberate: `guide.texture_resolution` is a real (typed) field and can be set from the command line
(in the reference it is a bare class attribute, :41); `guide.text` / `guide.shape_path` /
`log.exp_name` default to "" so that the tree can be built without pyrallis and are checked by `validate()`;
`guide.guidance` selects the offline stand-in for the diffusion model."""
import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional, Tuple

from ... import config_cli as _cli

INTERPOLATION_MODES = ("nearest", "bilinear", "bicubic", "mipmap")
UV_ATLASES = ("triangle", "charts")
TEXTURE_FILLS = ("dilate", "pullpush")   # log.mesh_texture_fill (src/view_bake.py TEXTURE_FILLS)
BAKE_UNSEEN = ("fallback", "inpaint")    # log.mesh_bake_unseen (src/view_bake.py BAKE_UNSEEN)
BAKE_BLENDS = ("mean", "bands")          # log.mesh_bake_blend (src/view_bake.py BAKE_BLENDS)
SHADINGS = ("albedo", "lambertian", "textureless")   # render.shading
DEFAULT_LIGHTS = (1.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)   # render.lights (models/render.py DEFAULT_LIGHTS)

RenderConfig = _cli.make_section("RenderConfig", (
    ("train_grid_size", int, 64, "side of the square training render, in latent pixels"),
    ("eval_grid_size", int, 512, "side of the square evaluation render, in decoded RGB pixels"),
    ("radius_range", Tuple[float, float], (1.0, 1.5), "camera distance is drawn uniformly from this range"),
    ("angle_overhead", float, 30, "elevations in [0, angle_overhead] degrees count as the overhead view bucket"),
    ("angle_front", float, 70, "azimuths within +-angle_front degrees count as the front view bucket"),
    ("backbone", str, "texture-mesh", "'texture-mesh' (latent texture) or 'texture-rgb-mesh' (RGB fine-tuning)"),
    ("batch_size", int, 1, "views rendered and guided per optimisation step (their gradients are averaged)"),
    ("antialias", bool, False, "antialias the edges of every render: silhouettes become differentiable w.r.t. the vertices"),
    ("shading", str, "albedo", " | ".join(SHADINGS) + " (lambertian: the training render times its SH lighting from smooth "
                               "vertex normals; textureless: the lighting alone, RGB backbone only)"),
    ("shading_ratio", float, 1.0, "shading other than albedo: the probability that a training step is shaded"),
    ("lights", Tuple[float, ...], DEFAULT_LIGHTS, "shading: nine spherical-harmonic coefficients (l = 0, 1, 2) of the light"),
), doc="mesh renderer")

GuideConfig = _cli.make_section("GuideConfig", (
    ("text", str, "", "prompt"),
    ("shape_path", str, "", "mesh to paint (.obj / .off)"),
    ("append_direction", bool, True, "append the view bucket (front / side / back / overhead) to the prompt"),
    ("concept_name", Optional[str], None, "Textual-Inversion concept"),
    ("diffusion_name", str, "CompVis/stable-diffusion-v1-4", "diffusion checkpoint (name or local directory)"),
    ("shape_scale", float, 0.6, "size of the mesh inside the unit cube"),
    ("dy", float, 0.25, "lift of the mesh along +y"),
    ("texture_resolution", int, 128, "side of the square latent texture"),
    ("texture_interpolation_mode", str, "nearest", " | ".join(INTERPOLATION_MODES) + " (mipmap: trilinear over a mip "
                                                   "pyramid, the level from each pixel's footprint in the texture)"),
    ("texture_max_mip_level", int, -1, "mipmap: coarsest level used; -1 = every level the texture's side allows"),
    ("texture_lod_bias", float, 0.0, "mipmap: added to the level log2(pixel footprint in texels); > 0 blurs"),
    ("texture_mip_coverage", bool, False, "mipmap: coverage-weighted pyramid -- the texels no face covers stay out of "
                                          "every level and receive no gradient"),
    ("texture_coverage_ring", int, 1, "texture_mip_coverage: rounds the covered texels are grown by (a bilinear tap "
                                      "reads one texel beyond a chart's edge)"),
    ("init_texture", Optional[str], None, "latent texture [4,R,R] or [1,4,R,R] (torch.save) to start from, e.g. the "
                                          "latent_texture.pt of the NeRF's textured mesh export; R = texture_resolution"),
    ("uv_atlas", str, "triangle", "atlas built for a mesh without UVs when xatlas is missing: " + " | ".join(UV_ATLASES)),
    ("guidance", str, "synthetic", "'synthetic' (seeded offline stand-in) or 'stable-diffusion' (diffusers adapter)"),
), doc="guidance")

OptimConfig = _cli.make_section("OptimConfig", (
    ("seed", int, 0, "experiment seed"),
    ("iters", int, 5000, "optimisation steps"),
    ("lr", float, 1e-2, "Adam learning rate"),
    ("resume", bool, False, "continue from the experiment's latest checkpoint"),
    ("ckpt", Optional[str], None, "explicit checkpoint to load"),
    ("disp_lr", float, 0.0, "Adam learning rate of the per-vertex offsets; 0 = the geometry stays fixed (the fork's "
                            "switched-off value is 5e-5); needs render.antialias and the bilinear texture lookup"),
    ("lap_weight", float, 100.0, "disp_lr > 0: weight of the mean squared Laplacian of the offsets"),
    ("reg_weight", float, 10.0, "disp_lr > 0: weight of the mean squared offset"),
), doc="optimisation")

LogConfig = _cli.make_section("LogConfig", (
    ("exp_name", str, "", "experiment name (directory under exp_root)"),
    ("exp_root", Path, Path("experiments/"), "where experiments live"),
    ("save_interval", int, 100, "steps between checkpoints / evaluation renders"),
    ("eval_only", bool, False, "no training: load a checkpoint and run the full evaluation"),
    ("eval_size", int, 10, "evaluation views during training"),
    ("full_eval_size", int, 100, "evaluation views of the final pass"),
    ("save_mesh", bool, True, "export the textured mesh with the final evaluation"),
    ("mesh_bake_views", int, 0, "with save_mesh: > 0 projects albedo.png from this many evaluation renders of the decoded "
                                "mesh instead of decoding the atlas as one picture (kept as albedo_preview.png)"),
    ("mesh_texture_fill", str, "dilate", "texels of the exported texture outside the charts: " + " | ".join(TEXTURE_FILLS)
                                         + " (dilate: the gutter only; pullpush: the whole atlas, so that mip levels "
                                         "built from it do not seam)"),
    ("mesh_bake_unseen", str, "fallback", "with mesh_bake_views: covered texels no view sees: " + " | ".join(BAKE_UNSEEN)
                                          + " (fallback: the decoded atlas; inpaint: filled from the seen texels)"),
    ("mesh_bake_blend", str, "mean", "with mesh_bake_views: how the views that see a texel are combined: "
                                     + " | ".join(BAKE_BLENDS) + " (mean: their angle-weighted mean; bands: the mean of "
                                     "their low-passed images plus the detail of the best view alone)"),
    ("mesh_bake_exposure", bool, False, "with mesh_bake_views: one gain per view and channel, solved from the overlaps"),
    ("mesh_bake_band_sigma", float, 0.0, "mesh_bake_blend bands: sigma of the low-pass in render pixels (0 = 1 pixel)"),
    ("eval_maps", bool, False, "evaluation also writes *_normals.png, *_depth.png and *_shaded.png beside every *_rgb.png"),
    ("max_keep_ckpts", int, 2, "older checkpoints are deleted beyond this count"),
), namespace={"exp_dir": property(lambda self: Path(self.exp_root) / self.exp_name)}, doc="logging and saving")


@dataclass
class TrainConfig:
    log: LogConfig = field(default_factory=LogConfig)
    render: RenderConfig = field(default_factory=RenderConfig)
    optim: OptimConfig = field(default_factory=OptimConfig)
    guide: GuideConfig = field(default_factory=GuideConfig)

    def __post_init__(self):
        # evaluation needs weights: without an explicit checkpoint take the experiment's latest one (:94-97)
        wants_weights = self.log.eval_only and self.optim.ckpt is None
        if wants_weights and not self.optim.resume:
            self.optim.resume = True

    def validate(self):
        unset = [key for key, value in (("log.exp_name", self.log.exp_name), ("guide.shape_path", self.guide.shape_path))
                 if not value]
        if unset:
            raise ValueError("required config fields not set: %s" % ", ".join(unset))
        if self.guide.texture_interpolation_mode not in INTERPOLATION_MODES:
            raise ValueError("guide.texture_interpolation_mode must be one of %s" % ", ".join(INTERPOLATION_MODES))
        if self.guide.texture_max_mip_level < -1:
            raise ValueError("guide.texture_max_mip_level must be -1 (every level) or >= 0 (got %s)"
                             % self.guide.texture_max_mip_level)
        if not math.isfinite(self.guide.texture_lod_bias):
            raise ValueError("guide.texture_lod_bias must be finite (got %s)" % self.guide.texture_lod_bias)
        if self.guide.texture_mip_coverage and self.guide.texture_interpolation_mode != "mipmap":
            raise ValueError("guide.texture_mip_coverage needs guide.texture_interpolation_mode mipmap (got %s)"
                             % self.guide.texture_interpolation_mode)
        if self.guide.texture_coverage_ring < 0:
            raise ValueError("guide.texture_coverage_ring must be >= 0 (got %s)" % self.guide.texture_coverage_ring)
        if self.log.mesh_texture_fill not in TEXTURE_FILLS:
            raise ValueError("log.mesh_texture_fill must be one of %s, not %r"
                             % (" | ".join(TEXTURE_FILLS), self.log.mesh_texture_fill))
        if self.log.mesh_bake_unseen not in BAKE_UNSEEN:
            raise ValueError("log.mesh_bake_unseen must be one of %s, not %r"
                             % (" | ".join(BAKE_UNSEEN), self.log.mesh_bake_unseen))
        if self.guide.uv_atlas not in UV_ATLASES:
            raise ValueError("guide.uv_atlas must be one of %s, not %r" % (" | ".join(UV_ATLASES), self.guide.uv_atlas))
        if self.log.mesh_bake_blend not in BAKE_BLENDS:
            raise ValueError("log.mesh_bake_blend must be one of %s, not %r"
                             % (" | ".join(BAKE_BLENDS), self.log.mesh_bake_blend))
        if not self.log.mesh_bake_band_sigma >= 0:
            raise ValueError("log.mesh_bake_band_sigma must be >= 0 (got %s)" % self.log.mesh_bake_band_sigma)
        if (self.log.mesh_bake_blend != "mean" or self.log.mesh_bake_exposure) and not self.log.mesh_bake_views > 0:
            raise ValueError("log.mesh_bake_blend = %r / log.mesh_bake_exposure = %r need log.mesh_bake_views > 0"
                             % (self.log.mesh_bake_blend, self.log.mesh_bake_exposure))
        if self.log.mesh_bake_views < 0:
            raise ValueError("log.mesh_bake_views must be >= 0 (got %s)" % self.log.mesh_bake_views)
        if self.log.mesh_bake_views > 0 and self.guide.texture_resolution < 1:
            raise ValueError("log.mesh_bake_views = %s needs guide.texture_resolution > 0: the views are baked into the "
                             "exported texture" % self.log.mesh_bake_views)
        if self.render.batch_size < 1:
            raise ValueError("render.batch_size must be >= 1 (got %s)" % self.render.batch_size)
        if not self.optim.disp_lr >= 0:
            raise ValueError("optim.disp_lr must be >= 0 (got %s; 0 keeps the geometry fixed)" % self.optim.disp_lr)
        for name in ("lap_weight", "reg_weight"):
            if not getattr(self.optim, name) >= 0:
                raise ValueError("optim.%s must be >= 0 (got %s)" % (name, getattr(self.optim, name)))
        if self.optim.disp_lr > 0 and self.guide.texture_interpolation_mode != "bilinear":
            raise ValueError("optim.disp_lr > 0 needs guide.texture_interpolation_mode bilinear (got %s): the lookup's "
                             "gradient w.r.t. the UVs exists for that mode only" % self.guide.texture_interpolation_mode)
        if self.optim.disp_lr > 0 and not self.render.antialias:
            raise ValueError("optim.disp_lr > 0 needs render.antialias: without it a silhouette gives no gradient and "
                             "only the texture slides over the surface")
        if self.render.shading not in SHADINGS:
            raise ValueError("render.shading must be one of %s, not %r" % (" | ".join(SHADINGS), self.render.shading))
        if not 0.0 <= self.render.shading_ratio <= 1.0:
            raise ValueError("render.shading_ratio must be in [0, 1] (got %s)" % self.render.shading_ratio)
        if self.render.shading == "textureless" and self.render.backbone != "texture-rgb-mesh":
            raise ValueError("render.shading textureless needs render.backbone texture-rgb-mesh: a grey latent is not "
                             "defined (the lighting would be written into all four latent channels)")
        lights = self.render.lights
        if (not isinstance(lights, (tuple, list)) or len(lights) != 9
                or not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in lights)):
            raise ValueError("render.lights must be nine finite floats (got %r)" % (lights,))
        return self


def apply_overrides(cfg: TrainConfig, flat: dict) -> TrainConfig:
    return _cli.apply_overrides(cfg, flat)


def load_config(argv=None) -> TrainConfig:
    return _cli.load_config(TrainConfig, argv).validate()
