"""TexturedMeshModel of the Latent-Paint path on the HIP raster kernels (csrc/raster.hip).

Drop-in for the reference's class of the same name: it is constructed exactly as the reference trainer
constructs it (src/latent_paint/training/trainer.py:59-60: `TexturedMeshModel(cfg, device=...,
render_grid_size=..., latent_mode=..., texture_resolution=...)`, signature src/latent_paint/models/
textured_mesh.py:16-22), exposes the members that trainer touches (`latent_mode`, `get_params()` :114-118,
`render(theta, phi, radius, decode_func, test, dims)` :181-240, `export_mesh(path, guidance)` :120-179) and keeps
the checkpoint keys (`background_sphere_colors`, `texture_img`, `texture_img_rgb_finetune`, :60-79).  What it
computes: a learnable 4-channel latent texture [1,4,R,R] looked up through the mesh's UV map, over a learnable
background = per-face-vertex colours [1,F_env,3,4] of a large sphere around the scene."""
import os
import warnings
from pathlib import Path

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import view_bake
from ...latent_nerf.raymarching.raymarching import bake_view_poses, pull_push_fill
from ...uv_atlas import chart_atlas, check_atlas_choice, per_triangle_atlas
from .mesh import Mesh
from .render import DEFAULT_LIGHTS, Renderer, mesh_umbrella, texture_coverage

# latent -> RGB linear estimate (rows = latent channels), the table of textured_mesh.py:34-40
LATENT_RGB_ROWS = ((0.298, 0.207, 0.208), (0.187, 0.286, 0.173), (-0.158, 0.189, 0.264), (-0.184, -0.271, -0.473))
LATENT_SIDE = 64   # side of the latent image the diffusion model consumes (src/stable_diffusion.py:259)
PER_TRIANGLE_MIPMAP_WARNING = (
    "guide.texture_interpolation_mode mipmap on the per-triangle atlas: faces that are neighbours on the mesh are not "
    "neighbours in this atlas, so the coarse mip levels average unrelated faces, and no filter in texture space can "
    "help that.  Use --guide.uv_atlas charts, a mesh with its own UVs, or a small --guide.texture_max_mip_level.")


def load_init_texture(path, R):
    """A latent texture saved with torch.save, [4,R,R] or [1,4,R,R] -> [1,4,R,R] f32 (CPU)."""
    tex = torch.load(path, map_location="cpu", weights_only=True)
    if not torch.is_tensor(tex):
        raise ValueError("guide.init_texture %s does not hold a tensor" % path)
    if tex.dim() == 3:
        tex = tex[None]
    if tex.dim() != 4 or tex.shape[:2] != (1, 4) or tex.shape[2] != tex.shape[3]:
        raise ValueError("guide.init_texture %s has shape %s; expected [4,R,R] or [1,4,R,R]" % (path, tuple(tex.shape)))
    if tex.shape[-1] != R:
        raise ValueError("guide.init_texture %s is %d x %d but guide.texture_resolution is %d: set "
                         "--guide.texture_resolution %d" % (path, tex.shape[-2], tex.shape[-1], R, tex.shape[-1]))
    return tex.float().contiguous()


class TexturedMeshModel(nn.Module):
    def __init__(self, opt, render_grid_size=64, latent_mode=True, texture_resolution=128,
                 device=torch.device("cpu")):
        super().__init__()
        self.opt = opt
        self.device = torch.device(device)
        self.latent_mode = latent_mode
        self.dy = opt.guide.dy
        self.mesh_scale = opt.guide.shape_scale
        self.texture_resolution = int(texture_resolution)
        self.linear_rgb_estimator = torch.tensor(LATENT_RGB_ROWS, device=self.device)
        self.renderer = Renderer(device=self.device, dim=(render_grid_size, render_grid_size),
                                 interpolation_mode=opt.guide.texture_interpolation_mode,
                                 max_mip_level=getattr(opt.guide, "texture_max_mip_level", -1),
                                 lod_bias=getattr(opt.guide, "texture_lod_bias", 0.0),
                                 mip_coverage=getattr(opt.guide, "texture_mip_coverage", False),
                                 coverage_ring=getattr(opt.guide, "texture_coverage_ring", 1),
                                 antialias=getattr(getattr(opt, "render", None), "antialias", False),
                                 lights=getattr(getattr(opt, "render", None), "lights", DEFAULT_LIGHTS))
        # shaded training renders (render.shading): the fork's `image * lighting` (src/latent_paint_mesh/training/
        # trainer.py).  The draw of render.shading_ratio has a RandomState of its own, so the trainer's draws stay put.
        self.shading = getattr(getattr(opt, "render", None), "shading", "albedo")
        self.shading_ratio = float(getattr(getattr(opt, "render", None), "shading_ratio", 1.0))
        if self.shading not in ("albedo", "lambertian", "textureless"):
            raise ValueError("render.shading must be albedo, lambertian or textureless (got %r)" % (self.shading,))
        if self.shading == "textureless" and latent_mode:
            raise ValueError("render.shading textureless needs the RGB backbone: a grey latent is not defined")
        self._shading_rng = np.random.RandomState(int(getattr(getattr(opt, "optim", None), "seed", 0)))
        self.env_sphere, self.mesh = self.init_meshes()
        self.background_sphere_colors, self.texture_img, self.texture_img_rgb_finetune = self.init_paint()
        # geometry learning (optim.disp_lr > 0): one offset per vertex, the fork's switched-off `displacement`
        # (src/latent_paint_mesh/models/textured_mesh.py:77).  Registered only then: default checkpoints keep their keys.
        optim = getattr(opt, "optim", None)
        self.learn_geometry = float(getattr(optim, "disp_lr", 0.0)) > 0.0
        self.lap_weight = float(getattr(optim, "lap_weight", 0.0))
        self.reg_weight = float(getattr(optim, "reg_weight", 0.0))
        if self.learn_geometry:
            self.displacement = nn.Parameter(torch.zeros_like(self.mesh.vertices.to(self.device).float()))
        self.vt, self.ft = self.init_texture_map()
        # per-face-vertex UVs [1,F,3,2] (kal.ops.mesh.index_vertices_by_faces in the reference, :48-50)
        self.face_attributes = self.vt[self.ft.long()][None].detach()

    # ------------------------------------------------------------------ construction
    def init_meshes(self, env_sphere_path="shapes/env_sphere.obj"):
        """Background sphere + the mesh to paint (scaled into the unit cube, lifted by dy).  The sphere is read from
        the reference's fixture when the working directory has it (`shapes/env_sphere.obj`: 5120 faces, radius 20);
        otherwise the same icosphere is generated."""
        if os.path.exists(env_sphere_path):
            env = Mesh(env_sphere_path, self.device)
        else:
            from ...latent_nerf.training.shape import make_icosphere
            ev, ef = make_icosphere(4, 20.0)
            env = Mesh(vertices=ev, faces=ef, device=self.device)
        shape = Mesh(self.opt.guide.shape_path, self.device)
        shape.normalize_mesh(inplace=True, target_scale=self.mesh_scale, dy=self.dy)
        return env, shape

    def init_paint(self, init_rgb_color=(1.0, 0.0, 0.0)):
        """Learnable state: background colours ~ U(0,1); latent texture = 0.3 x (the latent whose linear RGB
        estimate is `init_rgb_color`, ridge-regularised least squares) + 0.4 x N(0,1), or the file named by
        `guide.init_texture` (a baked texture; the mesh's own UVs then line it up); an RGB texture that is only
        used by the 'texture-rgb-mesh' fine-tuning backbone (filled from a checkpoint)."""
        dev, R = self.device, self.texture_resolution
        sky = nn.Parameter(torch.rand(1, self.env_sphere.faces.shape[0], 3, 4, device=dev))
        M = self.linear_rgb_estimator                     # [4,3]: rgb = latent @ M
        ridge = M @ M.T + 1e-2 * torch.eye(4, device=dev)
        seed_latent = torch.linalg.pinv(ridge) @ M @ torch.tensor(init_rgb_color, device=dev)
        latent_tex = nn.Parameter(0.3 * seed_latent.view(1, 4, 1, 1) + 0.4 * torch.randn(1, 4, R, R, device=dev))
        init = getattr(self.opt.guide, "init_texture", None)
        if init:
            latent_tex = nn.Parameter(load_init_texture(init, R).to(dev))
        rgb_tex = nn.Parameter(torch.zeros(1, 3, R, R, device=dev))
        return sky, latent_tex, rgb_tex

    def init_texture_map(self):
        """UV map, in the reference's order of preference (:81-109): the mesh's own UVs when every face corner
        has one; else `vt.pth` / `ft.pth` cached in the experiment directory; else a fresh atlas (xatlas when
        importable, as the reference; otherwise the built-in atlas `guide.uv_atlas` names: the per-triangle one or
        the chart atlas at the texture's resolution), which is then cached."""
        mesh = self.mesh
        if mesh.vt is not None and mesh.ft is not None and mesh.vt.shape[0] > 0 and int(mesh.ft.min()) > -1:
            return mesh.vt.to(self.device), mesh.ft.to(self.device)
        cache = Path(self.opt.log.exp_dir)
        vt_file, ft_file = cache / "vt.pth", cache / "ft.pth"
        if vt_file.exists() and ft_file.exists():
            return (torch.load(vt_file, weights_only=True).to(self.device),
                    torch.load(ft_file, weights_only=True).to(self.device))
        try:
            import xatlas
        except ImportError:
            kind = check_atlas_choice(getattr(self.opt.guide, "uv_atlas", "triangle"), "guide.uv_atlas")
            if kind == "charts":
                vt, ft = chart_atlas(mesh.vertices.to(self.device).float(), mesh.faces.to(self.device),
                                     self.texture_resolution)
            else:
                vt, ft = per_triangle_atlas(mesh.faces.shape[0], self.device)
                if getattr(self.opt.guide, "texture_interpolation_mode", None) == "mipmap":
                    warnings.warn(PER_TRIANGLE_MIPMAP_WARNING, stacklevel=2)
        else:
            atlas = xatlas.Atlas()
            atlas.add_mesh(mesh.vertices.cpu().numpy(), mesh.faces.int().cpu().numpy())
            chart = xatlas.ChartOptions()
            chart.max_iterations = 4
            atlas.generate(chart_options=chart)
            _, ft_np, vt_np = atlas[0]
            vt = torch.from_numpy(vt_np.astype(np.float32)).to(self.device)
            ft = torch.from_numpy(ft_np.astype(np.int64)).to(self.device)
        cache.mkdir(parents=True, exist_ok=True)
        torch.save(vt.cpu(), vt_file)
        torch.save(ft.cpu(), ft_file)
        return vt, ft

    def forward(self, x):
        raise NotImplementedError("TexturedMeshModel is driven through render()")

    def get_params(self):
        """What the optimiser trains: the background colours plus the texture of the active backbone."""
        texture = self.texture_img if self.latent_mode else self.texture_img_rgb_finetune
        return [self.background_sphere_colors, texture]

    def get_geometry_params(self):
        """What the geometry group of the optimiser trains (at optim.disp_lr): the vertex offsets; [] when off."""
        return [self.displacement] if self.learn_geometry else []

    def surface_vertices(self):
        """The vertices that are rendered and exported: the mesh's own, plus the learned offsets when geometry is on."""
        if not self.learn_geometry:
            return self.mesh.vertices
        return self.mesh.vertices.to(self.device).float() + self.displacement

    def geometry_loss(self):
        """lap_weight * mean_i |(L d)_i|^2 + reg_weight * mean_i |d_i|^2 of the offsets d, L the face-weighted uniform
        Laplacian (render.mesh_umbrella: no dense matrix, no inverse).  The fork's term
        (src/latent_paint_mesh/models/textured_mesh.py:314-317) with its dense V x V `L` replaced, and a MEAN per vertex
        where the fork sums, so that the weights do not depend on the size of the mesh."""
        d = self.displacement
        lap = mesh_umbrella(d, self.mesh.faces)
        return self.lap_weight * lap.square().sum(-1).mean() + self.reg_weight * d.square().sum(-1).mean()

    def _antialias(self, image, coverage, state):
        """Edge-antialiased (image, mask) of one render: both go through the pass as one [B,C+1,H,W] batch."""
        both = self.renderer.antialias_views(torch.cat([image, coverage], dim=1), state, self.mesh.faces)
        return both[:, :-1], both[:, -1:]

    # ------------------------------------------------------------------ rendering
    def _view(self, theta, phi, radius):
        """Scalars (one view) or sequences of one length B -> the keyword arguments of Renderer.render_views*."""
        seq = [isinstance(a, (list, tuple)) or (torch.is_tensor(a) and a.dim() > 0) or
               (isinstance(a, np.ndarray) and a.ndim > 0) for a in (theta, phi, radius)]
        if any(seq) and not all(seq):
            raise ValueError("render: theta, phi and radius must be all scalars or all sequences")
        if not seq[0]:
            theta, phi, radius = [theta], [phi], [radius]
        as_floats = lambda a: [float(v) for v in a]
        return {"elev": as_floats(theta), "azim": as_floats(phi), "radius": as_floats(radius), "look_at_height": self.dy}

    def render(self, theta, phi, radius, decode_func=None, test=False, dims=None, maps=False):
        """theta, phi, radius: scalars (one view, [1,...] results) or sequences of length B ([B,...] results)."""
        if test:
            return self.render_test(theta, phi, radius, decode_func, dims=dims, maps=maps)
        return self.render_train(theta, phi, radius)

    def render_train(self, theta, phi, radius):
        """-> {'image' [B,C,h,w], 'mask' [B,1,h,w], 'background', 'foreground'}; C = 4 latents (or 3 RGB when
        fine-tuning).  The rasterisation itself carries no gradient: 'image' is differentiable w.r.t. the texture
        (under the mesh) and the background colours (elsewhere).
        With render.antialias the composite and the coverage are edge-antialiased with the mesh's own raster state
        ('image' and 'mask' are then the antialiased ones); with optim.disp_lr > 0 the mesh is rendered at
        vertices + displacement, 'image' and 'mask' are differentiable w.r.t. the offsets (inside the faces through the
        UVs, at silhouettes through the antialiasing) and 'geometry_loss' (geometry_loss(), a scalar) is added.
        With render.shading lambertian / textureless a step is shaded with probability render.shading_ratio: the
        foreground is `foreground * lighting` on every channel, latent or RGB, as the fork trains (textureless: the
        lighting alone on three channels, RGB backbone only); composite, antialiasing and resize follow as before, and
        'normal' [B,3,h,w], 'lighting', 'depth' [B,1,h,w] (Renderer.shade_views, at the render's size) and 'shading' (the
        mode) are added.  The lighting depends on the surface's orientation, so the offsets then receive the image's
        gradient inside a face even under a constant texture."""
        if self.latent_mode:
            texture, sky_colors = self.texture_img, self.background_sphere_colors
        else:
            texture = self.texture_img_rgb_finetune
            sky_colors = self.background_sphere_colors @ self.linear_rgb_estimator
        view = self._view(theta, phi, radius)
        foreground, coverage, state = self.renderer.render_views_texture(
            self.surface_vertices(), self.mesh.faces, self.face_attributes, texture, return_state=True, **view)
        background, _ = self.renderer.render_views(self.env_sphere, sky_colors, **view)
        coverage = coverage.detach()
        maps = self._shading_maps(state) if self._shaded_step() else None
        if maps is not None:   # lighting is 0 on background, as the foreground is
            foreground = (foreground * maps["lighting"] if self.shading == "lambertian"
                          else maps["lighting"].expand(-1, 3, -1, -1))
        image = background * (1 - coverage) + foreground * coverage
        if self.renderer.antialias:
            image, coverage = self._antialias(image, coverage, state)
        out = {"image": image, "mask": coverage, "background": background, "foreground": foreground}
        if self.latent_mode and coverage.shape[-1] != LATENT_SIDE:
            # the diffusion model takes LATENT_SIDE x LATENT_SIDE latents whatever the render size
            out = {k: F.interpolate(v, (LATENT_SIDE, LATENT_SIDE), mode="bicubic") for k, v in out.items()}
        if maps is not None:   # (at the render's own size: a resampled normal is no unit vector)
            out.update(maps, shading=self.shading)
        if self.learn_geometry:
            out["geometry_loss"] = self.geometry_loss()
        return out

    def _shaded_step(self):
        """Whether this training step is shaded: never with render.shading albedo (and nothing is drawn then), else with
        probability render.shading_ratio."""
        return self.shading != "albedo" and float(self._shading_rng.uniform(0, 1)) < self.shading_ratio

    def _shading_maps(self, state):
        """{'normal' [B,3,H,W], 'lighting' [B,1,H,W], 'depth' [B,1,H,W]} of a rendered batch (Renderer.shade_views)."""
        normal, lighting, depth = self.renderer.shade_views(self.surface_vertices(), self.mesh.faces, state)
        return {"normal": normal, "lighting": lighting, "depth": depth}

    def render_test(self, theta, phi, radius, decode_func=None, dims=None, maps=False):
        """Evaluation view: the latent texture is decoded to RGB first (`decode_func` = the guidance's
        `decode_latents`), then rendered at `dims` on a white background; edge-antialiased with render.antialias.
        maps: 'normal', 'lighting' and 'depth' of the same views (Renderer.shade_views, at `dims`) are added."""
        if self.latent_mode:
            if decode_func is None:
                raise ValueError("decode function was not supplied to decode the latent texture image")
            texture = decode_func(self.texture_img)
        else:
            texture = self.texture_img_rgb_finetune
        image, coverage, state = self.renderer.render_views_texture(
            self.surface_vertices(), self.mesh.faces, self.face_attributes, texture, dims=dims, white_background=True,
            return_state=True, **self._view(theta, phi, radius))
        if self.renderer.antialias:
            image, coverage = self._antialias(image, coverage, state)
        out = {"image": image, "texture_map": texture, "mask": coverage}
        if maps:
            out.update(self._shading_maps(state))
        return out

    # ------------------------------------------------------------------ export
    @torch.no_grad()
    def export_mesh(self, path, guidance=None, bake_views=0, view_size=None, fill="dilate", unseen="fallback",
                    view_blend="mean", view_exposure=False, view_band_sigma=0.0):
        """Writes `albedo.png` (the decoded texture), `mesh.obj` (v / vt / f v/vt) and `mesh.mtl` into `path`.
        bake_views = K > 0: the decoder sees the whole atlas as one picture, so chart borders and unrelated neighbouring
        charts are decoded together; instead `albedo.png` is projected from K evaluation renders of the decoded mesh
        (render_test at `view_size`, default render.eval_grid_size; the directions of raymarching.bake_view_poses at the
        evaluation radius) with view_bake.bake_views, the decoded atlas filling the texels no view sees and kept as
        `albedo_preview.png`.
        fill = "pullpush": the texels of the decoded atlas that no face covers (raymarching.uv_raster at the decoded
        side) are filled from the covered ones over the whole atlas (raymarching.pull_push_fill; the covered texels keep
        their bits), and so is the view bake's image beyond its gutter -- mip levels built from the files then do not
        seam at chart borders.  "dilate" leaves every file byte for byte what it was.  unseen = "inpaint" (K > 0):
        covered texels no view sees are filled from the seen ones instead of taking the decoded atlas' colour.
        view_blend = "bands", view_exposure = True, view_band_sigma (K > 0): two-band blending and per-view exposure
        gains of view_bake.bake_views (sigma in pixels of the renders; 0: 1 pixel, the renders are not up-scaled); off
        by default, and every file is then byte for byte what it was.
        -> dict(rgb [3,R,R]; K > 0: + view_rgb, view_weight, view_count, mask; + view_best with "bands", view_gains
        with view_exposure)."""
        from PIL import Image
        bake_views = int(bake_views)
        if bake_views < 0:
            raise ValueError("export_mesh: bake_views must be >= 0 (got %d)" % bake_views)
        view_bake.check_choice(fill, view_bake.TEXTURE_FILLS, "export_mesh: fill")
        view_bake.check_choice(unseen, view_bake.BAKE_UNSEEN, "export_mesh: unseen")
        view_bake.check_choice(view_blend, view_bake.BAKE_BLENDS, "export_mesh: view_blend")
        if not float(view_band_sigma) >= 0.0:
            raise ValueError("export_mesh: view_band_sigma must be >= 0 (got %r)" % (view_band_sigma,))
        if bake_views == 0 and (view_blend != "mean" or view_exposure):
            raise ValueError("export_mesh: view_blend = %r / view_exposure = %r need bake_views > 0"
                             % (view_blend, view_exposure))
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        if self.latent_mode:
            if guidance is None:
                raise ValueError("export_mesh needs the guidance model to decode the latent texture")
            from ...latent_nerf.training.guidance import decode_with
            rgb = decode_with(guidance, self.texture_img)
        else:
            rgb = self.texture_img_rgb_finetune
        if fill == "pullpush":
            covered = texture_coverage(self.surface_vertices(), self.mesh.faces, self.face_attributes[0], rgb.shape[-1],
                                       ring=0)
            rgb = pull_push_fill(rgb[0].float(), covered.float())[0][None]
        albedo = (rgb[0].permute(1, 2, 0).clamp(0, 1).cpu().numpy() * 255).astype(np.uint8)
        result = {"rgb": rgb[0]}
        if bake_views > 0:
            Image.fromarray(albedo).save(path / "albedo_preview.png")
            result.update(self._bake_rendered_views(rgb, bake_views, view_size, fill, unseen,
                                                    (view_blend, bool(view_exposure), float(view_band_sigma))))
            # (the projected image is rounded to 8 bits, as the NeRF exporter's; the preview above keeps the upstream
            # exporter's truncation, so that it and the K = 0 file stay byte for byte what they were)
            albedo = view_bake.to_uint8(result["view_rgb"])
        Image.fromarray(albedo).save(path / "albedo.png")
        self._write_obj(path)
        return result

    def _bake_rendered_views(self, rgb, K, view_size, fill="dilate", unseen="fallback", blend=("mean", False, 0.0)):
        """export_mesh's view bake over the decoded atlas `rgb` [1,3,R,R]: K renders of it on the mesh, projected back."""
        side = int(view_size or self.opt.render.eval_grid_size)
        poses = bake_view_poses(K)
        view = self._view([t for t, _ in poses], [p for _, p in poses], [self.opt.render.radius_range[1] * 1.2] * K)
        cams = self.renderer._cameras(view["elev"], view["azim"], view["radius"], view["look_at_height"])
        # (the atlas is decoded already: render_test's decoder hands it back; the RGB backbone renders its own texture)
        images = self.render_test(view["elev"], view["azim"], view["radius"], decode_func=lambda _t: rgb,
                                  dims=(side, side))["image"]
        baked = view_bake.bake_views(self.surface_vertices(), self.mesh.faces, self.vt, self.ft, images.clamp(0, 1), cams,
                                     rgb.shape[-1], fallback=rgb[0].float().clamp(0, 1), fill=fill, unseen=unseen,
                                     blend=blend[0], exposure=blend[1], band_sigma=blend[2])
        return {"view_rgb": baked["rgb"], "view_weight": baked["view_weight"], "view_count": baked["view_count"],
                "mask": baked["mask"], **{k: baked[k] for k in ("view_gains", "view_best") if k in baked}}

    def _write_obj(self, path):
        v = self.surface_vertices().detach().cpu().numpy()
        f = self.mesh.faces.cpu().numpy() + 1
        vt = self.vt.cpu().numpy()
        ft = self.ft.cpu().numpy() + 1
        lines = ["mtllib mesh.mtl"]
        lines += ["v %s %s %s" % (p[0], p[1], p[2]) for p in v]
        lines += ["vt %s %s" % (t[0], t[1]) for t in vt]
        lines.append("usemtl mat0")
        lines += ["f %d/%d %d/%d %d/%d" % (a[0], b[0], a[1], b[1], a[2], b[2]) for a, b in zip(f, ft)]
        (path / "mesh.obj").write_text("\n".join(lines) + "\n")
        (path / "mesh.mtl").write_text("newmtl mat0\nKa 1.000000 1.000000 1.000000\nKd 1.000000 1.000000 1.000000\n"
                                       "Ks 0.000000 0.000000 0.000000\nTr 1.000000\nillum 1\nNs 0.000000\n"
                                       "map_Kd albedo.png\n")
