"""The coverage-weighted pyramids end to end on the GPU: Latent-Paint training with `guide.texture_mip_coverage`, the
exports' fill="pullpush" and the view bake's unseen="inpaint".

The one bound used here is the push's, derived in tests/test_gpu_mipcov.py: a filled texel is within (13 L + 2) ULP of
the magnitude the fill propagates, L the levels of the (padded) side; for values in [lo, hi] that magnitude is at most
max(|lo|, |hi|).  The float64 box pyramid (tests/mip_reference.pyramid) of such a texture adds nothing to it."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests import mip_reference as M
from tests.test_gpu_view_bake import _nerf, fibonacci_cameras, smooth_images

pytestmark = pytest.mark.gpu

ULP = M.ULP
SHAPES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _push_bound(R, magnitude):
    """pull_push_fill pads the side to the next power of two: L = ceil(log2 R) levels."""
    return (13 * (R - 1).bit_length() + 2) * ULP * magnitude


# ------------------------------------------------------------------------------------------------------- training
def _paint_cfg(tmp_path, name, **over):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": name, "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(SHAPES, "blub.obj"), "guide.texture_resolution": 64,
            "guide.texture_interpolation_mode": "mipmap"}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def _one_step(tr):
    tex0 = tr.mesh_model.texture_img.detach().clone()
    data = next(iter(tr.dataloaders["train"]))
    tr.train_step += 1
    tr.optimizer.zero_grad()
    pred, _ = tr.train_render(data)
    tr.optimizer.step()
    assert pred.shape == (1, 4, 64, 64) and bool(torch.isfinite(pred).all())
    return (tr.mesh_model.texture_img.detach() - tex0).abs()[0] > 0           # [4,R,R]: Adam moves what got a gradient


def test_trainer_step_with_coverage_moves_no_texel_outside_it(dev, tmp_path):
    from src.latent_paint.models.render import texture_coverage
    from src.latent_paint.training.trainer import Trainer
    plain = Trainer(_paint_cfg(tmp_path, "plain"), device=dev)
    assert plain.cfg.guide.uv_atlas == "triangle" and plain.mesh_model.renderer.mip_coverage is False
    model = plain.mesh_model
    covered = texture_coverage(model.mesh.vertices, model.mesh.faces, model.face_attributes[0], 64, ring=1)
    bare = texture_coverage(model.mesh.vertices, model.mesh.faces, model.face_attributes[0], 64, ring=0)
    assert 100 < int(bare.sum()) < int(covered.sum()) < 64 * 64 and bool(covered[bare].all())
    outside = ~covered
    moved_plain = _one_step(plain)
    print("plain mipmap: %d of %d texels moved, %d of them outside the coverage (%d texels)" % (
        int(moved_plain[0].sum()), 64 * 64, int(moved_plain[0][outside].sum()), int(outside.sum())))
    assert int(moved_plain[:, outside].sum()) > 0                             # the comparison has teeth
    tr = Trainer(_paint_cfg(tmp_path, "cov", **{"guide.texture_mip_coverage": True}), device=dev)
    r = tr.mesh_model.renderer
    assert (r.mip_coverage, r.coverage_ring, r.interpolation_mode) == (True, 1, "mipmap")
    moved = _one_step(tr)
    w0, wpyr = r.coverage_weights(tr.mesh_model.mesh.vertices, tr.mesh_model.mesh.faces, tr.mesh_model.face_attributes[0],
                                  64, 6)
    assert torch.equal(w0 > 0, covered) and len(r._coverage) == 1             # one side so far, computed once
    assert int(moved.sum()) > 1000
    assert not bool(moved[:, outside].any()), int(moved[:, outside].sum())
    # a checkpoint round-trip: the flag is configuration, the texture is state
    path = tr.save_checkpoint(full=True)
    tr2 = Trainer(_paint_cfg(tmp_path, "cov", **{"guide.texture_mip_coverage": True, "optim.resume": True,
                                                 "guide.texture_coverage_ring": 2}), device=dev)
    assert path.exists() and tr2.train_step == 2
    assert torch.equal(tr2.mesh_model.texture_img, tr.mesh_model.texture_img)
    assert tr2.mesh_model.renderer.coverage_ring == 2
    moved2 = _one_step(tr2)
    wider = texture_coverage(model.mesh.vertices, model.mesh.faces, model.face_attributes[0], 64, ring=2)
    assert int(wider.sum()) > int(covered.sum()) and not bool(moved2[:, ~wider].any())


def test_render_test_with_a_decoded_texture_of_another_side(dev, tmp_path):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    cfg = _paint_cfg(tmp_path, "decoded", **{"guide.texture_mip_coverage": True})
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=64)
    decode = lambda side: (lambda t: F.interpolate(t[:, :3].sigmoid(), (side, side), mode="bilinear"))
    view = (math.radians(60.0), math.radians(30.0), 1.25)
    with torch.no_grad():
        big = model.render(*view, decode_func=decode(512), test=True, dims=(48, 48))      # 8 R: nine levels
        again = model.render(*view, decode_func=decode(512), test=True, dims=(48, 48))
        odd = model.render(*view, decode_func=decode(63), test=True, dims=(48, 48))       # no level: level 0 alone
        sides = sorted(k[0] for k in model.renderer._coverage)
        model.renderer.mip_coverage = False
        big_plain = model.render(*view, decode_func=decode(512), test=True, dims=(48, 48))
    assert sides == [63, 512]                                                 # one coverage per side, reused
    assert big["image"].shape == (1, 3, 48, 48) and big["texture_map"].shape == (1, 3, 512, 512)
    assert bool(torch.isfinite(big["image"]).all()) and torch.equal(big["image"], again["image"])
    assert odd["image"].shape == (1, 3, 48, 48) and bool(torch.isfinite(odd["image"]).all())
    assert torch.equal(big["mask"], big_plain["mask"]) and 0.05 < float(big["mask"].mean()) < 0.9
    # the decoded texture is in (0, 1): so is every normalised lookup of it; and it differs from the plain pyramid's,
    # which reads the texels between the charts too
    assert float(big["image"].min()) >= 0.0 and float(big["image"].max()) <= 1.0 + 1e-6
    assert not torch.equal(big["image"], big_plain["image"])


# ------------------------------------------------------------------------------------------------------- exports
def _sphere(dev):
    """The small marching-cubes sphere of tests/test_gpu_view_bake.py (r = 0.6 on a 32^3 lattice)."""
    from src.latent_nerf.raymarching import marching_cubes
    a = torch.linspace(-1, 1, 32)
    X, Y, Z = torch.meshgrid(a, a, a, indexing="ij")
    vol = (0.6 - torch.sqrt(X * X + Y * Y + Z * Z)).float().to(dev)
    v, f, _ = marching_cubes(vol, 0.0, (-1, -1, -1), (1, 1, 1))
    return v, f


def test_pullpush_fill_leaves_no_seam_in_any_mip_level(dev):
    from src.latent_nerf.raymarching import chart_atlas
    net, _ = _nerf(dev)
    v, f = _sphere(dev)
    R = 64
    vt, ft, _ = chart_atlas(v, f, R)
    const = torch.tensor([0.25, 0.5, 0.8123], device=dev)
    fn = lambda pts: const[None].expand(pts.shape[0], 3)
    plain = net.bake_texture(v, f, vt, ft, resolution=R, fn=fn)
    dilate = net.bake_texture(v, f, vt, ft, resolution=R, fn=fn, fill="dilate")
    push = net.bake_texture(v, f, vt, ft, resolution=R, fn=fn, fill="pullpush")
    for key in ("texture", "mask", "rgb"):
        assert torch.equal(plain[key], dilate[key]), key
    mask = plain["mask"]
    assert int((mask == 2).sum()) > 500 and int((mask == 1).sum()) > 0 and int((mask == 0).sum()) > 100
    # every texel the gutter bake owns keeps its bits; the rest is filled and marked 3
    assert torch.equal(push["texture"][:, mask > 0], plain["texture"][:, mask > 0])
    assert torch.equal(push["mask"][mask > 0], mask[mask > 0]) and bool((push["mask"][mask == 0] == 3).all())
    c64 = const.double().cpu().view(3, 1, 1)
    L = M.full_levels(R)
    levels = M.pyramid(push["texture"].cpu(), L)
    assert len(levels) == 7 and levels[-1].shape == (3, 1, 1)
    for l, lev in enumerate(levels):
        assert bool(((lev - c64).abs() <= _push_bound(R, c64.abs())).all()), l
    # the gutter alone: from level 3 on a coarse texel under a chart averages the empty colour in
    under = F.max_pool2d((mask == 2).float()[None, None], 8)[0, 0].bool().cpu()            # level-3 texels under a chart
    lev3 = M.pyramid(plain["texture"].cpu(), 3)[3]
    off = ((lev3 - c64).abs() > 0.1 * c64)[:, under]
    print("dilate: %d of %d level-3 texels under a chart are more than 10 %% off" % (int(off[0].sum()), int(under.sum())))
    assert bool(off.any())


def test_export_files_with_fill(dev, tmp_path):
    net, cfg = _nerf(dev)
    kw = dict(resolution=64, S=32, thresh=cfg.density_thresh, texture_resolution=64, atlas="charts", field_normals=True)
    plain = net.export_mesh(str(tmp_path / "plain"), **kw)
    dilate = net.export_mesh(str(tmp_path / "dilate"), fill="dilate", unseen="fallback", **kw)
    names = {p.name for p in (tmp_path / "plain").iterdir()}
    assert names == {"mesh.obj", "mesh.mtl", "albedo.png", "latent_texture.pt", "normal_object.png"}
    assert names == {p.name for p in (tmp_path / "dilate").iterdir()}
    for name in names:
        assert (tmp_path / "dilate" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    push = net.export_mesh(str(tmp_path / "push"), fill="pullpush", **kw)
    assert names == {p.name for p in (tmp_path / "push").iterdir()}
    mask = plain["mask"]
    assert int((mask == 0).sum()) > 100 and bool((push["mask"][mask == 0] == 3).all())
    for key in ("texture", "rgb", "normal_map"):
        assert torch.equal(push[key][:, mask > 0], plain[key][:, mask > 0]), key
        assert not torch.equal(push[key][:, mask == 0], plain[key][:, mask == 0]), key
    for name in ("mesh.obj", "mesh.mtl"):
        assert (tmp_path / "push" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    for name in ("albedo.png", "latent_texture.pt", "normal_object.png"):
        assert (tmp_path / "push" / name).read_bytes() != (tmp_path / "plain" / name).read_bytes(), name
    saved = torch.load(tmp_path / "push" / "latent_texture.pt", weights_only=True)
    assert torch.equal(saved, push["texture"].cpu())
    with pytest.raises(ValueError, match="fill"):
        net.export_mesh(str(tmp_path / "bad"), fill="push", **kw)
    with pytest.raises(ValueError, match="unseen"):
        net.export_mesh(str(tmp_path / "bad"), unseen="paint", **kw)


def test_inpaint_fills_the_texels_no_view_sees(dev):
    from src import view_bake
    from src.uv_atlas import atlas_min_resolution, per_triangle_atlas
    v, f = _sphere(dev)
    vt, ft = per_triangle_atlas(f.shape[0], dev)
    R = atlas_min_resolution(f.shape[0])
    side = 64
    cams = fibonacci_cameras(1, 1.8, 55.0, side, side, dev)
    images = torch.from_numpy(smooth_images(1, 3, side, side)).to(dev)
    fallback = torch.full((3, R, R), 2.0, device=dev)                          # outside every image's range
    args = (v, f, vt, ft, images, cams, R)
    base = view_bake.bake_views(*args, fallback=fallback)
    same = view_bake.bake_views(*args, fallback=fallback, unseen="fallback", fill="dilate")
    got = view_bake.bake_views(*args, fallback=fallback, unseen="inpaint")
    for key in ("rgb", "mask", "view_count", "view_weight"):
        assert torch.equal(base[key], same[key]), key
    covered = base["mask"] == 2
    seen = covered & (base["view_count"] > 0)
    hole = covered & ~seen
    print("one view: %d covered texels, %d seen, %d inpainted" % (int(covered.sum()), int(seen.sum()), int(hole.sum())))
    assert int(seen.sum()) > 1000 and int(hole.sum()) > 1000                   # one view cannot see the far side
    assert torch.equal(got["view_count"], base["view_count"]) and torch.equal(got["mask"], base["mask"])
    assert torch.equal(got["rgb"][:, seen], base["rgb"][:, seen])
    assert bool((base["rgb"][:, hole] == 2.0).all())
    lo, hi = base["rgb"][:, seen].amin(1), base["rgb"][:, seen].amax(1)
    assert float(hi.max()) <= 1.0 and float(lo.min()) >= 0.0
    slack = float(_push_bound(R, 1.0))
    inp = got["rgb"][:, hole]
    assert bool((inp >= lo[:, None] - slack).all()) and bool((inp <= hi[:, None] + slack).all())
    assert not bool((inp == base["rgb"][:, hole]).any())
    # no view at all: nothing to fill from, the fallback stays
    none = view_bake.bake_views(*args, fallback=fallback, unseen="inpaint", erode=1000)
    assert int(none["view_count"].sum()) == 0 and bool((none["rgb"][:, covered] == 2.0).all())
    # fill="pullpush" on top: the whole atlas, the covered texels and the gutter unchanged
    full = view_bake.bake_views(*args, fallback=fallback, unseen="inpaint", fill="pullpush")
    owned = got["mask"] > 0
    assert torch.equal(full["rgb"][:, owned], got["rgb"][:, owned]) and bool((full["mask"][~owned] == 3).all())
    assert float(full["rgb"].max()) <= float(got["rgb"][:, owned].max()) + slack


def test_latent_paint_export_fills_the_decoded_atlas(dev, tmp_path):
    import numpy as np
    from PIL import Image

    from src.latent_paint.models.render import texture_coverage
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    from tests.test_gpu_view_bake import _LinearGuidance
    torch.manual_seed(3)
    cfg = _paint_cfg(tmp_path, "paint", **{"guide.texture_interpolation_mode": "bilinear"})
    model = TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=True, texture_resolution=64)
    guidance = _LinearGuidance()
    plain = model.export_mesh(tmp_path / "plain", guidance=guidance)
    dilate = model.export_mesh(tmp_path / "dilate", guidance=guidance, fill="dilate", unseen="fallback")
    for name in ("albedo.png", "mesh.obj", "mesh.mtl"):
        assert (tmp_path / "dilate" / name).read_bytes() == (tmp_path / "plain" / name).read_bytes(), name
    assert torch.equal(plain["rgb"], dilate["rgb"])
    push = model.export_mesh(tmp_path / "push", guidance=guidance, fill="pullpush")
    covered = texture_coverage(model.mesh.vertices, model.mesh.faces, model.face_attributes[0], 64, ring=0)
    assert torch.equal(push["rgb"][:, covered], plain["rgb"][:, covered])
    assert not torch.equal(push["rgb"][:, ~covered], plain["rgb"][:, ~covered])
    lo, hi = plain["rgb"][:, covered].amin(1), plain["rgb"][:, covered].amax(1)
    slack = float(_push_bound(64, float(plain["rgb"].abs().max())))
    assert bool((push["rgb"] >= lo.view(3, 1, 1) - slack).all()) and bool((push["rgb"] <= hi.view(3, 1, 1) + slack).all())
    img = np.asarray(Image.open(tmp_path / "push" / "albedo.png"))
    assert np.array_equal(img, (push["rgb"].permute(1, 2, 0).clamp(0, 1).cpu().numpy() * 255).astype(np.uint8))
    with pytest.raises(ValueError, match="fill"):
        model.export_mesh(tmp_path / "bad", guidance=guidance, fill="push")
