"""Geometry learning of the Latent-Paint path (optim.disp_lr, render.antialias) from the model up to the trainer: off by
default bit for bit, a descent direction under an image loss, a short fit, and a trainer run with its checkpoints."""
import math
import os

import pytest
import torch

from tests import raster_batch_reference as R

pytestmark = pytest.mark.gpu
GEOMETRY = {"optim.disp_lr": 5e-5, "render.antialias": True, "guide.texture_interpolation_mode": "bilinear"}
VIEWS = ([math.radians(70.0), math.radians(95.0), math.radians(60.0), math.radians(110.0)],
         [0.3, 1.9, 3.4, 5.0], [1.3, 1.2, 1.4, 1.25])


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _cfg(tmp_path, shape=None, **over):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "geo", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": shape or os.path.join(R.SHAPES, "blub.obj")}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat).validate()


def _model(cfg, dev, side):
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    return TexturedMeshModel(cfg, device=dev, render_grid_size=side, latent_mode=True,
                             texture_resolution=cfg.guide.texture_resolution).to(dev)


# ------------------------------------------------------------------------------------------------ defaults
def test_defaults_equal_the_composition_of_the_public_renderer_calls(dev, tmp_path):
    torch.manual_seed(0)
    cfg = _cfg(tmp_path, **{"guide.texture_resolution": 32})
    m = _model(cfg, dev, 64)
    assert sorted(m.state_dict()) == ["background_sphere_colors", "texture_img", "texture_img_rgb_finetune"]
    theta, phi, rad = VIEWS[0][:2], VIEWS[1][:2], VIEWS[2][:2]
    out = m.render(theta, phi, rad)
    assert set(out) == {"image", "mask", "background", "foreground"}
    view = dict(elev=theta, azim=phi, radius=rad, look_at_height=m.dy)
    fg, cov = m.renderer.render_views_texture(m.mesh.vertices, m.mesh.faces, m.face_attributes, m.texture_img, **view)
    bg, _ = m.renderer.render_views(m.env_sphere, m.background_sphere_colors, **view)
    assert torch.equal(out["foreground"], fg) and torch.equal(out["mask"], cov) and torch.equal(out["background"], bg)
    assert torch.equal(out["image"], bg * (1 - cov) + fg * cov)
    decode = lambda t: t[:, :3] * 0.5 + 0.25
    test = m.render(theta, phi, rad, decode_func=decode, test=True, dims=(48, 40))
    img, cov = m.renderer.render_views_texture(m.mesh.vertices, m.mesh.faces, m.face_attributes, decode(m.texture_img),
                                               dims=(48, 40), white_background=True, **view)
    assert torch.equal(test["image"], img) and torch.equal(test["mask"], cov)
    # the exported mesh holds the mesh's own vertices, printed as before
    m.latent_mode = False
    m.export_mesh(tmp_path / "mesh")
    lines = (tmp_path / "mesh" / "mesh.obj").read_text().split("\n")
    v = m.mesh.vertices.cpu().numpy()
    assert lines[1:1 + len(v)] == ["v %s %s %s" % (p[0], p[1], p[2]) for p in v]


# ------------------------------------------------------------------------------------------------ descent and fit
@pytest.fixture(scope="module")
def sphere(dev, tmp_path_factory):
    """A geometry-learning model on make_icosphere(2, 0.5) at 32 x 32 with a 16 x 16 bilinear texture, and the target:
    the antialiased image and mask of the same sphere scaled 1.25 along x, 4 views."""
    from src.latent_nerf.training.shape import make_icosphere
    from src.latent_paint.training.trainer import Trainer
    tmp = tmp_path_factory.mktemp("sphere")
    v, f = make_icosphere(2, 0.5)
    obj = tmp / "sphere.obj"
    obj.write_text("".join("v %r %r %r\n" % tuple(p.tolist()) for p in v)
                   + "".join("f %d %d %d\n" % tuple((t + 1).tolist()) for t in f))
    torch.manual_seed(1)
    cfg = _cfg(tmp, shape=str(obj), **{**GEOMETRY, "optim.disp_lr": 2e-3, "guide.texture_resolution": 16,
                                        "guide.shape_scale": 0.5, "render.train_grid_size": 32, "render.batch_size": 4})
    tr = Trainer(cfg, device=dev)
    m = tr.mesh_model
    own = m.mesh.vertices.clone()
    with torch.no_grad():
        m.mesh.vertices = own * torch.tensor([1.25, 1.0, 1.0], device=own.device)
        target = m.render(*VIEWS)
        m.mesh.vertices = own

    def loss_of(out):
        return (out["image"] - target["image"]).square().mean() + (out["mask"] - target["mask"]).square().mean()

    def iou(out):
        a, b = out["mask"].clamp(0, 1), target["mask"].clamp(0, 1)
        return float(torch.minimum(a, b).sum() / torch.maximum(a, b).sum())

    return tr, loss_of, iou


def test_a_quarter_pixel_step_against_the_gradient_lowers_the_loss(sphere):
    tr, loss_of, _ = sphere
    m = tr.mesh_model
    with torch.no_grad():
        m.displacement.zero_()
    loss0 = loss_of(m.render(*VIEWS))
    (g,) = torch.autograd.grad(loss0, m.displacement)
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    quarter_pixel = 0.25 * (2.0 / 32) * 1.2 / (1.0 / math.tan(math.pi / 6))   # in world units at the nearest camera
    with torch.no_grad():
        m.displacement.add_(g * (-quarter_pixel / float(g.norm(dim=1).max())))
        loss1 = loss_of(m.render(*VIEWS))
        m.displacement.zero_()
    print("descent: loss %.6g -> %.6g" % (float(loss0.detach()), float(loss1)))
    assert float(loss1) < float(loss0.detach())


def test_fifty_steps_of_the_trainers_optimiser_fit_the_target(sphere):
    tr, loss_of, iou = sphere
    m = tr.mesh_model
    with torch.no_grad():
        m.displacement.zero_()
        first = m.render(*VIEWS)
        loss0, iou0 = float(loss_of(first)), iou(first)
    for _ in range(50):
        tr.optimizer.zero_grad()
        out = m.render(*VIEWS)
        (loss_of(out) + out["geometry_loss"]).backward()
        tr.optimizer.step()
    with torch.no_grad():
        last = m.render(*VIEWS)
        loss1, iou1 = float(loss_of(last)), iou(last)
    print("fit: loss %.6g -> %.6g (ratio %.4f), mask IoU %.4f -> %.4f" % (loss0, loss1, loss1 / loss0, iou0, iou1))
    assert loss1 < loss0 and iou1 > iou0
    assert bool(torch.isfinite(m.displacement).all()) and float(m.displacement.detach().abs().max()) > 0


# ------------------------------------------------------------------------------------------------ the trainer
def test_trainer_learns_offsets_checkpoints_them_and_exports_the_displaced_mesh(dev, tmp_path):
    from src.latent_paint.training.trainer import Trainer
    over = {**GEOMETRY, "optim.iters": 3, "log.save_interval": 3, "log.eval_size": 1, "log.full_eval_size": 1,
            "render.eval_grid_size": 64, "guide.texture_resolution": 32}
    tr = Trainer(_cfg(tmp_path, **over), device=dev)
    assert len(tr.optimizer.small) == 3 and tr.optimizer.small[2][3] == pytest.approx(5e-5)
    tr.train()
    d = tr.mesh_model.displacement.detach().clone()
    assert tr.train_step == 3 and bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0
    assert float(d.abs().max()) < 1e-3                                    # three Adam steps at 5e-5
    state = torch.load(tr.ckpt_path / "step_000003.pth", map_location="cpu", weights_only=True)
    assert torch.equal(state["model"]["displacement"], d.cpu())
    obj = (tmp_path / "geo" / "mesh" / "mesh.obj").read_text().split("\n")
    moved = (tr.mesh_model.mesh.vertices + d).cpu().numpy()
    assert obj[1:1 + len(moved)] == ["v %s %s %s" % (p[0], p[1], p[2]) for p in moved]
    # a resumed run loads the offsets and the optimiser state, and continues
    tr2 = Trainer(_cfg(tmp_path, **{**over, "optim.iters": 5, "optim.resume": True}), device=dev)
    assert torch.equal(tr2.mesh_model.displacement.detach(), d) and tr2.train_step == 4
    assert tr2.optimizer.step_no == 3
    tr2.train()
    assert tr2.train_step == 5 and not torch.equal(tr2.mesh_model.displacement.detach(), d)
    # a checkpoint without offsets starts a geometry run from zero offsets, and says so
    plain = {k: v for k, v in state["model"].items() if k != "displacement"}
    torch.save(plain, tmp_path / "plain.pth")
    tr3 = Trainer(_cfg(tmp_path / "b", **{**over, "optim.ckpt": str(tmp_path / "plain.pth")}), device=dev)
    assert float(tr3.mesh_model.displacement.detach().abs().max()) == 0.0
    assert "no vertex offsets" in (tmp_path / "b" / "geo" / "log.txt").read_text()
