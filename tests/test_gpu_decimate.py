"""Mesh decimation on the MI355X: lnerf_decimate against the numpy restatement (tests/decimate_reference.py: faces
equal, vertices and normals bit for bit, the same rounds and collapses) on marching-cubes meshes, repeatability, the
refusal of out-of-range face indices, and NeRFRenderer.export_mesh(target_faces=N) end to end (f32 and the bf16
`blocked` default, the textured variant at 1024^2, Latent-Paint starting from it, the trainer's log.mesh_target_faces)."""
import functools
import os
import re
import warnings

import numpy as np
import pytest
import torch

from tests import decimate_reference as D
from tests import mc_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _lattice(n):
    x = np.linspace(-1, 1, n, dtype=np.float32)
    return np.meshgrid(x, x, x, indexing="ij")


def _bipyramid():
    t = 2 * np.pi * np.arange(3) / 3
    v = np.concatenate([[[0, 0, 1], [0, 0, -1]], np.stack([np.cos(t), np.sin(t), 0 * t], -1)]).astype(np.float32)
    f = np.array([[0, 2, 3], [0, 3, 4], [0, 4, 2], [1, 3, 2], [1, 4, 3], [1, 2, 4]], np.int32)
    return v, f


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, target_faces, max_error)."""
    box = (-1, -1, -1), (1, 1, 1)
    if name == "sphere":
        X, Y, Z = _lattice(40)
        v, f, _ = R.marching_cubes((0.6 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), 0.0, *box)
        return v, f, 1000, np.inf
    if name == "torus":
        X, Y, Z = _lattice(48)
        v, f, _ = R.marching_cubes((0.2 - np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)).astype(np.float32),
                                   0.0, *box)
        return v, f, 1000, np.inf
    if name == "box":
        v, f, _ = R.marching_cubes(np.ones((5, 6, 7), np.float32), 0.0, (-1, -2, -3), (1, 2, 3))
        return v, f, 12, 1e-12
    if name == "noise":
        vol = np.random.default_rng(0).standard_normal((12, 12, 12)).astype(np.float32)
        v, f, _ = R.marching_cubes(vol, 0.0, (0, 0, 0), (1, 1, 1))
        return v, f, len(f) // 4, np.inf
    if name == "open":
        X, Y, Z = _lattice(32)
        v, f, _ = R.marching_cubes((0.8 - np.sqrt(X * X + Y * Y + (Z + 0.6) ** 2)).astype(np.float32), 0.0, *box,
                                   close_boundary=False)
        return v, f, 300, np.inf
    if name == "unchanged":
        v, f, _, _ = _case("sphere")
        return v, f, len(f), np.inf
    if name == "link":
        v, f = _bipyramid()
        return v, f, 0, np.inf
    if name == "bumpy":     # >= 10 k faces
        X, Y, Z = _lattice(64)
        sdf = 0.6 - np.sqrt(X * X + Y * Y + Z * Z) + 0.04 * np.sin(9 * X) * np.sin(9 * Y) * np.sin(9 * Z)
        v, f, _ = R.marching_cubes(sdf.astype(np.float32), 0.0, *box)
        return v, f, 2000, np.inf
    raise KeyError(name)


CASES = ["sphere", "torus", "box", "noise", "open", "unchanged", "link", "bumpy"]


def _op(dev, v, f, target, max_error=np.inf):
    from src.latent_nerf.raymarching import decimate_mesh
    st = {}
    ov, of, on = decimate_mesh(torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f)).to(dev), target,
                               max_error, stats=st)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), of.cpu().numpy(), on.cpu().numpy(), st


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", CASES)
def test_op_matches_restatement_bit_for_bit(dev, case):
    v, f, target, max_error = _case(case)
    if case == "bumpy":
        assert len(f) >= 10000
    gv, gf, gn, st = _op(dev, v, f, target, max_error)
    rv, rf, rn, info = D.decimate(v, f, target, max_error)
    assert np.array_equal(gf, rf)
    assert np.array_equal(_bits(gv), _bits(rv))
    assert np.array_equal(_bits(gn), _bits(rn))
    assert st == info
    if case in ("sphere", "torus", "bumpy"):
        assert len(gf) in (target, target - 1) and R.is_closed_oriented_manifold(gf)
    if case == "link":
        assert len(gf) == 4 and st["collapses"] == 1


def test_two_runs_are_identical(dev):
    v, f, target, _ = _case("bumpy")
    a, b = _op(dev, v, f, target), _op(dev, v, f, target)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)
    assert a[3] == b[3] and a[3]["rounds"] > 1


def test_out_of_range_indices_are_refused_without_a_fault(dev):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import decimate_mesh
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    v, f = _bipyramid()
    V, F = len(v), len(f)
    lib = B.get_lib()
    nbytes = lib.lnerf_decimate_scratch_bytes(V, F)
    assert nbytes > 0 and lib.lnerf_decimate_scratch_bytes(-1, F) == 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    counts = torch.zeros(4, dtype=torch.int64, device=dev)
    tv = torch.from_numpy(v).to(dev)
    out_v, out_n = torch.empty(V, 3, device=dev), torch.empty(V, 3, device=dev)
    out_f = torch.empty(F, 3, dtype=torch.int32, device=dev)
    for bad in (V, -1, 2 ** 31 - 1):
        fb = f.copy()
        fb[3, 1] = bad
        tf = torch.from_numpy(fb).to(dev)
        rc = lib.lnerf_decimate(_p(tv), V, _p(tf), F, 0, float("inf"), 8, _p(scratch), nbytes, _p(out_v), _p(out_f),
                                _p(out_n), _p(counts), _stream())
        assert rc == -1 and b"1 faces index outside" in lib.lnerf_last_error()
        with pytest.raises(B.LnerfError, match="outside"):
            decimate_mesh(tv, tf, 0)
    # bad faces in two different waves (faces 3 and 129 of 130) are counted together
    f130 = np.resize(f, (130, 3)).copy()
    f130[3, 1], f130[129, 0] = V, -1
    with pytest.raises(B.LnerfError, match="decimate: 2 faces index outside"):
        decimate_mesh(tv, torch.from_numpy(f130).to(dev), 0)
    with pytest.raises(ValueError):
        decimate_mesh(tv, torch.from_numpy(f).to(dev), -1)
    with pytest.raises(ValueError, match="no CPU path"):
        decimate_mesh(torch.from_numpy(v), torch.from_numpy(f), 0)
    gv, gf, _, st = _op(dev, v, f, 0)                                  # the device is fine afterwards
    assert len(gf) == 4 and st["collapses"] == 1


def _nerf(dev, precision, grid=32):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    kw = dict(grid_size=grid, train_h=16, train_w=16)
    if precision == "bf16":
        kw.update(mlp_precision="bf16", table_dtype="bf16", gridtype="blocked")
    cfg = RenderConfig(**kw)
    return NeRFNetwork(cfg, log2_hashmap_size=14).to(dev), cfg


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_export_mesh_decimated_end_to_end(dev, tmp_path, precision):
    from src.latent_nerf.raymarching import decimate_mesh
    from src.latent_paint.models.mesh import read_obj
    net, cfg = _nerf(dev, precision)
    full = net.export_mesh(str(tmp_path / "full"), resolution=64, S=32, thresh=cfg.density_thresh)
    F0 = int(full["faces"].shape[0])
    assert full["faces_before"] == F0 > 600
    N = F0 // 3
    out = net.export_mesh(str(tmp_path / "dec"), resolution=64, S=32, thresh=cfg.density_thresh, target_faces=N)
    assert out["faces_before"] == F0
    v, f, n = (out[k].cpu().numpy() for k in ("verts", "faces", "normals"))
    assert len(f) in (N, N - 1) and R.is_closed_oriented_manifold(f)
    # exactly the op on the marching-cubes mesh, and the colours are the field's at the decimated vertices
    dv, df, dn = decimate_mesh(full["verts"], full["faces"], N)
    assert np.array_equal(f, df.cpu().numpy()) and np.array_equal(_bits(v), _bits(dv.cpu().numpy()))
    assert np.array_equal(_bits(n), _bits(dn.cpu().numpy()))
    with torch.no_grad():
        _, feats = net.field(out["verts"].contiguous(), out["verts"].shape[0])
    assert torch.equal(out["colors"], net._latent_preview(feats))
    rv, rf, vt, _ = read_obj(str(tmp_path / "dec" / "mesh.obj"))
    assert rf.shape[0] in (N, N - 1) and vt is None
    assert np.array_equal(rv.numpy(), v) and np.array_equal(rf.numpy(), f.astype(np.int64))


def _bench_field(dev):
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mesh_export", os.path.join(ROOT, "tools", "bench_mesh_export.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.field(dev, "bf16")


def test_textured_512_export_decimated_bakes_without_the_atlas_warning(dev, tmp_path):
    from src.latent_paint.models.mesh import read_obj
    from src.uv_atlas import atlas_min_resolution
    net, cfg = _bench_field(dev)
    N = 20000
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        out = net.export_mesh(str(tmp_path), resolution=512, S=128, thresh=cfg.density_thresh, texture_resolution=1024,
                              target_faces=N)
    assert atlas_min_resolution(out["faces_before"]) > 1024          # undecimated, this mesh would warn at 1024^2
    assert not [w for w in caught if "texture_resolution" in str(w.message)]
    assert out["faces"].shape[0] in (N, N - 1) and out["texture"].shape == (4, 1024, 1024)
    v, f, vt, ft = read_obj(str(tmp_path / "mesh.obj"))
    assert f.shape[0] in (N, N - 1) and vt is not None and ft.shape == f.shape
    assert (tmp_path / "latent_texture.pt").exists()


def test_latent_paint_starts_from_the_decimated_export(dev, tmp_path):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.models.mesh import read_obj
    from src.latent_paint.training.trainer import Trainer
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    cfg = RenderConfig(grid_size=32, train_h=16, train_w=16, nerf_type=NeRFType("latent"))
    net = NeRFNetwork(cfg, log2_hashmap_size=14).to(dev)
    Rt = 256
    out = net.export_mesh(str(tmp_path / "nerf"), resolution=40, S=32, thresh=cfg.density_thresh, texture_resolution=Rt,
                          target_faces=0)
    N = out["faces"].shape[0] // 2
    out = net.export_mesh(str(tmp_path / "nerf"), resolution=40, S=32, thresh=cfg.density_thresh, texture_resolution=Rt,
                          target_faces=N)
    assert out["faces"].shape[0] in (N, N - 1) and out["faces_before"] > N
    lt = torch.load(tmp_path / "nerf" / "latent_texture.pt", weights_only=True)
    flat = {"log.exp_name": "paint", "log.exp_root": str(tmp_path), "guide.text": "a goldfish",
            "guide.shape_path": str(tmp_path / "nerf" / "mesh.obj"),
            "guide.init_texture": str(tmp_path / "nerf" / "latent_texture.pt"),
            "guide.texture_resolution": Rt, "guide.texture_interpolation_mode": "bilinear", "optim.iters": 1,
            "log.save_interval": 100, "log.eval_size": 1, "log.full_eval_size": 1, "render.eval_grid_size": 64,
            "log.save_mesh": False}
    tr = Trainer(apply_overrides(TrainConfig(), flat).validate(), device=dev)
    assert torch.equal(tr.mesh_model.texture_img.detach().cpu(), lt[None])
    _, f, vt, ft = read_obj(str(tmp_path / "nerf" / "mesh.obj"))
    assert f.shape[0] in (N, N - 1)
    assert torch.equal(tr.mesh_model.vt.cpu(), vt) and torch.equal(tr.mesh_model.ft.cpu(), ft)
    tr.train()
    assert tr.train_step == 1


def test_trainer_log_mesh_target_faces(dev, tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    from src.latent_paint.models.mesh import read_obj
    N = 400
    flat = {"log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32, "render.eval_h": 32,
            "render.eval_w": 32, "render.grid_size": 32, "optim.iters": 4, "log.save_interval": 100,
            "log.eval_size": 1, "log.full_eval_size": 2, "optim.fp16": False, "guide.text": "a lego man",
            "log.exp_name": "d", "log.save_mesh": True, "log.mesh_target_faces": N}
    tr = Trainer(apply_overrides(TrainConfig(), flat), device=dev)
    assert tr.cfg.log.mesh_target_faces == N
    tr.train()
    _, f, _, _ = read_obj(str(tr.exp_path / "mesh" / "mesh.obj"))
    m = re.search(r"(\d+) triangles; (\d+) before decimation", (tr.exp_path / "log.txt").read_text())
    assert m is not None
    after, before = int(m.group(1)), int(m.group(2))
    assert f.shape[0] == after > 0 and after <= before
    if before > N:
        assert after < before
