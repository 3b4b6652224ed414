"""Mesh export on the MI355X: lnerf_marching_cubes against the numpy restatement (tests/mc_reference.py: faces equal,
vertices bit for bit), its edge cases and geometry, a real shape (teddy's winding-number grid), NeRFRenderer.export_mesh
end to end (f32 and the bf16 `blocked` default) and the trainer's `log.save_mesh`."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from tests import mc_reference as R

pytestmark = pytest.mark.gpu

TEDDY = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes", "teddy.obj")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _mc(vol, iso, lo, hi, close=True):
    from src.latent_nerf.raymarching import marching_cubes
    v, f, n = marching_cubes(vol, iso, lo, hi, close_boundary=close)
    torch.cuda.synchronize()
    return v.cpu().numpy(), f.cpu().numpy(), n.cpu().numpy()


def _grid(shape, lo, hi):
    axes = [np.float32(lo[a]) + ((np.float32(hi[a]) - np.float32(lo[a])) * np.arange(shape[a], dtype=np.float32))
            / np.float32(shape[a] - 1) for a in range(3)]
    return np.meshgrid(*axes, indexing="ij")


@functools.lru_cache(maxsize=None)
def _volumes():
    rng = np.random.default_rng(5)
    X, Y, Z = _grid((32, 32, 32), (-1, -1, -1), (1, 1, 1))
    sphere = (0.55 - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    torus = (0.2 - np.sqrt((np.sqrt(X * X + Y * Y) - 0.55) ** 2 + Z * Z)).astype(np.float32)
    noise = rng.standard_normal((24, 24, 24)).astype(np.float32)
    X2, Y2, Z2 = _grid((40, 57, 33), (-1.0, -0.5, 0.0), (1.0, 2.0, 0.75))
    aniso = (np.sin(3 * X2) * np.cos(2 * Y2) + 0.8 * Z2 - 0.3).astype(np.float32)
    ties = rng.integers(0, 3, (17, 13, 19)).astype(np.float32)       # many values exactly at iso 1
    ties[3, 4, 5] = np.nan
    # a plane through 1088 blocks of points (closed; 1039 open): over 1024, a thread of the top-level scan owns two
    slab = (np.float32(0.31) - _grid((62, 254, 270), (-1, -1, -1), (1, 1, 1))[0]).astype(np.float32)
    return [("sphere", sphere, 0.0, (-1, -1, -1), (1, 1, 1)),
            ("torus", torus, 0.0, (-1, -1, -1), (1, 1, 1)),
            ("noise", noise, 0.1, (0, 0, 0), (1, 1, 1)),
            ("aniso", aniso, 0.0, (-1.0, -0.5, 0.0), (1.0, 2.0, 0.75)),
            ("ties", ties, 1.0, (0, 0, 0), (2, 3, 4)),
            ("slab", slab, 0.0, (-1, -1, -1), (1, 1, 1))]


@pytest.mark.parametrize("close", [True, False])
@pytest.mark.parametrize("case", [c[0] for c in _volumes()])
def test_op_matches_restatement_bit_for_bit(dev, case, close):
    name, vol, iso, lo, hi = [c for c in _volumes() if c[0] == case][0]
    v, f, n = _mc(torch.from_numpy(vol).to(dev), iso, lo, hi, close)
    rv, rf, rn = R.marching_cubes(vol, iso, lo, hi, close_boundary=close)
    assert len(f) > 0
    if case == "slab":
        assert np.prod(np.add(vol.shape, 2 if close else 0)) > 1024 * 4096          # over 1024 blocks either way
        assert (len(rv), len(rf)) == ((179080, 358156) if close else (68580, 136114))
    assert np.array_equal(f, rf)
    assert v.shape == rv.shape and np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    ok = np.isfinite(rn).all(1)
    assert np.abs(n[ok] - rn[ok]).max() <= 1e-6
    if close:
        assert R.is_closed_oriented_manifold(f)
    v2, f2, n2 = _mc(torch.from_numpy(vol).to(dev), iso, lo, hi, close)
    assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(f, f2)
    assert np.array_equal(n.view(np.uint32), n2.view(np.uint32))


def test_empty_and_all_inside(dev):
    v, f, n = _mc(torch.zeros(8, 9, 10, device=dev), 0.5, (0, 0, 0), (1, 1, 1))
    assert v.shape == (0, 3) and f.shape == (0, 3)
    ones = torch.ones(8, 9, 10, device=dev)
    v, f, n = _mc(ones, 0.5, (0, 0, 0), (1, 1, 1), close=False)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    v, f, n = _mc(ones, 0.5, (-1, -2, -3), (1, 2, 3))
    assert R.is_closed_oriented_manifold(f)
    assert np.array_equal(v.min(0), np.float32([-1, -2, -3])) and np.array_equal(v.max(0), np.float32([1, 2, 3]))
    assert abs(R.signed_volume(v, f) - 48.0) < 1e-3
    rv, rf, _ = R.marching_cubes(np.ones((8, 9, 10), np.float32), 0.5, (-1, -2, -3), (1, 2, 3))
    assert np.array_equal(f, rf) and np.array_equal(v, rv)


def test_undersized_buffers_report_true_counts_and_stay_in_bounds(dev):
    from src.latent_nerf.raymarching import backend as _b
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    name, vol, iso, lo, hi = _volumes()[0]
    rv, rf, rn = R.marching_cubes(vol, iso, lo, hi)
    V, F = len(rv), len(rf)
    t = torch.from_numpy(vol).to(dev)
    nb = _b.get_lib().lnerf_marching_cubes_scratch_bytes(*vol.shape, _b.MC_CLOSE_BOUNDARY)
    scratch = torch.empty(nb, device=dev, dtype=torch.uint8)
    counts = torch.zeros(2, device=dev, dtype=torch.int64)
    mv, mf, guard = V // 3, F // 2, 4096
    sentinel = -7.0
    verts = torch.full((mv + guard, 3), sentinel, device=dev)
    normals = torch.full((mv + guard, 3), sentinel, device=dev)
    faces = torch.full((mf + guard, 3), -7, device=dev, dtype=torch.int32)
    _b.call("lnerf_marching_cubes", _p(t), *vol.shape, float(iso), *[float(x) for x in lo], *[float(x) for x in hi],
            _b.MC_CLOSE_BOUNDARY, _p(scratch), nb, _p(verts), _p(normals), mv, _p(faces), mf, _p(counts), _stream())
    torch.cuda.synchronize()
    assert counts.tolist() == [V, F]
    assert np.array_equal(verts[:mv].cpu().numpy(), rv[:mv]) and np.array_equal(faces[:mf].cpu().numpy(), rf[:mf])
    assert bool((verts[mv:] == sentinel).all()) and bool((normals[mv:] == sentinel).all())
    assert bool((faces[mf:] == -7).all())
    # count only: nothing written at all
    verts.fill_(sentinel)
    counts.zero_()
    _b.call("lnerf_marching_cubes", _p(t), *vol.shape, float(iso), *[float(x) for x in lo], *[float(x) for x in hi],
            _b.MC_CLOSE_BOUNDARY | _b.MC_COUNT_ONLY, _p(scratch), nb, _p(verts), None, mv, None, 0, _p(counts),
            _stream())
    torch.cuda.synchronize()
    assert counts.tolist() == [V, F] and bool((verts == sentinel).all())
    # argument validation: -1 with a message
    lib = _b.get_lib()
    rc = lib.lnerf_marching_cubes(_p(t), 1, 2, 2, 0.0, 0., 0., 0., 1., 1., 1., 0, _p(scratch), nb, None, None, 0, None, 0,
                                  _p(counts), _stream())
    assert rc == -1 and b"lattice" in lib.lnerf_last_error()
    rc = lib.lnerf_marching_cubes(_p(t), *vol.shape, 0.0, 0., 0., 0., 1., 1., 1., 1, _p(scratch), 16, None, None, 0,
                                  None, 0, _p(counts), _stream())
    assert rc == -1 and b"scratch" in lib.lnerf_last_error()
    with pytest.raises(ValueError):
        from src.latent_nerf.raymarching import marching_cubes
        marching_cubes(torch.from_numpy(vol), iso, lo, hi)     # CPU tensor: no CPU path


def test_sphere_geometry_at_128(dev):
    r = 0.6
    X, Y, Z = _grid((128,) * 3, (-1, -1, -1), (1, 1, 1))
    vol = (r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32)
    v, f, n = _mc(torch.from_numpy(vol).to(dev), 0.0, (-1, -1, -1), (1, 1, 1))
    h = 2.0 / 127
    rad = np.linalg.norm(v.astype(np.float64), axis=1)
    assert np.abs(rad - r).max() < h
    vol_mesh = R.signed_volume(v, f)
    ref = 4.0 / 3.0 * math.pi * r ** 3
    assert vol_mesh > 0 and abs(vol_mesh - ref) < 0.01 * ref
    assert R.is_closed_oriented_manifold(f) and R.euler_characteristic(v, f) == 2
    assert (np.einsum("ij,ij->i", n, v) > 0.99 * rad).all()      # unit normals along the radius, outward


def test_teddy_winding_grid_round_trips(dev):
    from src.latent_nerf.training import shape as S
    verts, faces = S.load_obj(TEDDY)
    verts = S.normalize_mesh(verts, target_scale=0.7, dy=0.0)
    Rz = 128
    occ = S.MeshOccupancy(verts, faces, dev, bound=1.0, resolution=Rz)
    wind = occ.winding[0, 0].permute(2, 1, 0).contiguous()        # (z, y, x) -> (x, y, z)
    c0, c1 = -1 + 1.0 / Rz, 1 - 1.0 / Rz                            # first and last voxel centre
    from src.latent_nerf.raymarching import marching_cubes
    v, f, _ = marching_cubes(wind, 0.5, (c0,) * 3, (c1,) * 3)
    assert f.shape[0] > 1000 and R.is_closed_oriented_manifold(f.cpu().numpy())
    h = 2.0 / Rz
    d_out = S.mesh_distance(v.contiguous(), occ.triangles)
    assert float((d_out < h).float().mean()) >= 0.99
    # the other way round for teddy's OUTER surface: teddy's parts interpenetrate (winding numbers up to 3), and a
    # vertex buried inside another part (winding > 1 at the vertex) lies on no iso-0.5 surface
    tv = verts.float().to(dev).contiguous()
    outer = S.mesh_winding_number(tv, occ.triangles) < 1.0
    assert int(outer.sum()) > 0.75 * tv.shape[0]
    d_in = S.mesh_distance(tv[outer].contiguous(), v[f.long()].contiguous())
    assert float(d_in.max()) < 2 * h


def _nerf(dev, precision):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(11)
    if precision == "f32":
        cfg = RenderConfig(grid_size=32, train_h=16, train_w=16)
    else:
        cfg = RenderConfig(grid_size=32, train_h=16, train_w=16, mlp_precision="bf16", table_dtype="bf16",
                           gridtype="blocked")
    net = NeRFNetwork(cfg, log2_hashmap_size=14).to(dev)
    return net, cfg


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_export_mesh_end_to_end(dev, tmp_path, precision):
    from src.latent_paint.models.mesh import read_obj
    net, cfg = _nerf(dev, precision)
    Rl = 64
    vol = net.density_lattice(Rl, S=32)
    # the lattice against the oracle's sigma_latent_mlp(grid_encode(...))
    X, Y, Z = _grid((Rl,) * 3, (-1, -1, -1), (1, 1, 1))
    xyz = torch.from_numpy(np.stack([X, Y, Z], -1).reshape(-1, 3))
    lv = O.make_grid_levels(16, 2, 16, 2048, 14, blocked=precision == "bf16")
    table = net.encoder.embeddings.detach().cpu().float()
    if precision == "bf16":
        table = table.bfloat16().float()
    params = {k: getattr(net, k).detach().cpu() for k in ("w1", "b1", "w2", "b2", "w3", "b3")}
    with torch.no_grad():
        feat = O.grid_encode((xyz + 1.0) / 2.0, table, lv)
        sig, _ = O.sigma_latent_mlp(feat, xyz, params, bf16=precision == "bf16")
    e = float((vol.cpu().reshape(-1) - sig).abs().max())
    s = float(sig.abs().max())
    assert e <= (5e-4 * s if precision == "bf16" else 1e-4 * s + 1e-5), (e, s)
    # export: the blob makes a closed surface around the origin at density_thresh
    out = net.export_mesh(str(tmp_path), resolution=Rl, S=32, thresh=cfg.density_thresh)
    v, f = out["verts"].cpu().numpy(), out["faces"].cpu().numpy()
    rv, rf, _ = R.marching_cubes(vol.cpu().numpy(), cfg.density_thresh, (-1, -1, -1), (1, 1, 1))
    assert np.array_equal(f, rf) and np.array_equal(v.view(np.uint32), rv.view(np.uint32))
    assert len(f) > 100 and R.is_closed_oriented_manifold(f) and R.signed_volume(v, f) > 0
    assert np.abs(v).max() < 0.9                                    # a blob, not the box
    assert float(vol[Rl // 2, Rl // 2, Rl // 2]) > cfg.density_thresh
    c = out["colors"]
    assert c.shape == out["verts"].shape and float(c.min()) >= 0 and float(c.max()) <= 1
    rv2, rf2, vt, _ = read_obj(os.path.join(str(tmp_path), "mesh.obj"))
    assert out["path"] == os.path.join(str(tmp_path), "mesh.obj")
    assert np.array_equal(rv2.numpy(), v) and np.array_equal(rf2.numpy(), f.astype(np.int64)) and vt is None
    # the default iso is min(mean density, density_thresh)
    net.mean_density_dev.fill_(3.0)
    out2 = net.export_mesh(str(tmp_path / "d"), resolution=32, S=16)
    assert out2["iso"] == 3.0 and out2["faces"].shape[0] > 0


def test_trainer_save_mesh(dev, tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    flat = {"log.exp_root": str(tmp_path), "render.train_h": 32, "render.train_w": 32, "render.eval_h": 32,
            "render.eval_w": 32, "render.grid_size": 32, "optim.iters": 4, "log.save_interval": 100,
            "log.eval_size": 1, "log.full_eval_size": 2, "optim.fp16": False, "guide.text": "a lego man"}
    tr = Trainer(apply_overrides(TrainConfig(), dict(flat, **{"log.exp_name": "m", "log.save_mesh": True})), device=dev)
    tr.train()
    obj = tr.exp_path / "mesh" / "mesh.obj"
    assert obj.exists()
    from src.latent_paint.models.mesh import read_obj
    v, f, _, _ = read_obj(str(obj))
    assert v.shape[0] > 0 and f.shape[0] > 0
    tr2 = Trainer(apply_overrides(TrainConfig(), dict(flat, **{"log.exp_name": "n"})), device=dev)
    tr2.train()
    assert not (tr2.exp_path / "mesh").exists()
    before = sorted(p.relative_to(tr2.exp_path) for p in tr2.exp_path.rglob("*"))
    tr2.full_eval()
    after = sorted(p.relative_to(tr2.exp_path) for p in tr2.exp_path.rglob("*"))
    assert before == after
