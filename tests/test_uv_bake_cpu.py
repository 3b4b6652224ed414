"""Texture baking without a GPU: the numpy restatement of lnerf_uv_raster / lnerf_uv_dilate (tests/uv_reference.py) on
cases whose answer is known, the shared per-triangle atlas, the textured OBJ writer and the configuration surface."""
import math
import os

import numpy as np
import pytest
import torch

from tests import uv_reference as U

BLUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes", "blub.obj")


def _square():
    verts = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float32)
    faces = np.array([[0, 1, 2], [0, 2, 3]], np.int64)
    return verts, faces, verts[:, :2].copy(), faces.copy()


@pytest.mark.parametrize("R", [1, 7, 8, 33])
def test_unit_square_is_covered_once_and_the_diagonal_goes_to_the_higher_face(R):
    verts, faces, vt, ft = _square()
    tf, idx, pos, n_items, n_bad = U.uv_raster(verts, faces, vt, ft, R)
    count, per_face = U.coverage_count(verts, faces, vt, ft, R)
    i, j = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    diag = (i + j) == R - 1                                           # texel centres on u = v
    assert n_bad == 0 and (tf >= 0).all() and np.array_equal(idx, np.arange(R * R))
    assert np.array_equal(count, np.where(diag, 2, 1))
    assert (tf[diag] == 1).all()
    # face 0 = (0,0), (1,0), (1,1): the half below the diagonal (v < u)
    u, v = (j + 0.5) / R, 1 - (i + 0.5) / R
    assert np.array_equal(tf[~diag], np.where(v < u, 0, 1)[~diag])
    # the surface point of texel (i, j) is (u, v, 0)
    assert np.abs(pos[:, 0] - u.reshape(-1)).max() < 1e-6 and np.abs(pos[:, 1] - v.reshape(-1)).max() < 1e-6
    assert (pos[:, 2] == 0).all()
    assert n_items == sum(per_face_box(verts, faces, vt, ft, R))


def per_face_box(verts, faces, vt, ft, R):
    _, _, _, (_, _, w, h), _ = U.face_setup(verts, faces, vt, ft, R)
    return (w * h).tolist()


def test_candidate_box_is_padded_by_one_texel_and_clipped():
    verts, faces, vt, ft = _square()
    # the full square at R = 8: corners X in {0, 8}: floor(0) - 1 = -1 -> 0, floor(8) + 1 = 9 -> 7
    assert per_face_box(verts, faces, vt, ft, 8) == [64, 64]
    small = np.array([[0.3, 0.3], [0.45, 0.3], [0.3, 0.45]], np.float32)
    _, _, _, (j0, i0, w, h), _ = U.face_setup(verts[:3], faces[:1], small, np.array([[0, 1, 2]]), 10)
    # X in [3, 4.5] -> columns 2 .. 5; Y = (1 - v) * 10 in [5.5, 7] -> rows 4 .. 8
    assert (j0[0], i0[0], w[0], h[0]) == (2, 4, 4, 5)


def test_degenerate_nan_and_out_of_range_faces_cover_nothing():
    verts, faces, vt, ft = _square()
    vt_bad = np.concatenate([vt, [[0.5, 0.5], [np.nan, 0.2]]]).astype(np.float32)
    faces2 = np.array([[0, 1, 2], [0, 1, 2], [0, 1, 2], [0, 1, 9]])
    ft2 = np.array([[4, 4, 4], [0, 1, 5], [0, 1, 2], [0, 1, 2]])     # degenerate, NaN, fine, vertex out of range
    tf, idx, pos, _, n_bad = U.uv_raster(verts, faces2, vt_bad, ft2, 16)
    assert n_bad == 1
    assert set(np.unique(tf).tolist()) <= {-1, 2}
    assert (tf >= 0).sum() == len(idx) > 0
    _, per_face = U.coverage_count(verts, faces2, vt_bad, ft2, 16)
    assert per_face.tolist()[:2] == [0, 0] and per_face[3] == 0


@pytest.mark.parametrize("F", [1, 2, 11, 500, 5760])
def test_per_triangle_atlas_charts_each_cover_a_texel_and_never_share_one(F):
    from src.uv_atlas import atlas_cells, atlas_min_resolution, per_triangle_atlas
    vt, ft = per_triangle_atlas(F, "cpu")
    n = atlas_cells(F)
    assert n == int(math.ceil(math.sqrt((F + 1) // 2))) and atlas_min_resolution(F) == 4 * n
    verts = np.zeros((3 * F, 3), np.float32)
    for R in (atlas_min_resolution(F), atlas_min_resolution(F) + 3, 6 * n + 1):
        count, per_face = U.coverage_count(verts, ft.numpy(), vt.numpy(), ft.numpy(), R)
        assert per_face.min() >= 1, (F, R)
        assert count.max() <= 1, (F, R)


def test_per_triangle_atlas_keeps_its_old_import_path():
    from src.latent_paint.models.textured_mesh import per_triangle_atlas as old
    from src.uv_atlas import per_triangle_atlas
    assert old is per_triangle_atlas


def test_barycentrics_sum_to_one_and_reproduce_the_point():
    from src.latent_paint.models.mesh import read_obj
    v, f, vt, ft = (x.numpy() for x in read_obj(BLUB))
    R = 128
    tf, idx, pos, _, _ = U.uv_raster(v, f, vt, ft, R)
    assert len(idx) > 0.3 * R * R
    b0, b1, b2 = U.barycentrics(v, f, vt, ft, R, idx, tf)
    assert np.abs(b0.astype(np.float64) + b1 + b2 - 1).max() < 1e-6
    g = tf.reshape(-1)[idx]
    b = np.stack([b0, b1, b2], 1).astype(np.float64)
    P = v[f[g]].astype(np.float64)
    assert np.abs((b[:, :, None] * P).sum(1) - pos).max() < 1e-5
    # ... and the texture coordinates they interpolate are the texel centre's
    T = vt[ft[g]].astype(np.float64)
    uv = (b[:, :, None] * T).sum(1)
    i, j = idx // R, idx % R
    assert np.abs(uv[:, 0] - (j + 0.5) / R).max() < 1e-5 and np.abs(uv[:, 1] - (1 - (i + 0.5) / R)).max() < 1e-5


def test_dilation_rounds():
    rng = np.random.default_rng(3)
    C, R = 3, 24
    tex = np.zeros((C, R, R), np.float32)
    mask = np.zeros((R, R), np.uint8)
    mask[8:12, 9:14] = 2
    mask[5, 5] = 2
    tex[:, mask == 2] = rng.standard_normal((C, int((mask == 2).sum()))).astype(np.float32)
    one, m1 = U.uv_dilate(tex, mask, 1)
    assert np.array_equal(one[:, mask == 2], tex[:, mask == 2]) and (m1[mask == 2] == 2).all()
    full = mask != 0
    ring = np.zeros_like(full)
    for di, dj in U.NEIGHBOURS:
        ring |= np.roll(np.roll(np.pad(full, 1), di, 0), dj, 1)[1:-1, 1:-1]
    ring &= ~full
    assert np.array_equal(m1 == 1, ring) and (m1[~ring & ~full] == 0).all()
    for i, j in zip(*np.nonzero(ring)):
        nb = [tex[:, i + di, j + dj] for di, dj in U.NEIGHBOURS
              if 0 <= i + di < R and 0 <= j + dj < R and full[i + di, j + dj]]
        assert np.allclose(one[:, i, j], np.mean(nb, 0), rtol=1e-6, atol=1e-7)
    three, m3 = U.uv_dilate(tex, mask, 3)
    assert np.array_equal(three[:, mask == 2], tex[:, mask == 2])
    far = np.ones((R, R), bool)                 # Chebyshev distance > 3 from every covered texel
    for i, j in zip(*np.nonzero(full)):
        far[max(0, i - 3):i + 4, max(0, j - 3):j + 4] = False
    assert far.any() and (m3[far] == 0).all() and (three[:, far] == 0).all()
    assert (m3[~far & ~full] == 1).all()
    assert np.array_equal(U.uv_dilate(tex, mask, 0)[0], tex)


def test_textured_obj_reads_back(tmp_path):
    from src.latent_nerf.models.mesh_io import write_textured_obj
    from src.latent_paint.models.mesh import read_obj
    from src.uv_atlas import per_triangle_atlas
    rng = np.random.default_rng(0)
    v = rng.standard_normal((40, 3)).astype(np.float32)
    f = rng.integers(0, 40, (31, 3))
    vt, ft = per_triangle_atlas(31, "cpu")
    vt = vt.numpy()
    vt[0] = [np.float32(1) / np.float32(3), np.nextafter(np.float32(0.5), np.float32(1))]
    n = rng.standard_normal((40, 3)).astype(np.float32)
    out = write_textured_obj(str(tmp_path / "m" / "mesh.obj"), v, f, vt, ft.numpy(), n)
    rv, rf, rvt, rft = read_obj(out)
    assert np.array_equal(rv.numpy().view(np.uint32), v.view(np.uint32))
    assert np.array_equal(rvt.numpy().view(np.uint32), vt.view(np.uint32))
    assert np.array_equal(rf.numpy(), f) and np.array_equal(rft.numpy(), ft.numpy())
    text = open(out).read()
    assert text.splitlines()[1] == "mtllib mesh.mtl" and "usemtl material0" in text
    assert "\nvn " in text and "\nf %d/%d/%d " % (f[0, 0] + 1, 1, f[0, 0] + 1) in text
    assert "map_Kd albedo.png" in (tmp_path / "m" / "mesh.mtl").read_text()
    out2 = write_textured_obj(str(tmp_path / "n" / "mesh.obj"), v, f, vt, ft.numpy())      # without normals
    assert np.array_equal(read_obj(out2)[3].numpy(), ft.numpy()) and "\nvn " not in open(out2).read()


def test_config_surface_and_init_texture_loader(tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig as NerfConfig
    from src.latent_paint.configs.train_config import TrainConfig, load_config
    from src.latent_paint.models.textured_mesh import load_init_texture
    assert NerfConfig().log.mesh_texture_resolution == 0 and TrainConfig().guide.init_texture is None
    cfg = load_config(["--log.exp_name", "x", "--guide.shape_path", "m.obj", "--guide.init_texture", "t.pt"])
    assert cfg.guide.init_texture == "t.pt"
    t = torch.randn(4, 16, 16)
    torch.save(t, tmp_path / "a.pt")
    torch.save(t[None], tmp_path / "b.pt")
    assert torch.equal(load_init_texture(str(tmp_path / "a.pt"), 16), t[None])
    assert torch.equal(load_init_texture(str(tmp_path / "b.pt"), 16), t[None])
    with pytest.raises(ValueError, match="texture_resolution 16"):
        load_init_texture(str(tmp_path / "a.pt"), 32)
    torch.save(torch.randn(3, 16, 16), tmp_path / "c.pt")
    with pytest.raises(ValueError, match="expected"):
        load_init_texture(str(tmp_path / "c.pt"), 16)
