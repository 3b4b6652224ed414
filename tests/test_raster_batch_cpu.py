"""The ground the batched rasteriser's GPU equalities rest on, checked without a GPU.

lnerf_rasterize_batch gives the brute-force result restricted to the (pixel, face) pairs inside each face's pixel box
(include/lnerf_hip.h states the box rule; tests/raster_batch_reference.py restates it in numpy f32).  The two agree
bit for bit exactly where the brute-force test accepts no pair outside a box.  The one-pixel pad is there for that, but
it is not a proof, so the condition is checked here on the meshes and scenes the GPU tests use."""
import math

import numpy as np
import pytest
import torch

from oracle import raster_oracle as RO
from tests import raster_batch_reference as R
from tests.test_gpu_raster_ops import _grid_scene, _pixel_centres, _random_scene


def _check_no_pair_outside(H, W, fz, fxy):
    boxes = R.face_boxes(H, W, fz, fxy)
    accepted = R.accepted_pairs(H, W, fz, fxy)
    outside = accepted & ~R.pair_mask(H, W, boxes)
    assert int(outside.sum()) == 0, "%d accepted pairs outside their box" % int(outside.sum())
    idx, bary = RO.rasterize(H, W, fz, fxy)
    ridx, rbary = R.restricted_rasterize(H, W, fz, fxy, boxes)
    assert torch.equal(ridx, idx) and torch.equal(rbary, bary)
    return boxes, idx, int(accepted.sum())


def test_restatement_is_the_oracle():
    """With whole-image boxes the restated expressions are RO.rasterize itself."""
    H, W = 45, 29
    fz, fxy = _random_scene(300, seed=300)
    idx, bary = RO.rasterize(H, W, fz, fxy)
    ridx, rbary = R.restricted_rasterize(H, W, fz, fxy, R.whole_image_boxes(H, W, fz.shape[0]))
    assert torch.equal(ridx, idx) and torch.equal(rbary, bary)
    # and a restriction really restricts: with every box empty nothing is hit
    none = np.tile(np.array(R.EMPTY, dtype=np.int16), (fz.shape[0], 1))
    eidx, ebary = R.restricted_rasterize(H, W, fz, fxy, none)
    assert bool((eidx == -1).all()) and bool((ebary == 0).all())


@pytest.mark.parametrize("shape", ["blub", "teddy", "env_sphere"])
def test_no_accepted_pair_outside_its_box_on_the_meshes(shape):
    H = W = 32
    verts, faces = R.load_shape(shape)
    hit = 0
    for view in R.training_views(4, seed=11):
        fz, fxy = R.oracle_prepare(verts, faces, view)
        boxes, idx, n_pairs = _check_no_pair_outside(H, W, fz, fxy)
        hit += int((idx >= 0).sum())
        assert n_pairs > 0
        # the boxes cull: most faces miss most of the image
        area = (boxes[:, 1] - boxes[:, 0] + 1).clip(0).astype(np.int64) * (boxes[:, 3] - boxes[:, 2] + 1).clip(0)
        assert float(area.mean()) < 0.25 * H * W
    assert hit > 4 * 20


@pytest.mark.parametrize("scene", ["grid", "random300", "random129"])
def test_no_accepted_pair_outside_its_box_on_the_synthetic_scenes(scene):
    if scene == "grid":
        H, W = 37, 53
        fz, fxy = _grid_scene(H, W)
    else:
        H, W = 45, 29
        fz, fxy = _random_scene(int(scene[6:]), seed=int(scene[6:]))
    _check_no_pair_outside(H, W, fz, fxy)


def test_boxes_of_the_special_faces():
    H, W = 24, 40
    px, py = _pixel_centres(H, W)
    z = [-1.0, -1.5, -2.0]
    # a vertex exactly on a pixel centre is inside its box, with the pad to spare
    j, i = 17, 9
    on = [[float(px[j]), float(py[i])], [float(px[j + 3]), float(py[i])], [float(px[j]), float(py[i + 2])]]
    off_right = [[1.5, 0.0], [1.9, 0.1], [1.6, 0.4]]                 # wholly off-screen
    behind = on
    zero_area = [on[0], on[1], on[0]]
    nan = [[float("nan"), 0.0], [0.1, 0.2], [0.3, -0.1]]
    inf = [[0.0, float("inf")], [0.1, 0.2], [0.3, -0.1]]
    corner = [[-1.0, 1.0], [-0.97, 1.0], [-1.0, 0.95]]               # clipped at the image's corner
    fxy = torch.tensor([on, off_right, behind, on, zero_area, nan, inf, corner, nan], dtype=torch.float32)
    fz = torch.tensor([z, z, [1.0, 1.5, 2.0], [-1.0, 0.5, -2.0], z, z, z, z, [float("nan"), -1.0, -1.0]])
    box = R.face_boxes(H, W, fz, fxy)
    assert box.dtype == np.int16 and box.shape == (9, 4)
    # (rounding may put the f32 pixel coordinate a hair either side of the integer: the pad absorbs it)
    assert j - 2 <= box[0, 0] <= j - 1 and j + 4 <= box[0, 1] <= j + 5
    assert i - 2 <= box[0, 2] <= i - 1 and i + 3 <= box[0, 3] <= i + 4
    for k in (1, 2, 3, 4, 8):                                        # off-screen, behind, across z = 0, zero area, NaN depth
        assert tuple(box[k]) == R.EMPTY, k
    assert box[5].tolist() == [0, W - 1, 0, H - 1] and box[6].tolist() == [0, W - 1, 0, H - 1]
    assert box[7, 0] == 0 and box[7, 2] == 0 and 0 < box[7, 1] < 4 and 0 < box[7, 3] < 4
    # every pixel centre inside a face's bounding rectangle lies in its box, for every face of a random scene
    fz, fxy = _random_scene(300, seed=5)
    box = R.face_boxes(H, W, fz, fxy)
    live = box[:, 1] >= box[:, 0]
    x, y = fxy[..., 0], fxy[..., 1]
    inside_x = (px[None] >= x.min(1).values[:, None]) & (px[None] <= x.max(1).values[:, None])     # [F,W]
    inside_y = (py[None] >= y.min(1).values[:, None]) & (py[None] <= y.max(1).values[:, None])     # [F,H]
    jj, ii = torch.arange(W)[None], torch.arange(H)[None]
    b = torch.as_tensor(box.astype(np.int64))
    in_x = (jj >= b[:, :1]) & (jj <= b[:, 1:2])
    in_y = (ii >= b[:, 2:3]) & (ii <= b[:, 3:4])
    lv = torch.as_tensor(live)
    assert bool((in_x | ~inside_x)[lv].all()) and bool((in_y | ~inside_y)[lv].all())
    assert int(lv.sum()) > 200


def test_collate_gives_k_poses_and_batch_size_is_validated(tmp_path):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.training.views_dataset import ViewsDataset
    cfg = apply_overrides(TrainConfig(), {"render.batch_size": 3, "log.exp_name": "x", "guide.shape_path": "x.obj"})
    assert TrainConfig().render.batch_size == 1 and cfg.validate().render.batch_size == 3
    ds = ViewsDataset(cfg.render, "cpu", "train", 100, seed=2)
    data = ds.collate([0, 1, 2])
    assert set(data) == {"dir", "theta", "phi", "radius"} and data["dir"].shape == (3,)
    for key in ("theta", "phi", "radius"):
        assert isinstance(data[key], list) and len(data[key]) == 3 and all(isinstance(v, float) for v in data[key])
    assert all(0 <= t <= math.radians(150) for t in data["theta"]) and all(1.0 <= r <= 1.5 for r in data["radius"])
    assert len(set(data["theta"])) == 3
    items = list(ds.dataloader())
    assert [len(d["dir"]) for d in items] == [3] * 33 + [1]          # 100 views a pass, three at a time
    assert isinstance(items[-1]["theta"], float)
    one = ViewsDataset(TrainConfig().render, "cpu", "train", 100, seed=2).dataloader()
    assert all(isinstance(d["theta"], float) and d["dir"].shape == (1,) for d in one)
    val = list(ViewsDataset(cfg.render, "cpu", "val", 4).dataloader())    # evaluation stays one view at a time
    assert len(val) == 4 and all(isinstance(d["theta"], float) for d in val)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="batch_size"):
            apply_overrides(TrainConfig(), {"render.batch_size": bad, "log.exp_name": "x",
                                            "guide.shape_path": "x.obj"}).validate()
        with pytest.raises(ValueError, match="batch_size"):
            ViewsDataset(apply_overrides(TrainConfig(), {"render.batch_size": bad}).render, "cpu", "train", 100)
