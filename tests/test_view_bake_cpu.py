"""Host side of the view-projected albedo (no GPU): the view directions of bake_view_poses, the NeRF camera as the
rasteriser's record (nerf_camera_record) against the oracle's rays, and the config fields of both trees."""
import math

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O
from src.latent_nerf.raymarching.raymarching import GOLDEN_ANGLE, bake_view_poses, nerf_camera_record


def test_bake_view_poses_lattice():
    lo, hi = math.radians(15.0), math.radians(150.0)
    for K in (1, 2, 6, 16, 97):
        poses = bake_view_poses(K)
        assert len(poses) == K
        assert poses == bake_view_poses(K)                                   # deterministic
        th = np.array([p[0] for p in poses])
        assert (th > lo).all() and (th < hi).all()
        assert (np.diff(th) > 0).all() if K > 1 else True                    # one view per stratum, top to bottom
        # the polar cosine at the mid-point of the k-th of K equal strata, the azimuth k golden angles on
        c = math.cos(lo) + (np.arange(K) + 0.5) / K * (math.cos(hi) - math.cos(lo))
        assert np.allclose(np.cos(th), c, atol=1e-12)
        assert np.allclose([p[1] for p in poses], (np.arange(K) * GOLDEN_ANGLE) % (2 * math.pi), atol=1e-12)
    one = bake_view_poses(1)
    assert one[0][1] == 0.0 and abs(math.cos(one[0][0]) - 0.5 * (math.cos(lo) + math.cos(hi))) < 1e-12
    band = bake_view_poses(5, theta_range=(math.radians(60.0), math.radians(90.0)))
    assert all(math.radians(60.0) < t < math.radians(90.0) for t, _ in band)
    for bad in (0, -3):
        with pytest.raises(ValueError):
            bake_view_poses(bad)
    with pytest.raises(ValueError):
        bake_view_poses(4, theta_range=(2.0, 1.0))


def _project(rec, x, H, W):
    """Steps 2-3 of the projection rule (include/lnerf_hip.h, lnerf_uv_project_views) in float64."""
    rec = np.asarray(rec, dtype=np.float64)
    p = rec[:9].reshape(3, 3) @ (x - rec[9:12])
    assert p[2] < 0
    X, Y = rec[12] * p[0] / -p[2], rec[13] * p[1] / -p[2]
    return ((X + 1) * W - 1) / 2, ((1 - Y) * H - 1) / 2


def test_nerf_camera_record_lands_on_the_rays_pixel():
    H, W = 40, 56
    fy = H / (2 * math.tan(math.radians(55.0) / 2))
    fx = 1.1 * fy
    c2w = O.pose_from_angles(math.radians(70.0), math.radians(33.0), 1.7, target=(0.05, -0.1, 0.02))
    rec = nerf_camera_record(c2w, fx, fy, W / 2, H / 2, H, W)
    assert len(rec) == 14
    ro, rd = O.get_rays(c2w, fx, fy, W / 2, H / 2, H, W)
    ro, rd = ro[0].double().numpy(), rd[0].double().numpy()
    worst = 0.0
    for i, j, t in ((0, 0, 0.5), (0, W - 1, 1.0), (H - 1, 0, 2.5), (H - 1, W - 1, 1.3), (17, 5, 0.8), (20, 28, 3.0),
                    (3, 50, 1.9)):
        x = ro[i * W + j] + t * rd[i * W + j]
        u, v = _project(rec, x, H, W)
        worst = max(worst, abs(u - j), abs(v - i))
    assert worst < 1e-4, worst
    # the same record from a plain nested list
    assert nerf_camera_record(c2w.tolist(), fx, fy, W / 2, H / 2, H, W) == rec
    # the record has no principal point: anything off centre is refused
    for cx, cy in ((W / 2 + 0.5, H / 2), (W / 2, H / 2 - 1.0)):
        with pytest.raises(ValueError, match="principal point"):
            nerf_camera_record(c2w, fx, fy, cx, cy, H, W)


def test_intrinsics_from_fov_are_centred():
    from src.latent_nerf.models.nerf_utils import intrinsics_from_fov, pose_from_angles
    fx, fy, cx, cy = intrinsics_from_fov(55.0, 48, 64)
    rec = nerf_camera_record(pose_from_angles(1.0, 0.3, 1.8), fx, fy, cx, cy, 48, 64)
    assert rec[12] == pytest.approx(2 * fx / 64) and rec[13] == pytest.approx(2 * fy / 48)
    eye = np.array(rec[9:12])
    assert abs(np.linalg.norm(eye) - 1.8) < 1e-6
    assert np.allclose(np.array(rec[6:9]), eye / np.linalg.norm(eye), atol=1e-6)   # camera z points away from the scene


def test_nerf_config_fields():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    cfg = TrainConfig()
    assert cfg.log.mesh_bake_views == 0 and cfg.log.mesh_bake_view_size == 0
    ok = apply_overrides(TrainConfig(), {"log.mesh_bake_views": 16, "log.mesh_texture_resolution": 512,
                                         "log.mesh_bake_view_size": 64})
    assert ok.log.mesh_bake_views == 16 and ok.log.mesh_bake_view_size == 64
    with pytest.raises(ValueError, match="mesh_texture_resolution"):
        apply_overrides(TrainConfig(), {"log.mesh_bake_views": 16})
    for key in ("log.mesh_bake_views", "log.mesh_bake_view_size"):
        with pytest.raises(ValueError, match=key.split(".")[1]):
            apply_overrides(TrainConfig(), {key: -1, "log.mesh_texture_resolution": 512})


def test_paint_config_fields():
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    base = {"log.exp_name": "x", "guide.shape_path": "shape.obj"}
    assert TrainConfig().log.mesh_bake_views == 0
    assert apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": 8})).validate().log.mesh_bake_views == 8
    with pytest.raises(ValueError, match="texture_resolution"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": 8, "guide.texture_resolution": 0})).validate()
    with pytest.raises(ValueError, match="mesh_bake_views"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": -2})).validate()


def test_projection_entry_point_refuses_bad_arguments(built_lib):
    """Every argument check of lnerf_uv_project_views runs before the launch: the pointers here are made up."""
    import ctypes
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    ok = ctypes.c_void_p(4096)

    def call(P=8, K=2, H=16, W=16, C=3, cos_min=0.2, power=4.0, slack=2.0, zbuf=ok, pos=ok):
        rc = lib.lnerf_uv_project_views(pos, ok, P, ok, K, H, W, zbuf, ok, C, cos_min, power, slack, ok, ok, ok, None)
        return rc, lib.lnerf_last_error()

    for kw, word in ((dict(P=-1), b"P ="), (dict(K=0), b"K must"), (dict(H=1), b"H and W"), (dict(W=40000), b"H and W"),
                     (dict(C=0), b"C must"), (dict(C=5), b"C must"), (dict(cos_min=0.0), b"cos_min"),
                     (dict(cos_min=1.5), b"cos_min"), (dict(power=-1.0), b"power"), (dict(slack=float("inf")), b"slack"),
                     (dict(cos_min=float("nan")), b"cos_min"), (dict(zbuf=None), b"null"), (dict(pos=None), b"null")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert call(P=0, pos=None)[0] == 0                                       # no points: nothing is launched
