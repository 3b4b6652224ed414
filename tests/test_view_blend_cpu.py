"""Host side of exposure matching and two-band blending (no GPU): the library's new entry points and their argument
checks, the low-pass taps, view_bake.exposure_gains on hand-made statistics and against the least-squares restatement,
the numpy restatement's own properties, and the config fields of both trees."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import view_blend_reference as VR

NEW = ("lnerf_view_lowpass_scratch_bytes", "lnerf_view_lowpass", "lnerf_view_overlap_stats", "lnerf_uv_project_views_bands")


def test_library_exports_the_entry_points(built_lib):
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    assert set(NEW) <= set(B.header_symbols()) and set(NEW) <= set(B._SIGNATURES)
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.lnerf_abi_version() == 7                                       # additive: the version stays
    assert lib.lnerf_view_lowpass_scratch_bytes(3, 4, 40, 24) == 3 * 5 * 40 * 24 * 4
    assert lib.lnerf_view_lowpass_scratch_bytes(0, 3, 8, 8) == 0 and lib.lnerf_view_lowpass_scratch_bytes(2, 5, 8, 8) == 0


def test_entry_points_refuse_bad_arguments(built_lib):
    """Every argument check runs before the first launch: the pointers here are made up."""
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    ok = ctypes.c_void_p(4096)
    taps = (ctypes.c_float * 129)(*([1.0 / 129] * 129))

    def lowpass(K=2, C=3, H=8, W=8, r=1, images=ok, taps=taps, nbytes=1 << 20, scratch=ok):
        return lib.lnerf_view_lowpass(images, ok, K, C, H, W, taps, r, scratch, nbytes, ok, None), lib.lnerf_last_error()

    for kw, word in ((dict(K=0), b"K"), (dict(C=5), b"C"), (dict(H=0), b"H"), (dict(r=-1), b"r must"), (dict(r=65), b"r must"),
                     (dict(images=None), b"null"), (dict(taps=None), b"null"), (dict(nbytes=16), b"scratch"),
                     (dict(scratch=ctypes.c_void_p(4100)), b"aligned"), (dict(K=65535, H=4096, W=4096), b"2^31")):
        rc, msg = lowpass(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    bad = (ctypes.c_float * 3)(0.25, float("nan"), 0.25)
    assert lowpass(taps=bad)[0] == -1

    def stats(P=8, K=2, H=16, W=16, C=3, cos_min=0.2, slack=2.0, low=ok, pos=ok, N=ok):
        rc = lib.lnerf_view_overlap_stats(pos, ok, P, ok, K, H, W, ok, low, C, cos_min, slack, N, ok, None)
        return rc, lib.lnerf_last_error()

    for kw, word in ((dict(P=-1), b"P ="), (dict(K=0), b"K must"), (dict(K=65), b"K must"), (dict(H=1), b"H and W"),
                     (dict(C=0), b"C must"), (dict(cos_min=0.0), b"cos_min"), (dict(slack=-1.0), b"slack"),
                     (dict(low=None), b"null"), (dict(N=None), b"null"), (dict(pos=None), b"null")):
        rc, msg = stats(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert stats(P=0, pos=None)[0] == 0

    def bands(P=8, K=2, H=16, W=16, C=3, cos_min=0.2, power=4.0, slack=2.0, low=ok, pos=ok, best=ok):
        rc = lib.lnerf_uv_project_views_bands(pos, ok, P, ok, K, H, W, ok, ok, low, None, C, cos_min, power, slack, ok, ok,
                                              ok, best, None)
        return rc, lib.lnerf_last_error()

    for kw, word in ((dict(P=-1), b"P ="), (dict(K=0), b"K must"), (dict(K=65536), b"K must"), (dict(W=40000), b"H and W"),
                     (dict(C=5), b"C must"), (dict(cos_min=1.5), b"cos_min"), (dict(power=-1.0), b"power"),
                     (dict(slack=float("inf")), b"slack"), (dict(low=None), b"null"), (dict(best=None), b"null"),
                     (dict(pos=None), b"null")):
        rc, msg = bands(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    assert bands(P=0, pos=None, best=None)[0] == 0


def test_gaussian_taps():
    from src.latent_nerf.raymarching import gaussian_taps
    for sigma in (0.5, 1.0, 2.0, 3.0, 8.0, 10.0, 21.0):
        g = gaussian_taps(sigma)
        r = math.ceil(3 * sigma)
        assert len(g) == 2 * r + 1 and abs(math.fsum(g) - 1.0) < 1e-15
        assert g == g[::-1] and all(a < b for a, b in zip(g[:r], g[1:r + 1]))        # symmetric, one peak
        assert abs(g[r + 1] / g[r] - math.exp(-0.5 / sigma ** 2)) < 1e-15
        assert np.array_equal(np.float32(g).astype(np.float64), VR.ref_taps(sigma))   # the restatement's, to the bit
        assert abs(float(np.float32(g).astype(np.float64).sum()) - 1.0) < (2 * r + 1) * 2.0 ** -25
    assert gaussian_taps(0.0) == [1.0]
    for bad in (-1.0, float("nan"), float("inf"), 22.0):                              # r = 66 > 64
        with pytest.raises(ValueError):
            gaussian_taps(bad)


def _stats(K, C, pairs):
    """N, S for the overlaps pairs = {(i, j): (n, colour_i [C], colour_j [C])}."""
    N = torch.zeros(K, K, dtype=torch.int64)
    S = torch.zeros(K, K, C, dtype=torch.int64)
    for (i, j), (n, ci, cj) in pairs.items():
        N[i, j] = N[j, i] = n
        S[i, j] = torch.tensor([round(n * v * 2 ** 24) for v in ci])
        S[j, i] = torch.tensor([round(n * v * 2 ** 24) for v in cj])
    return N, S


def test_exposure_gains_on_hand_made_statistics():
    from src.view_bake import EXPOSURE_PRIOR, exposure_gains
    assert abs(EXPOSURE_PRIOR - ((1 / 255) / 0.1) ** 2) < 5e-5
    # two views that show the colour m through the gains a and b, and a third that overlaps nothing
    a, b, m = np.array([0.8, 1.25, 1.0]), np.array([1.25, 0.9, 1.1]), np.array([0.5, 0.3, 0.7])
    N, S = _stats(3, 3, {(0, 1): (1000, a * m, b * m)})
    g = exposure_gains(N, S, prior=1e-9).numpy()
    assert g.shape == (3, 3) and g.dtype == np.float64
    assert (g[2] == 1.0).all()                                                # isolated: exactly 1
    # as prior -> 0 the corrected views agree, g_0 a = g_1 b, and of those pairs the prior picks the one nearest (1, 1)
    assert np.abs(g[0] * a - g[1] * b).max() < 1e-7
    t = (1 / a + 1 / b) / (1 / a ** 2 + 1 / b ** 2)
    assert np.abs(g[0] - t / a).max() < 1e-6 and np.abs(g[1] - t / b).max() < 1e-6
    # gains of 1 are a fixed point whatever the prior
    N1, S1 = _stats(2, 1, {(0, 1): (50, [0.4], [0.4])})
    assert np.abs(exposure_gains(N1, S1).numpy() - 1.0).max() < 1e-12
    # a chain 0 - 1 - 2 (0 and 2 never overlap) still agrees end to end
    gains = np.array([[0.8], [1.0], [1.25]])
    N3, S3 = _stats(3, 1, {(0, 1): (300, 0.5 * gains[0], 0.5 * gains[1]), (1, 2): (200, 0.6 * gains[1], 0.6 * gains[2])})
    g3 = exposure_gains(N3, S3, prior=1e-9).numpy()
    assert np.abs(g3 * gains / (g3 * gains)[0] - 1.0).max() < 1e-6
    # the default prior leaves a little of the error: less than a tenth, more than nothing
    gd = exposure_gains(N3, S3).numpy() * gains
    assert 0.0 < gd.max() / gd.min() - 1.0 < 0.1 * (1.25 / 0.8 - 1.0)
    # no overlap at all: all 1
    assert (exposure_gains(torch.zeros(4, 4, dtype=torch.int64), torch.zeros(4, 4, 3, dtype=torch.int64)).numpy() == 1).all()
    for bad in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="prior"):
            exposure_gains(N, S, prior=bad)
    with pytest.raises(ValueError, match="N must be"):
        exposure_gains(N, S[:2])


def test_exposure_gains_match_the_least_squares_restatement():
    from src.view_bake import exposure_gains
    rng = np.random.default_rng(3)
    K, C = 7, 3
    true = rng.uniform(0.8, 1.25, (K, C))
    pairs = {}
    for i in range(K - 1):                                  # view 6 stays alone
        for j in range(i + 1, K - 1):
            if rng.uniform() < 0.6 or j == i + 1:
                colour = rng.uniform(0.2, 0.8, C)
                pairs[(i, j)] = (int(rng.integers(10, 5000)), colour * true[i], colour * true[j])
    N, S = _stats(K, C, pairs)
    M = np.where(N.numpy()[..., None] > 0, S.numpy() / (2.0 ** 24 * np.maximum(N.numpy(), 1))[..., None], 0.0)
    for prior in (1.5e-3, 1e-2, 1e-5):
        got = exposure_gains(N, S, prior=prior).numpy()
        want = VR.ref_gains(N.numpy(), M, prior)
        assert np.abs(got - want).max() < 1e-9, (prior, np.abs(got - want).max())
        assert (got[K - 1] == 1.0).all()


def test_restatement_lowpass_properties():
    rng = np.random.default_rng(0)
    K, C, H, W = 2, 2, 12, 9
    images = rng.uniform(0, 1, (K, C, H, W))
    zbuf = np.where(rng.uniform(size=(K, H, W)) < 0.7, -1.0, 1.0)
    zbuf[1] = 1.0                                           # a view with no usable pixel
    low = VR.ref_lowpass(images, zbuf, 2.0)
    assert (low[1] == 0).all() and np.isfinite(low).all()
    dirty = np.where((zbuf < 0)[:, None], images, np.nan)
    assert np.array_equal(VR.ref_lowpass(dirty, zbuf, 2.0), low)
    flat = VR.ref_lowpass(np.full((1, 1, H, W), 0.37), zbuf[:1], 1.0)        # a constant stays the constant
    assert np.abs(flat - 0.37).max() < 1e-15
    assert np.array_equal(VR.ref_lowpass(images, -np.ones((K, H, W)), 0.0), images)


def test_bake_views_checks_its_options():
    from src import view_bake
    dummy = torch.zeros(1)
    with pytest.raises(ValueError, match="blend"):
        view_bake.bake_views(dummy, dummy, dummy, dummy, dummy, dummy, 8, blend="median")
    with pytest.raises(ValueError, match="band_sigma"):
        view_bake.bake_views(dummy, dummy, dummy, dummy, dummy, dummy, 8, band_sigma=-1.0)
    assert view_bake.BAKE_BLENDS == ("mean", "bands")


def test_nerf_config_fields():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    lg = TrainConfig().log
    assert (lg.mesh_bake_blend, lg.mesh_bake_exposure, lg.mesh_bake_band_sigma) == ("mean", False, 0.0)
    base = {"log.mesh_bake_views": 16, "log.mesh_texture_resolution": 512}
    ok = apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_blend": "bands", "log.mesh_bake_exposure": True,
                                                      "log.mesh_bake_band_sigma": 4.0}))
    assert (ok.log.mesh_bake_blend, ok.log.mesh_bake_exposure, ok.log.mesh_bake_band_sigma) == ("bands", True, 4.0)
    with pytest.raises(ValueError, match="mesh_bake_blend"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_blend": "median"}))
    with pytest.raises(ValueError, match="mesh_bake_band_sigma"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_band_sigma": -1.0}))
    for key, value in (("log.mesh_bake_blend", "bands"), ("log.mesh_bake_exposure", True)):
        with pytest.raises(ValueError, match="mesh_bake_views"):
            apply_overrides(TrainConfig(), {key: value})


def test_paint_config_fields():
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides, load_config
    base = {"log.exp_name": "x", "guide.shape_path": "shape.obj"}
    lg = TrainConfig().log
    assert (lg.mesh_bake_blend, lg.mesh_bake_exposure, lg.mesh_bake_band_sigma) == ("mean", False, 0.0)
    ok = apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": 8, "log.mesh_bake_blend": "bands",
                                                      "log.mesh_bake_exposure": True, "log.mesh_bake_band_sigma": 2.0})).validate()
    assert (ok.log.mesh_bake_blend, ok.log.mesh_bake_exposure, ok.log.mesh_bake_band_sigma) == ("bands", True, 2.0)
    with pytest.raises(ValueError, match="mesh_bake_blend"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": 8, "log.mesh_bake_blend": "median"})).validate()
    with pytest.raises(ValueError, match="mesh_bake_band_sigma"):
        apply_overrides(TrainConfig(), dict(base, **{"log.mesh_bake_views": 8, "log.mesh_bake_band_sigma": -0.5})).validate()
    for key, value in (("log.mesh_bake_blend", "bands"), ("log.mesh_bake_exposure", True)):
        with pytest.raises(ValueError, match="mesh_bake_views"):
            apply_overrides(TrainConfig(), dict(base, **{key: value})).validate()
    c = load_config(["--log.exp_name", "x", "--guide.shape_path", "s.obj", "--log.mesh_bake_views", "4",
                     "--log.mesh_bake_blend", "bands", "--log.mesh_bake_exposure", "true"])
    assert c.log.mesh_bake_blend == "bands" and c.log.mesh_bake_exposure is True
