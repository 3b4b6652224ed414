"""The distortion loss (optim.lambda_distortion, render(distortion=True), lnerf_distortion_*) without a GPU.

1. tests/distortion_reference.py: in float64 the header's prefix form equals the O(k^2) double sum of the definition, its
   analytic gradient equals torch autograd of the double sum, and sum_i g_i w_i = 2 L (the identity the backward's one
   sweep rests on); the op-level case of tests/test_gpu_distortion.py meets its preconditions with no sample left out.
2. The float32 restatement's error against float64 is measured and printed per ray (forward: |loss|, backward:
   max_s |dsigma|): the yardstick of the GPU tests.
3. The configuration: optim.lambda_distortion defaults to 0, parses from the command line and refuses negative values.
4. render(distortion=True) refuses evaluation mode and the uniform sampler before any tensor is touched.
5. Both ABI entry points refuse bad arguments before any launch; distortion_loss refuses CPU tensors."""
import ctypes

import numpy as np
import pytest
import torch

from tests import distortion_reference as D


@pytest.fixture(scope="module")
def case():
    k = D.op_case()
    D.check_case(k)            # the preconditions, before anything is compared
    return k


def test_op_case_meets_its_preconditions(case):
    w, T, tau = D.check_case(case)
    assert len(w) == case["M"] == sum(D.COUNTS) and (w == 0).sum() > 100 and (w > 0).sum() > 1000


def test_prefix_form_equals_the_double_sum_and_its_gradient_the_autograd_gradient(case):
    k = case
    r64 = D.restate(k["sig"], k["deltas"], k["rays"], k["n_ids"], D.T_THRESH, k["d_loss"], np.float64)
    loss64, grad64 = D.reference_gradient(k["sig"], k["deltas"], k["rays"], k["n_ids"], k["d_loss"])
    ref = D.double_sum(k["sig"], k["deltas"], k["rays"], k["n_ids"])
    assert np.abs(ref - loss64).max() <= 1e-14 * np.abs(ref).max()          # numpy and torch state the same definition
    e_f = float(np.abs(r64["loss"] - ref).max()) / float(np.abs(ref).max())
    e_b = float(np.abs(r64["dsigmas"] - grad64).max()) / float(np.abs(grad64).max())
    print("float64: prefix form against the double sum %.3e, analytic against autograd gradient %.3e (relative to the "
          "largest entry)" % (e_f, e_b))
    assert e_f <= 1e-12 and e_b <= 1e-12
    assert float(ref.max()) > 1e-3 and float(np.abs(grad64).max()) > 1e-6
    # the empty ray and the ids of no ray
    absent = sorted(set(range(k["n_ids"])) - set(k["ids"].tolist()))
    assert len(absent) == 4 and not ref[absent].any() and ref[k["ids"][D.R_EMPTY]] == 0.0
    # rows behind the cut are exact zeros, in both
    dead = ~r64["live"]
    assert dead.sum() > 100 and not r64["dsigmas"][dead].any() and not grad64[dead].any()
    assert np.isfinite(r64["dsigmas"]).all() and np.isfinite(grad64).all()


def test_sum_of_g_w_is_twice_the_loss(case):
    """sum_i g_i w_i = 2 L per ray, with g written out from the totals as the backward does (float64)."""
    k = case
    r = D.restate(k["sig"], k["deltas"], k["rays"], k["n_ids"], D.T_THRESH, None, np.float64)
    d = k["deltas"].astype(np.float64)
    at = 0
    for rid, off, cnt in k["rays"].tolist():
        w, m, dt = r["w"][at:at + cnt], r["m"][at:at + cnt], d[off:off + cnt, 0]
        A = np.concatenate([[0.0], np.cumsum(w)[:-1]]) if cnt else w
        B = np.concatenate([[0.0], np.cumsum(w * m)[:-1]]) if cnt else w
        A_tot, B_tot = r["sums"][rid]
        g = 2 * (2 * (m * A - B) + (B_tot - m * A_tot)) + (2.0 / 3.0) * w * dt
        L = float(r["loss"][rid])
        assert abs(float((g * w).sum()) - 2 * L) <= 1e-12 * max(L, 1e-300), (rid, cnt)
        at += cnt


def test_float32_restatement_error_is_measured(case):
    k = case
    e = D.f32_errors(k["sig"], k["deltas"], k["rays"], k["n_ids"], k["d_loss"])
    gmax = D.per_ray_max(e["grad64"], k["rays"], k["n_ids"])
    for rid, _, cnt in k["rays"].tolist():
        print("ray id %2d (%3d samples): loss %.6e, f32 error %.3e; max |dsigma| %.3e, f32 error %.3e"
              % (rid, cnt, e["loss64"][rid], e["fwd"][rid], gmax[rid], e["bwd"][rid]))
    assert np.isfinite(e["r32"]["loss"]).all() and np.isfinite(e["r32"]["dsigmas"]).all()
    assert e["r32"]["loss"].dtype == np.float32 and e["r32"]["dsigmas"].dtype == np.float32
    # float32 and float64 agree on which samples are live (the margin precondition is for this)
    r64 = D.restate(k["sig"], k["deltas"], k["rays"], k["n_ids"], D.T_THRESH, None, np.float64)
    assert np.array_equal(e["r32"]["live"], r64["live"])
    # the arithmetic is sound in float32: relative to the ray's own scale the error is a few hundred ulps at most
    big = e["loss64"] > 0
    assert float((e["fwd"][big] / e["loss64"][big]).max()) < 1e-4
    assert float((e["bwd"][gmax > 0] / gmax[gmax > 0]).max()) < 1e-3


def test_config_field_parses_and_refuses_negatives():
    from src.config_cli import load_config
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    assert TrainConfig().optim.lambda_distortion == 0.0
    cfg = apply_overrides(TrainConfig(), {"optim.lambda_distortion": 1e-2})
    assert cfg.optim.lambda_distortion == 1e-2 and cfg.optim.start_shading_iter is None
    cfg = load_config(TrainConfig, ["--optim.lambda_distortion", "0.01", "--guide.text=x"])
    assert cfg.optim.lambda_distortion == 0.01
    with pytest.raises(ValueError, match="lambda_distortion"):
        load_config(TrainConfig, ["--optim.lambda_distortion=-0.5"])
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="lambda_distortion"):
            apply_overrides(TrainConfig(), {"optim.lambda_distortion": bad})


def _net(**over):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    return NeRFNetwork(RenderConfig(grid_size=16, train_h=8, train_w=8, **over), log2_hashmap_size=8)


def test_renderer_refuses_distortion_outside_marched_training_renders():
    """All before any tensor is touched (no GPU here: the rays are CPU tensors or None)."""
    net = _net().eval()
    z = torch.zeros(1, 4, 3)
    for kw in ({}, {"shading": "normal"}, {"shading": "lambertian", "light_d": [0, 0, 1]}):
        with pytest.raises(ValueError, match="distortion=True"):
            net.render(z, z, distortion=True, **kw)
    with pytest.raises(ValueError, match="distortion=True"):
        net.render(None, None, distortion=True, prepared=object())
    flat = _net(cuda_ray=False).train()
    with pytest.raises(ValueError, match="distortion=True"):
        flat.render(z, z, distortion=True)
    with pytest.raises(ValueError, match="distortion=True"):
        flat.eval().render(z, z, distortion=True)


def test_abi_entry_points_refuse_bad_arguments(built_lib):
    from src.latent_nerf.raymarching import backend as B
    assert len(B._SIGNATURES["lnerf_distortion_forward"]) == 8 and len(B._SIGNATURES["lnerf_distortion_backward"]) == 10
    assert {"lnerf_distortion_forward", "lnerf_distortion_backward"} <= set(B.header_symbols())
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7
    P = ctypes.c_void_p
    ok = P(4096)

    def fwd(sig=ok, deltas=ok, rays=ok, N=8, T=1e-4, loss=ok, sums=ok):
        return lib.lnerf_distortion_forward(sig, deltas, rays, N, T, loss, sums, None), lib.lnerf_last_error()

    def bwd(sig=ok, deltas=ok, rays=ok, N=8, T=1e-4, d_loss=ok, loss=ok, sums=ok, out=ok):
        return lib.lnerf_distortion_backward(sig, deltas, rays, N, T, d_loss, loss, sums, out, None), lib.lnerf_last_error()

    for call, name, outputs in ((fwd, b"distortion_forward", ("loss", "sums")),
                                (bwd, b"distortion_backward", ("d_loss", "loss", "sums", "out"))):
        for arg in ("sig", "deltas", "rays") + outputs:
            rc, msg = call(**{arg: None})
            assert rc == -1 and name in msg and b"null pointer" in msg, (arg, msg)
        rc, msg = call(N=-1)
        assert rc == -1 and name in msg and b"negative N" in msg
        rc, msg = call(deltas=P(4096 + 4))
        assert rc == -1 and name in msg and b"8-byte aligned" in msg
        for T in (-0.1, 1.0, 2.0, float("nan")):
            rc, msg = call(T=T)
            assert rc == -1 and name in msg and b"T_thresh" in msg, T
        assert call(N=0)[0] == 0                        # nothing to do: no launch, no pointer read
    with pytest.raises(B.LnerfError, match="distortion_forward"):
        B.call("lnerf_distortion_forward", None, None, None, 8, 1e-4, None, None, None)


def test_distortion_loss_refuses_cpu_tensors(case):
    from src.latent_nerf import raymarching
    from src.latent_nerf.raymarching import raymarching as rm
    assert raymarching.distortion_loss is rm.distortion_loss and "distortion_loss" in raymarching.__all__
    t = torch.from_numpy
    with pytest.raises(ValueError, match="no CPU path"):
        rm.distortion_loss(t(case["sig"]), t(case["deltas"]), t(case["rays"]), D.T_THRESH, case["n_ids"])
