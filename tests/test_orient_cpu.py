"""The orientation regulariser (optim.lambda_orient, render(orient=True), lnerf_shade_fd_orient_*) without a GPU.

1. tests/orient_reference.py: its float32 terms are the op-order restatement (the normal is shading_reference._lambert's
   bit for bit), its float64 numpy gradient -- the Lambert part plus the orientation part -- equals torch float64 autograd
   of the definition with detached weights to 1e-12 relative, and the op-level case of tests/test_gpu_orient.py meets its
   preconditions for both density scales.
2. The configuration: optim.lambda_orient defaults to 0, refuses negative values and refuses > 0 without
   optim.start_shading_iter.
3. The ABI table holds both entry points at ABI 7; the host wrappers refuse CPU tensors.
4. render(orient=True) refuses shading='albedo', evaluation mode and the uniform sampler before any device work."""
import numpy as np
import pytest
import torch

from tests import orient_reference as Q
from tests import shading_reference as R


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max()) / float(np.abs(np.asarray(ref)).max())


@pytest.mark.parametrize("C,density_scale", [(4, 1.0), (3, 0.5)])
def test_numpy_gradient_equals_float64_autograd_of_the_definition(C, density_scale):
    k = Q.op_case(C, density_scale)
    Q.check_case(k)
    args = (k["sig"].reshape(-1), k["alb"].reshape(-1, C), k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"], k["dsig"],
            k["dcol"], k["deltas"], k["rays_d"], density_scale, Q.T_THRESH)
    for d_orient in (k["d_orient"], None):
        b = Q.orient_backward(*args, d_orient)
        dsg, dalb, ori = Q.total_torch(*args, d_orient, k["N"])
        total = b["lam"] + b["orient"]
        print("C=%d scale=%g d_orient %s: dsigmas7 %.3e, dalbedo %.3e (relative to the largest entry)"
              % (C, density_scale, "given" if d_orient is not None else "None", _rel(total, dsg.numpy()),
                 _rel(b["dalb"], dalb.numpy())))
        assert _rel(total, dsg.numpy()) <= 1e-12 and _rel(b["dalb"], dalb.numpy()) <= 1e-12
        if d_orient is None:
            assert not b["orient"].any()
        else:
            assert float(np.abs(b["orient"]).max()) > 1e-3 * float(np.abs(b["lam"][:, 1:]).max())     # the term is visible
    fwd = Q.orient_forward(args[0], k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"], k["deltas"], k["rays_d"],
                           density_scale, Q.T_THRESH, k["N"])
    assert _rel(fwd, ori.numpy()) <= 1e-12
    assert fwd[Q.IDS[0]] == 0.0 and fwd[Q.IDS[Q.R_BACK]] == 0.0 and int((fwd > 0).sum()) >= 4


def test_float32_terms_are_the_op_order_restatement():
    k = Q.op_case(4, 1.0)
    t = Q.sample_terms(k["sig"].reshape(-1), k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"], k["rays_d"], np.float32)
    n, s, r, d, lam = R._lambert(k["sig"][t["rows"]], t["light"], t["ambient"], k["inv"])
    for name, ref in (("n", n), ("s", s), ("r", r), ("d", d), ("lam", lam)):
        assert t[name].dtype == np.float32 and np.array_equal(t[name].view(np.int32), ref.view(np.int32)), name
    assert t["q"].dtype == np.float32 and t["v"].dtype == np.float32
    # the float32 Lambert rows are shading_reference.shade_backward's, bit for bit
    C, cap = 4, k["cap"]
    b = Q.orient_backward(k["sig"].reshape(-1), k["alb"].reshape(-1, C), k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"],
                          k["dsig"], k["dcol"], k["deltas"], k["rays_d"], 1.0, Q.T_THRESH, None, np.float32)
    d7, dr7 = np.zeros(7 * cap, np.float32), np.zeros((7 * cap, C), np.float32)
    R.shade_backward(k["sig"].reshape(-1), k["alb"].reshape(-1, C), k["rays"], k["shade"], Q.RAYS_PER_VIEW, k["inv"],
                     k["dsig"], k["dcol"], d7, dr7)
    assert np.array_equal(b["lam"], d7.reshape(cap, 7)[b["rows"]])
    assert np.array_equal(b["dalb"], dr7.reshape(cap, 7, C)[b["rows"], 0])


def test_config_field_and_validation():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    assert TrainConfig().optim.lambda_orient == 0.0
    cfg = apply_overrides(TrainConfig(), {"optim.lambda_orient": 1e-2, "optim.start_shading_iter": 100})
    assert cfg.optim.lambda_orient == 1e-2
    assert apply_overrides(TrainConfig(), {"optim.lambda_orient": 0.0}).optim.start_shading_iter is None
    with pytest.raises(ValueError, match="lambda_orient"):
        apply_overrides(TrainConfig(), {"optim.lambda_orient": -1e-3, "optim.start_shading_iter": 100})
    with pytest.raises(ValueError, match="lambda_orient"):
        apply_overrides(TrainConfig(), {"optim.lambda_orient": float("nan"), "optim.start_shading_iter": 100})
    with pytest.raises(ValueError, match="start_shading_iter"):
        apply_overrides(TrainConfig(), {"optim.lambda_orient": 1e-2})


def test_abi_table_holds_both_entry_points(built_lib):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as rm
    assert len(B._SIGNATURES["lnerf_shade_fd_orient_forward"]) == 17
    assert len(B._SIGNATURES["lnerf_shade_fd_orient_backward"]) == 19
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7
    assert hasattr(lib, "lnerf_shade_fd_orient_forward") and hasattr(lib, "lnerf_shade_fd_orient_backward")
    # argument validation needs no device: bad arguments come back as errors before any launch
    with pytest.raises(B.LnerfError, match="shade_fd_orient_forward"):
        B.call("lnerf_shade_fd_orient_forward", None, None, 4, None, 8, 4, None, 2, 50.0, None, None, 1.0, 1e-4, None, None,
               None, None)
    with pytest.raises(B.LnerfError, match="shade_fd_orient_backward"):
        B.call("lnerf_shade_fd_orient_backward", None, None, 9, None, 8, 4, None, 2, 50.0, None, None, None, None, 1.0, 1e-4,
               1, None, None, None)
    k = Q.op_case(4, 1.0)
    t = torch.from_numpy
    with pytest.raises(ValueError, match="GPU"):
        rm.shade_fd(t(k["sig"].reshape(-1)), t(k["alb"].reshape(-1, 4)), t(k["rays"]), t(k["shade"]), Q.RAYS_PER_VIEW, Q.EPS,
                    orient=(t(k["deltas"]), t(k["rays_d"]), 1.0, Q.T_THRESH, k["N"]))


def _net(**over):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    return NeRFNetwork(RenderConfig(grid_size=16, train_h=8, train_w=8, **over), log2_hashmap_size=8)


def test_renderer_refuses_orient_outside_shaded_training_renders():
    """All before any tensor is touched (no GPU here: the rays are CPU tensors or None)."""
    net = _net().train()
    z = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="orient=True"):
        net.render(z, z, shading="albedo", orient=True)
    with pytest.raises(ValueError, match="orient=True"):
        net.render(z, z, orient=True)
    with pytest.raises(ValueError, match="orient=True"):
        net.render(None, None, shading="albedo", orient=True, prepared=object())
    net.eval()
    for shading in ("lambertian", "textureless", "normal"):
        with pytest.raises(ValueError, match="orient=True"):
            net.render(z, z, shading=shading, light_d=[0, 0, 1], orient=True)
    flat = _net(cuda_ray=False).train()
    with pytest.raises(ValueError, match="orient=True"):
        flat.render(z, z, shading="lambertian", light_d=[0, 0, 1], orient=True)
    # the other refusals of a shaded render still come first to their own callers
    with pytest.raises(ValueError, match="light_d"):
        net.train().render(None, None, shading="lambertian", orient=True, prepared=object())
