"""Host side of the field-normal entry points (lnerf_grid_encode_backward_input, lnerf_density_normals): exported,
validated before anything is launched, and reachable from the configuration.  No kernel runs here."""
import ctypes
import re
import subprocess

from src.latent_nerf.raymarching import backend as B

P = ctypes.c_void_p


def test_normal_entry_points_are_exported(built_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    exported = set(re.findall(r"\b(lnerf_[a-z0-9_]+)\b", out))
    assert {"lnerf_grid_encode_backward_input", "lnerf_density_normals"} <= exported
    assert {"lnerf_grid_encode_backward_input", "lnerf_density_normals"} <= set(B._SIGNATURES)
    assert B.get_lib().lnerf_abi_version() == 7      # additive: the ABI number does not move


def test_backward_input_validates_its_arguments(built_lib):
    lib = B.get_lib()
    offs = (ctypes.c_int32 * 3)(0, 32, 64)
    sc = (ctypes.c_float * 2)(1.0, 2.0)
    rs = (ctypes.c_int32 * 2)(2, 3)

    def call(level_dim=2, m_host=8, stride=8, dtype=B.F32, variant=0):
        return lib.lnerf_grid_encode_backward_input(P(16), 1.0, P(16), dtype, 2, level_dim, offs, sc, rs, m_host, None,
                                                    stride, P(16), P(16), variant, None)
    assert call(level_dim=4) == -1 and b"level_dim" in lib.lnerf_last_error()
    assert call(variant=B.GRID_BLOCKED | B.GRID_TILED) == -1 and b"exclude each other" in lib.lnerf_last_error()
    assert call(m_host=9, stride=8) == -1 and b"level_stride" in lib.lnerf_last_error()
    assert call(dtype=7) == -1 and b"bad dtype tag" in lib.lnerf_last_error()
    assert call(variant=1) == -1 and b"unknown variant" in lib.lnerf_last_error()
    # nothing to do: OK without touching a pointer
    assert lib.lnerf_grid_encode_backward_input(None, 1.0, None, B.F32, 2, 2, offs, sc, rs, 0, None, 0, None, None, 0,
                                                None) == 0


def test_density_normals_validates_its_arguments(built_lib):
    lib = B.get_lib()
    assert lib.lnerf_density_normals(P(16), P(16), P(16), 5.0, 0.0, 8, None, P(16), P(16), None) == -1
    assert b"blob_std" in lib.lnerf_last_error()
    assert lib.lnerf_density_normals(P(16), P(16), P(16), 5.0, 0.2, -1, None, P(16), P(16), None) == -1
    assert lib.lnerf_density_normals(None, P(16), P(16), 5.0, 0.2, 8, None, P(16), None, None) == -1
    assert b"null pointer" in lib.lnerf_last_error()
    assert lib.lnerf_density_normals(None, None, None, 5.0, 0.2, 0, None, None, None, None) == 0


def test_log_config_has_the_normal_flags():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides, load_config
    cfg = TrainConfig()
    assert cfg.log.eval_normals is False and cfg.log.mesh_field_normals is False
    cfg = apply_overrides(TrainConfig(), {"log.eval_normals": True, "log.mesh_field_normals": True})
    assert cfg.log.eval_normals is True and cfg.log.mesh_field_normals is True
    cfg = load_config(["--log.eval_normals", "true", "--log.mesh_field_normals", "true", "--guide.text", "x"])
    assert cfg.log.eval_normals is True and cfg.log.mesh_field_normals is True
    cfg = load_config(["--guide.text", "x"])
    assert cfg.log.eval_normals is False and cfg.log.mesh_field_normals is False


def test_training_renders_refuse_normal_shading():
    """No GPU needed: the refusal comes before any tensor is touched."""
    import pytest
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    net = NeRFNetwork(RenderConfig(grid_size=16, train_h=8, train_w=8), log2_hashmap_size=8).train()
    with pytest.raises(ValueError, match="evaluation render"):
        net.render(None, None, shading="normal", prepared=object())
    with pytest.raises(ValueError, match="shading must be"):
        net.eval().run_cuda(None, None, shading="lambertian")
