"""Host side of the shaded training renders (shading = 'lambertian' / 'textureless', optim.start_shading_iter): the entry
points are exported and validate before anything is launched, the configuration reaches them, the schedule and the lights
are reproducible, the numpy restatement's backward is the derivative of its forward, and the renderer refuses what it
does not build.  No kernel runs here."""
import collections
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import shading_reference as R
from src.latent_nerf.raymarching import backend as B

P = ctypes.c_void_p
NEW = {"lnerf_fd_points", "lnerf_shade_fd_forward", "lnerf_shade_fd_backward"}
TRAINER_SEED, TRAINER_STEPS, TRAINER_START = 1, 14, 3      # tests/test_gpu_shading.py's trainer case


def test_shade_entry_points_are_exported(built_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    assert NEW <= set(re.findall(r"\b(lnerf_[a-z0-9_]+)\b", out))
    assert NEW <= set(B._SIGNATURES) and NEW <= set(B.header_symbols())
    assert B.get_lib().lnerf_abi_version() == 7 and B.ABI_VERSION == 7      # additive: the ABI number does not move


def test_fd_points_validates_its_arguments(built_lib):
    lib = B.get_lib()
    assert lib.lnerf_fd_points(None, 1.0, 0.01, 8, None, P(16), P(16), None) == -1
    assert b"null pointer" in lib.lnerf_last_error()
    assert lib.lnerf_fd_points(P(16), 1.0, 0.01, 8, None, None, P(16), None) == -1
    assert b"null pointer" in lib.lnerf_last_error()
    for eps in (0.0, -1e-2):
        assert lib.lnerf_fd_points(P(16), 1.0, eps, 8, None, P(16), P(16), None) == -1
        assert b"eps" in lib.lnerf_last_error()
    assert lib.lnerf_fd_points(P(16), 1.0, 0.01, -1, None, P(16), P(16), None) == -1
    assert lib.lnerf_fd_points(None, 1.0, 0.01, 0, None, None, None, None) == 0          # zero work


@pytest.mark.parametrize("name", ["lnerf_shade_fd_forward", "lnerf_shade_fd_backward"])
def test_shade_validates_its_arguments(built_lib, name):
    lib = B.get_lib()
    fn = getattr(lib, name)
    tail = (P(16), P(16)) if name.endswith("forward") else (P(16), P(16), P(16), P(16))

    def call(C=4, N=2, rpv=1, first=P(16), shade=P(16)):
        return fn(first, P(16), C, P(16), N, rpv, shade, 2, 50.0, *tail, None)
    for C in (0, 5, -1):
        assert call(C=C) == -1 and b"C must be 1..4" in lib.lnerf_last_error()
    for rpv in (0, -3):
        assert call(rpv=rpv) == -1 and b"rays_per_view" in lib.lnerf_last_error()
    assert call(first=None) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert call(shade=None) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert call(N=-1) == -1
    assert fn(None, None, 4, None, 0, 1, None, 0, 50.0, *([None] * len(tail)), None) == 0     # zero work


def test_config_field_parses_and_defaults_to_none(tmp_path):
    from src.latent_nerf.configs.train_config import TrainConfig, load_config
    assert TrainConfig().optim.start_shading_iter is None
    assert load_config(["--guide.text", "x"]).optim.start_shading_iter is None
    cfg = load_config(["--guide.text", "x", "--optim.start_shading_iter", "1000"])
    assert cfg.optim.start_shading_iter == 1000 and isinstance(cfg.optim.start_shading_iter, int)
    y = tmp_path / "c.yaml"
    y.write_text("guide:\n  text: x\noptim:\n  start_shading_iter: 250\n")
    assert load_config(["--config_path", str(y)]).optim.start_shading_iter == 250


def test_schedule_is_reproducible_plain_before_the_start_and_has_the_upstream_shares():
    from src.latent_nerf.training import shading as SH
    a = SH.schedule(5, 1, 400, 100)
    assert a == SH.schedule(5, 1, 400, 100)                       # a function of (seed, step): two trainers, resumed runs
    assert a != SH.schedule(6, 1, 400, 100)
    assert set(a[:99]) == {"albedo"} and set(a[99:]) == set(SH.KINDS)
    assert set(SH.schedule(5, 1, 400, None)) == {"albedo"}
    assert a[149] == SH.shading_kind(5, 150, 100)                 # any step on its own (a resumed run)
    n = 10000
    share = collections.Counter(SH.schedule(0, 1, n, 1))
    for kind, want in (("albedo", 0.2), ("textureless", 0.4), ("lambertian", 0.4)):
        assert abs(share[kind] / n - want) <= 0.02, (kind, share)


def test_the_trainer_case_of_the_gpu_suite_draws_all_three_kinds():
    """tests/test_gpu_shading.py trains 14 steps from seed 1 with start_shading_iter = 3: the draws hold every kind, and
    enough plain steps after the first two eager ones for the plain step to be captured as well."""
    from src.latent_nerf.training import shading as SH
    s = SH.schedule(TRAINER_SEED, 1, TRAINER_STEPS, TRAINER_START)
    assert s[:2] == ["albedo", "albedo"] and set(s[2:]) == set(SH.KINDS)
    assert s[2:].count("albedo") >= 2 and sum(k != "albedo" for k in s) >= 4


def test_lights_are_unit_vectors_near_the_camera():
    from src.latent_nerf.training import shading as SH
    eye = (0.3, 0.9, -0.8)
    rows = [SH.shade_row(3, step, v, eye, kind) for step in range(1, 200) for v in (0, 1)
            for kind in ("lambertian", "textureless")]
    l = np.array([r[:3] for r in rows])
    assert np.allclose(np.linalg.norm(l, axis=1), 1.0, atol=1e-12)
    assert all(r[3] == SH.AMBIENT == 0.1 for r in rows)
    assert {r[4] for r in rows} == {0.0, 1.0}
    assert SH.light_direction(3, 7, 0, eye) == SH.light_direction(3, 7, 0, eye)
    assert SH.light_direction(3, 7, 0, eye) != SH.light_direction(3, 7, 1, eye)
    # eye + N(0, I): the mean direction is the camera's, the deviates have unit variance
    far = np.array([SH.light_direction(3, s, 0, (0.0, 0.0, 0.0)) for s in range(1, 4000)])
    assert np.abs(far.mean(0)).max() < 0.05


def _case(C, seed=0):
    rng = np.random.default_rng(seed)
    rays = np.array([[0, 0, 0], [1, 0, 5], [2, 5, 9], [5, 14, 3]], dtype=np.int32)
    cap = 20
    sig = rng.uniform(0.0, 3.0, (cap, 7)).astype(np.float32)
    sig[2] = 1.5                                   # s = 0
    sig[3, 1:] = sig[3, 1:2]                       # s = 0, centre different
    sig[7, 3] = np.nan                             # a NaN density in one offset row
    alb = rng.normal(size=(cap, 7, C)).astype(np.float32)
    shade = np.array([[0.6, 0.0, 0.8, 0.1, 0.0], [0.0, -1.0, 0.0, 0.1, 1.0]], dtype=np.float32)
    dsig = rng.normal(size=cap).astype(np.float32)
    dcol = rng.normal(size=(cap, C)).astype(np.float32)
    return rays, cap, sig, alb, shade, dsig, dcol


@pytest.mark.parametrize("C", [3, 4])
def test_numpy_backward_is_the_derivative_of_the_forward(C):
    """The f32 restatement's backward against f64 autograd of the same formulas, max |err| <= 1e-4 max |ref| per output,
    on inputs with s = 0 (twice), d < 0 and a NaN density; the NaN sample is held to the stated rule instead (n = 0, so
    d = 0 is not > 0: its offset rows get zero gradient), which autograd cannot state."""
    rays, cap, sig, alb, shade, dsig, dcol = _case(C)
    inv = 1.0 / (2.0 * 1e-2)
    sc, co = np.full(cap, 7.0, np.float32), np.full((cap, C), 7.0, np.float32)
    R.shade_forward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, 3, inv, sc, co)
    d7, dr7 = np.full(7 * cap, 9.0, np.float32), np.full((7 * cap, C), 9.0, np.float32)
    R.shade_backward(sig.reshape(-1), alb.reshape(-1, C), rays, shade, 3, inv, dsig, dcol, d7, dr7)
    rows, ids = R._span_rows(rays)
    outside = np.setdiff1d(np.arange(cap), rows)
    assert (sc[outside] == 7.0).all() and (co[outside] == 7.0).all()
    assert (d7.reshape(cap, 7)[outside] == 9.0).all() and (dr7.reshape(cap, 7, C)[outside] == 9.0).all()
    rec = shade[np.minimum(ids // 3, 1)]
    sg = torch.tensor(sig[rows], dtype=torch.float64)
    nan_rows = torch.isnan(sg).any(-1)
    sg = torch.where(torch.isnan(sg), torch.zeros_like(sg), sg).requires_grad_()
    al = torch.tensor(alb[rows, 0], dtype=torch.float64, requires_grad=True)
    col, s = R.shade_torch(sg, al, torch.tensor(rec[:, :3], dtype=torch.float64), torch.tensor(rec[:, 3], dtype=torch.float64),
                           torch.tensor(rec[:, 4] != 0), inv)
    d_ref = ((-(sg[:, 1::2] - sg[:, 2::2]) * inv / torch.sqrt(torch.clamp(s, min=1e-20))[:, None])
             * torch.tensor(rec[:, :3], dtype=torch.float64)).sum(-1)
    assert bool((s == 0).sum() >= 2) and bool((d_ref < 0).any()) and bool((d_ref > 0).any()) and int(nan_rows.sum()) == 1
    keep = ~nan_rows
    (col[keep] * torch.tensor(dcol[rows], dtype=torch.float64)[keep]).sum().backward()
    keep = keep.numpy()
    assert np.abs(co[rows][keep] - col.detach().numpy()[keep]).max() <= 1e-5 * float(col.detach().abs().max())
    got_s = d7.reshape(cap, 7)[rows]
    ref_s = sg.grad.numpy()
    assert (got_s[:, 0] == dsig[rows]).all()
    scale = np.abs(ref_s[keep, 1:]).max()
    err = np.abs(got_s[keep, 1:] - ref_s[keep, 1:]).max()
    print("C=%d dsigma7: max err %.3e, max ref %.3e" % (C, err, scale))
    assert scale > 0 and err <= 1e-4 * scale
    got_a, ref_a = dr7.reshape(cap, 7, C)[rows], al.grad.numpy()
    assert (got_a[:, 1:] == 0).all()
    assert np.abs(got_a[keep, 0] - ref_a[keep]).max() <= 1e-4 * np.abs(ref_a).max()
    assert (got_s[~keep, 1:] == 0).all()                   # the NaN sample: n = 0, no gradient to the offset rows
    assert np.isfinite(got_a[~keep]).all() and np.isfinite(co[rows][~keep]).all()


def _net(**over):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    return NeRFNetwork(RenderConfig(grid_size=16, train_h=8, train_w=8, **over), log2_hashmap_size=8)


def test_renderer_refusals():
    """All before any tensor is touched (no GPU here)."""
    from src.latent_nerf.models.renderer import PreparedRays
    net = _net().train()
    for shading in ("lambertian", "textureless"):
        with pytest.raises(ValueError, match="shading must be .*light_d"):
            net.render(None, None, shading=shading, prepared=object())
        with pytest.raises(ValueError, match="shading must be .*light_d"):
            net.eval().run_cuda(None, None, shading=shading)
        net.train()
    with pytest.raises(ValueError, match="shading must be"):
        net.run_cuda(None, None, shading="phong", light_d=[0, 0, 1])
    with pytest.raises(ValueError, match="uniform sampler"):
        net.run(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), shading="lambertian", light_d=[0, 0, 1])
    flat = _net(cuda_ray=False).train()
    with pytest.raises(ValueError, match="uniform sampler"):
        flat.render(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), shading="textureless", light_d=[0, 0, 1])
    from src.latent_nerf.models.nerf_utils import NeRFType
    tuned = _net(nerf_type=NeRFType("latent_tune")).train()
    with pytest.raises(ValueError, match="latent_tune"):
        tuned.render(None, None, shading="lambertian", light_d=[0, 0, 1], prepared=object())
    # bf16: 7 x capacity is the level stride of the one field node
    big = _net(mlp_precision="bf16", table_dtype="bf16").train()
    limit = (1 << 24) // 7
    with pytest.raises(ValueError, match="render.max_samples"):
        big.run_cuda(None, None, shading="lambertian", light_d=[0, 0, 1],
                     prepared=PreparedRays(None, None, (1, 64), 64, limit + 1))
    capped = _net(mlp_precision="bf16", table_dtype="bf16", max_samples=limit + 1).train()
    with pytest.raises(ValueError, match="render.max_samples"):
        capped.render(torch.zeros(1, 64, 3), torch.zeros(1, 64, 3), shading="textureless", light_d=[0, 0, 1])
    assert big._check_fd_stride(limit) is None and _net()._check_fd_stride(limit + 1) is None     # f32: no such limit


def test_the_scene_of_the_gpu_suite_has_well_conditioned_normals():
    """tests/test_gpu_shading.py leaves samples whose reference |g|^2 < 1e-12 out of nothing as long as there are at most
    0.1 % of them: with the scene's seed there are none, and every kind of ray (empty, short, long) occurs."""
    from oracle import nerf_oracle as O
    net, bits = R.scene_net(O, "f32")
    ro, rd, bg, g = R.scene_rays(O)
    lv, table, params = R.scene_oracle_leaves(O, net)
    S = R.SCENE
    ref = R.render_shaded_oracle(O, ro, rd, table.double(), {k: v.double() for k, v in params.items()}, lv, bits,
                                 light=S["LIGHT"], ambient=S["AMBIENT"], textureless=False, eps=S["EPS"], G=S["G"],
                                 max_steps=S["MAX_STEPS"], bg_color=bg)
    flat = int((ref["s"] < 1e-12).sum())
    print("scene: %d samples, %d with |g|^2 < 1e-12, smallest %.3e" % (ref["M"], flat, float(ref["s"].min())))
    assert ref["M"] > 100 and flat <= ref["M"] // 1000
    counts = ref["rays"][:, 2]
    assert int((counts == 0).sum()) > 0 and int(counts.max()) > 4
