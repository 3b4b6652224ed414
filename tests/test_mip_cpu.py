"""The mip-mapped texture lookup without a GPU: the float64 references of tests/mip_reference.py against independent
statements of what they compute, the config surface of `guide.texture_interpolation_mode mipmap`, and the C ABI of
csrc/texmip.hip (exports, ctypes table, every argument check -- made-up pointers, nothing is launched)."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

from src.latent_nerf.raymarching import backend as B
from src.latent_paint.configs.train_config import INTERPOLATION_MODES, TrainConfig, apply_overrides, load_config
from tests import mip_reference as M

NEW_SYMBOLS = ("lnerf_uv_footprint", "lnerf_mip_build", "lnerf_mip_build_backward", "lnerf_texture_mip_forward",
               "lnerf_texture_mip_backward")


def _faces(n, seed):
    """Oblique triangles with a different depth at every corner, a point strictly inside each, UVs in [0, 1]."""
    g = np.random.default_rng(seed)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    xy = f32(g.uniform(-1, 1, (n, 3, 2)))
    x, y = xy[..., 0], xy[..., 1]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    keep = np.abs(area) > 0.2
    xy = xy[keep]
    n = xy.shape[0]
    z = f32(-g.uniform(0.3, 6.0, (n, 3)))                      # up to 20 : 1 between the corners of one face
    uv = f32(g.uniform(0, 1, (n, 3, 2)))
    bary = g.dirichlet((2.0, 2.0, 2.0), n)
    p = f32((bary[..., None] * xy).sum(1))
    return xy, z, uv, p[:, 0], p[:, 1]


def test_analytic_uv_derivative_equals_central_differences():
    xy, z, uv, px, py = _faces(400, 1)
    assert xy.shape[0] > 100 and float((z.max(1) / z.min(1)).min()) < 0.2   # unequal z per corner: real perspective
    ux, vx, uy, vy = M.uv_derivatives(xy, z, uv, px, py)
    h = 1e-6
    up, vp = M.interp_uv(xy, z, uv, px + h, py)
    um, vm = M.interp_uv(xy, z, uv, px - h, py)
    uq, vq = M.interp_uv(xy, z, uv, px, py + h)
    un, vn = M.interp_uv(xy, z, uv, px, py - h)
    for got, hi, lo in ((ux, up, um), (vx, vp, vm), (uy, uq, un), (vy, vq, vn)):
        fd = (hi - lo) / (2 * h)
        # central differences: h^2 / 6 of the third derivative (the interpolant is a ratio of affine functions with its
        # pole outside the face) plus the cancellation of two float64 values over 2 h
        assert float(np.abs(got.v - fd).max()) <= 1e-7 * max(1.0, float(np.abs(fd).max())), float(np.abs(got.v - fd).max())
    # an affine map (equal z): the quotient rule's two terms cancel and the value is the affine slope
    ze = np.full_like(z, -2.0)
    ux, _, _, _ = M.uv_derivatives(xy, ze, uv, px, py)
    x, y, u = xy[..., 0], xy[..., 1], uv[..., 0]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    slope = (u[:, 0] * (y[:, 1] - y[:, 2]) + u[:, 1] * (y[:, 2] - y[:, 0]) + u[:, 2] * (y[:, 0] - y[:, 1])) / area
    assert float(np.abs(ux.v - slope).max()) < 1e-12 * float(np.abs(slope).max())


def test_footprint_reference_counts_the_kernels_roundings():
    """k of the tracked result is a property of the expression: the number the GPU test multiplies ULP * scale by."""
    H, W = 4, 6
    face_xy = torch.tensor([[[[-1.5, -1.2], [1.4, -1.0], [0.1, 1.6]]]])
    face_z = torch.tensor([[[-1.0, -2.0, -4.0]]])
    face_uv = torch.tensor([[[0.1, 0.2], [0.9, 0.3], [0.4, 0.8]]])
    idx = torch.zeros(H * W, dtype=torch.int32)
    idx[5] = -1
    rho, scale, k = M.footprint(idx, face_xy, face_z, face_uv, 1, H, W)
    assert k == M.FOOTPRINT_ROUNDINGS == 64
    assert rho[5] == 0 and scale[5] == 0 and bool((rho[idx.numpy() >= 0] > 0).all()) and bool((scale[idx.numpy() >= 0] > 0).all())
    # rho is a length per PIXEL step: the same view at twice the resolution halves it
    idx2 = torch.zeros(4 * H * W, dtype=torch.int32)
    rho2, _, _ = M.footprint(idx2, face_xy, face_z, face_uv, 1, 2 * H, 2 * W)
    cx, cy = M.pixel_centres(H, W)
    ux, vx, uy, vy = M.uv_derivatives(face_xy[0].double().numpy(), face_z[0].double().numpy(),
                                      face_uv.double().numpy(), cx[:1], cy[:1])
    want = max(math.hypot(float(ux.v[0]), float(vx.v[0])) * 2 / W, math.hypot(float(uy.v[0]), float(vy.v[0])) * 2 / H)
    assert abs(rho[0] - want) < 1e-15 and rho2.max() < rho.max()


@pytest.mark.parametrize("R,L", [(2, 1), (8, 3), (8, 1), (12, 2), (64, 6), (64, 2)])
def test_pyramid_backward_is_the_transpose_of_the_forward(R, L):
    g = torch.Generator().manual_seed(R + L)
    C = 3
    x = torch.randn(C, R, R, generator=g, dtype=torch.float64)
    y = [torch.randn(C, R >> l, R >> l, generator=g, dtype=torch.float64) for l in range(L + 1)]
    Px = M.pyramid(x, L)
    assert [tuple(p.shape) for p in Px] == [tuple(t.shape) for t in y]
    lhs = sum(float((a * b).sum()) for a, b in zip(Px, y))
    rhs = float((x * M.pyramid_transpose(y)).sum())
    assert abs(lhs - rhs) <= 1e-12 * sum(float((a * b).abs().sum()) for a, b in zip(Px, y))
    # the packed layout round-trips, and a coarse texel is the mean of the 2^l x 2^l block of the texture under it
    packed = M.pack(Px[1:])
    offs, S = M.level_offsets(R, L)
    assert packed.shape == (C, S) and all(torch.equal(a, b) for a, b in zip(M.unpack(packed, R, L), Px[1:]))
    k = 1 << L
    assert torch.allclose(Px[L], x.reshape(C, R >> L, k, R >> L, k).mean(dim=(2, 4)), atol=1e-14)
    assert M.full_levels(R) >= L


def test_trilinear_reference_at_integer_lambda_is_bilinear_on_that_level():
    g = torch.Generator().manual_seed(2)
    R, L, C = 16, 4, 3
    levels = M.pyramid(torch.randn(C, R, R, generator=g), L)
    uv = torch.rand(500, 2, generator=g) * 1.2 - 0.1
    vals, _, _ = M.bilinear_levels(levels, uv)
    for l in range(L + 1):
        rho = torch.full((500,), (2.0 ** l) / R)
        lam = M.lod(rho, R, L, 0.0)
        assert torch.equal(lam, torch.full((500,), float(l), dtype=torch.float64))
        w, l0, t = M.level_weights(lam, L)
        assert bool((l0 == l).all()) and bool((t == 0).all())
        assert torch.equal((w[:, :, None] * vals).sum(0), vals[l])
    # in between: the two neighbouring levels, weights 1 - t and t; beyond L and below 0: clamped; rho R <= 0: level 0
    lam = M.lod(torch.tensor([2.0 ** 1.25 / R, 1e3, 1e-9, 0.0, -1.0]), R, L, 0.0)
    assert torch.allclose(lam, torch.tensor([1.25, 4.0, 0.0, 0.0, 0.0], dtype=torch.float64), atol=1e-6)
    w, _, _ = M.level_weights(lam, L)
    assert torch.allclose(w[:, 0], torch.tensor([0, 0.75, 0.25, 0, 0], dtype=torch.float64), atol=1e-6)
    assert torch.equal(w[:, 1], torch.tensor([0, 0, 0, 0, 1.0], dtype=torch.float64))
    assert torch.equal(w.sum(0), torch.ones(5, dtype=torch.float64))
    assert float(M.lod(torch.tensor([1.0 / R]), R, L, 1.5)) == 1.5 and float(M.lod(torch.tensor([1.0 / R]), R, L, -1)) == 0


def test_mip_levels_per_texture_side():
    from src.latent_paint.models.render import mip_levels, mip_texels
    assert [mip_levels(R) for R in (1, 2, 3, 8, 12, 64, 1024, 96)] == [0, 1, 0, 3, 2, 6, 10, 5]
    assert [mip_levels(R) for R in (1, 2, 3, 8, 12, 64)] == [M.full_levels(R) for R in (1, 2, 3, 8, 12, 64)]
    assert mip_levels(64, 2) == 2 and mip_levels(12, 5) == 2 and mip_levels(64, 0) == 0 and mip_levels(7, 3) == 0
    assert mip_texels(12, 2) == 36 + 9 == M.level_offsets(12, 2)[1] and mip_texels(8, 0) == 0


def test_config_accepts_mipmap_from_flags_and_yaml(tmp_path):
    assert INTERPOLATION_MODES == ("nearest", "bilinear", "bicubic", "mipmap")
    base = ["--log.exp_name", "x", "--guide.shape_path", "shapes/blub.obj"]
    cfg = load_config(base + ["--guide.texture_interpolation_mode", "mipmap", "--guide.texture_max_mip_level", "3",
                              "--guide.texture_lod_bias", "-0.5"])
    g = cfg.guide
    assert (g.texture_interpolation_mode, g.texture_max_mip_level, g.texture_lod_bias) == ("mipmap", 3, -0.5)
    assert isinstance(g.texture_max_mip_level, int) and isinstance(g.texture_lod_bias, float)
    y = tmp_path / "mip.yaml"
    y.write_text("log:\n  exp_name: 'x'\nguide:\n  shape_path: shapes/blub.obj\n  texture_interpolation_mode: mipmap\n"
                 "  texture_max_mip_level: -1\n  texture_lod_bias: 0.25\n")
    g = load_config(["--config_path", str(y)]).guide
    assert (g.texture_interpolation_mode, g.texture_max_mip_level, g.texture_lod_bias) == ("mipmap", -1, 0.25)
    g = load_config(base + ["--guide.texture_interpolation_mode", "mipmap"]).guide
    assert (g.texture_max_mip_level, g.texture_lod_bias) == (-1, 0.0)


def test_config_rejects_bad_mip_fields_and_keeps_the_rest():
    def cfg(**kw):
        flat = {"log.exp_name": "x", "guide.shape_path": "s.obj"}
        flat.update({"guide." + k: v for k, v in kw.items()})
        return apply_overrides(TrainConfig(), flat).validate()

    for bias in ("nan", "inf", "-inf", float("nan")):
        with pytest.raises(ValueError, match="texture_lod_bias"):
            cfg(texture_interpolation_mode="mipmap", texture_lod_bias=bias)
    for level in (-2, "-7"):
        with pytest.raises(ValueError, match="texture_max_mip_level"):
            cfg(texture_max_mip_level=level)
    assert cfg(texture_max_mip_level=-1).guide.texture_max_mip_level == -1
    assert cfg(texture_max_mip_level=0).guide.texture_max_mip_level == 0
    with pytest.raises(ValueError, match="texture_interpolation_mode"):
        cfg(texture_interpolation_mode="trilinear")
    for mode in ("nearest", "bilinear", "bicubic"):
        assert cfg(texture_interpolation_mode=mode).guide.texture_interpolation_mode == mode
    g = TrainConfig().guide
    assert (g.texture_interpolation_mode, g.texture_max_mip_level, g.texture_lod_bias) == ("nearest", -1, 0.0)
    assert (g.texture_resolution, g.uv_atlas, g.init_texture, g.shape_scale, g.dy) == (128, "triangle", None, 0.6, 0.25)


def test_renderer_takes_the_mode_and_refuses_a_bad_bias():
    from src.latent_paint.models.render import Renderer
    r = Renderer("cpu", dim=(8, 8), interpolation_mode="mipmap", max_mip_level=2, lod_bias=0.5)
    assert (r.interpolation_mode, r.max_mip_level, r.lod_bias) == ("mipmap", 2, 0.5)
    r = Renderer("cpu", dim=(8, 8))
    assert (r.interpolation_mode, r.max_mip_level, r.lod_bias) == ("nearest", -1, 0.0)
    with pytest.raises(ValueError, match="lod_bias"):
        Renderer("cpu", dim=(8, 8), interpolation_mode="mipmap", lod_bias=float("inf"))
    with pytest.raises(AssertionError):
        Renderer("cpu", dim=(8, 8), interpolation_mode="trilinear")


def test_per_triangle_atlas_warning_names_the_ways_out(tmp_path, monkeypatch):
    import sys
    import types
    import warnings

    from src.latent_paint.models.textured_mesh import PER_TRIANGLE_MIPMAP_WARNING as W
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    assert "not neighbours" in W and "unrelated faces" in W
    for way in ("guide.uv_atlas charts", "own UVs", "texture_max_mip_level"):
        assert way in W
    # it fires when the model builds the per-triangle atlas itself in mode mipmap, and in no other mode
    monkeypatch.setitem(sys.modules, "xatlas", None)                   # not importable
    faces = torch.tensor([[0, 1, 2], [0, 2, 3]])

    def model(exp, mode):
        guide = types.SimpleNamespace(uv_atlas="triangle", texture_interpolation_mode=mode)
        mesh = types.SimpleNamespace(vertices=torch.rand(4, 3), faces=faces, vt=None, ft=None)
        return types.SimpleNamespace(mesh=mesh, device=torch.device("cpu"), texture_resolution=64,
                                     opt=types.SimpleNamespace(log=types.SimpleNamespace(exp_dir=str(exp)), guide=guide))

    with pytest.warns(UserWarning, match="per-triangle atlas"):
        vt, ft = TexturedMeshModel.init_texture_map(model(tmp_path / "a", "mipmap"))
    assert vt.shape == (6, 2) and ft.shape == (2, 3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        TexturedMeshModel.init_texture_map(model(tmp_path / "b", "bilinear"))
        TexturedMeshModel.init_texture_map(model(tmp_path / "a", "mipmap"))      # from the cache: not built here


def test_new_symbols_exported_and_bound(built_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    exported = set(re.findall(r"\b(lnerf_[a-z0-9_]+)\b", out))
    declared = B.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in exported and name in declared and name in B._SIGNATURES, name
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert B._SIGNATURES["lnerf_uv_footprint"] == [P, P, P, P, I, I, I, I, P, P]
    assert B._SIGNATURES["lnerf_mip_build"] == [P, I, I, I, P, P] == B._SIGNATURES["lnerf_mip_build_backward"]
    assert B._SIGNATURES["lnerf_texture_mip_forward"] == [P, P, P, P, P, I, I, I, I, F, P, P]
    assert B._SIGNATURES["lnerf_texture_mip_backward"] == [P, P, P, P, I, I, I, I, F, P, P, P]
    # the header's parameter kinds, parsed as tests/test_abi_cpu.py does
    text = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    kinds = {P: "ptr", I: "int", F: "float"}
    for name in NEW_SYMBOLS:
        args = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S).group(1)
        want = ["ptr" if "*" in a or "lnerf_stream_t" in a else "float" if a.strip().startswith("float") else "int"
                for a in " ".join(args.split()).split(",")]
        assert [kinds[t] for t in B._SIGNATURES[name]] == want, name
    assert B.get_lib().lnerf_abi_version() == B.ABI_VERSION == 7


def test_every_argument_check_refuses_before_a_launch(built_lib):
    """The pointers are made up: a call that got past its checks would need a GPU."""
    lib = B.get_lib()
    ok = ctypes.c_void_p(4096)
    nan, inf = float("nan"), float("inf")

    def fwd(uv=ok, rho=ok, idx=ok, tex=ok, pyr=ok, n=16, C=4, R=8, L=2, bias=0.0, out=ok):
        return lib.lnerf_texture_mip_forward(uv, rho, idx, tex, pyr, n, C, R, L, bias, out, None), lib.lnerf_last_error()

    def bwd(uv=ok, rho=ok, idx=ok, dout=ok, n=16, C=4, R=8, L=2, bias=0.0, dtex=ok, dpyr=ok):
        return (lib.lnerf_texture_mip_backward(uv, rho, idx, dout, n, C, R, L, bias, dtex, dpyr, None),
                lib.lnerf_last_error())

    def build(tex=ok, C=4, R=8, L=2, pyr=ok):
        return lib.lnerf_mip_build(tex, C, R, L, pyr, None), lib.lnerf_last_error()

    def build_bwd(dpyr=ok, C=4, R=8, L=2, dtex=ok):
        return lib.lnerf_mip_build_backward(dpyr, C, R, L, dtex, None), lib.lnerf_last_error()

    for call, who in ((fwd, b"texture_mip_forward"), (bwd, b"texture_mip_backward"), (build, b"mip_build"),
                      (build_bwd, b"mip_build_backward")):
        for kw, text in (({"C": 0}, b"C must be >= 1"), ({"R": 0}, b"R must be >= 1"), ({"L": -1}, b"L must be >= 0"),
                         ({"R": 12, "L": 3}, b"R must be divisible by 2^L"), ({"R": 8, "L": 4}, b"R must be divisible by 2^L"),
                         ({"R": 7, "L": 1}, b"R must be divisible by 2^L"), ({"R": 1 << 30, "L": 31}, b"R must be divisible by 2^L")):
            rc, msg = call(**kw)
            assert rc == -1 and text in msg and msg.startswith(who + b":"), (who, kw, msg)
    for call in (fwd, bwd):
        for bias in (nan, inf, -inf):
            rc, msg = call(bias=bias)
            assert rc == -1 and b"bias must be finite" in msg, (bias, msg)
        rc, msg = call(n=0)
        assert rc == -1 and b"n_pixels must be > 0" in msg
    for call, names in ((fwd, ("uv", "rho", "tex", "pyr", "out")), (bwd, ("uv", "rho", "dout", "dtex", "dpyr")),
                        (build, ("tex", "pyr")), (build_bwd, ("dpyr", "dtex"))):
        for name in names:
            rc, msg = call(**{name: None})
            assert rc == -1 and b"null pointer" in msg, (name, msg)

    def foot(idx=ok, xy=ok, z=ok, uv=ok, B_=1, H=8, W=8, F=2, rho=ok):
        return lib.lnerf_uv_footprint(idx, xy, z, uv, B_, H, W, F, rho, None), lib.lnerf_last_error()

    for name in ("idx", "xy", "z", "uv", "rho"):
        rc, msg = foot(**{name: None})
        assert rc == -1 and b"uv_footprint: null pointer" in msg, (name, msg)
    for kw in ({"B_": 0}, {"H": 0}, {"W": 0}, {"W": 32768}, {"B_": 65535, "H": 32767, "W": 32767}):
        rc, msg = foot(**kw)
        assert rc == -1 and b"B * H * W < 2^31" in msg, (kw, msg)
    rc, msg = foot(F=0)
    assert rc == -1 and b"no faces" in msg
