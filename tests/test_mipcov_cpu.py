"""The coverage-weighted pyramids without a GPU: the float64 references of tests/cov_reference.py against independent
statements of what they compute, the config surface (`guide.texture_mip_coverage`, `log.mesh_texture_fill`,
`log.mesh_bake_unseen`), and the C ABI of csrc/texmip.hip (exports, ctypes table, every argument check -- made-up
pointers, nothing is launched)."""
import ctypes
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from src.latent_nerf.raymarching import backend as B
from tests import cov_reference as V
from tests import mip_reference as M

NEW_SYMBOLS = ("lnerf_mipcov_weights", "lnerf_mipcov_pull", "lnerf_mipcov_pull_backward", "lnerf_mipcov_push",
               "lnerf_texture_mipcov_forward", "lnerf_texture_mipcov_backward")
SHAPES = [(2, 1), (8, 3), (8, 1), (12, 2), (64, 6), (64, 3)]


def _coverage(R, kind, g):
    k = torch.arange(R)
    if kind == "checker":
        return ((k[:, None] + k[None, :]) % 2).float()
    if kind == "random":
        return torch.rand(R, R, generator=g)
    w = (torch.rand(R, R, generator=g) > 0.6).float()          # "holes": 0/1 with a whole empty and a whole full block
    w[:R // 2, :R // 4] = 0
    w[R // 2:, R // 2:] = 1
    return w


@pytest.mark.parametrize("R,L", SHAPES)
def test_all_ones_coverage_is_the_plain_pyramid(R, L):
    g = torch.Generator().manual_seed(R + L)
    tex = torch.randn(3, R, R, generator=g)
    wl = V.weight_levels_f32(torch.ones(R, R), L)
    assert all(bool((w == 1).all()) for w in wl)
    vals, mags = V.pull(tex, wl, L)
    for a, b in zip(vals, M.pyramid(tex, L)):
        assert torch.allclose(a, b, rtol=0, atol=1e-15)
    # ... its transpose the plain transpose, and the push returns what it was given
    d = [torch.randn(3, R >> l, R >> l, generator=g, dtype=torch.float64) for l in range(L + 1)]
    assert torch.allclose(V.pull_transpose(d, wl), M.pyramid_transpose(d), rtol=0, atol=1e-14)
    Fl, _, filled, reached = V.push(tex, wl, vals, mags, L)
    assert all(torch.equal(a, b) for a, b in zip(Fl, vals)) and not bool(filled.any()) and bool(reached.all())


@pytest.mark.parametrize("kind", ["checker", "holes", "random"])
@pytest.mark.parametrize("R,L", SHAPES)
def test_transpose_is_the_adjoint_of_pull(R, L, kind):
    g = torch.Generator().manual_seed(R * 3 + L)
    w0 = _coverage(R, kind, g)
    wl = V.weight_levels_f32(w0, L)
    if kind != "random":           # 0/1 weights: multiples of 4^-l, the f32 pyramid is the exact one
        assert all(torch.equal(a.double(), b) for a, b in zip(wl, V.weight_levels(w0, L)))
    x = torch.randn(3, R, R, generator=g, dtype=torch.float64)
    y = [torch.randn(3, R >> l, R >> l, generator=g, dtype=torch.float64) for l in range(L + 1)]
    Px, mags = V.pull(x, wl, L)
    assert all(bool((p.abs() <= m * (1 + 1e-12)).all()) for p, m in zip(Px, mags))
    lhs = sum(float((a * b).sum()) for a, b in zip(Px, y))
    rhs = float((x * V.pull_transpose(y, wl)).sum())
    assert abs(lhs - rhs) <= 1e-12 * sum(float((a * b).abs().sum()) for a, b in zip(mags, y))
    # a coarse texel is the coverage-weighted mean of the block of the texture under it (nothing covered: 0)
    k = 1 << L
    blk_w = w0.double().reshape(R >> L, k, R >> L, k)
    num = (x.reshape(3, R >> L, k, R >> L, k) * blk_w).sum(dim=(2, 4))
    den = blk_w.sum(dim=(1, 3))
    want = torch.where(den > 0, num / den.clamp(min=1e-300), torch.zeros(()).double())
    # (fractional weights: the f32 levels carry their own roundings, 2 L ULP relative, into a mean of unit normals)
    assert torch.allclose(Px[L], want, rtol=0, atol=1e-12 if kind != "random" else 100 * L * M.ULP)
    # no gradient reaches an uncovered texel through the pyramid
    y0 = [torch.zeros_like(y[0])] + y[1:]
    assert bool((V.pull_transpose(y0, wl)[:, w0 == 0] == 0).all())


@pytest.mark.parametrize("R,L", SHAPES)
def test_push_reference_fills_with_convex_combinations(R, L):
    g = torch.Generator().manual_seed(R * 5 + L)
    w0 = _coverage(R, "holes", g)
    wl = V.weight_levels_f32(w0, L)
    const = torch.tensor([0.75, -1.5, 3.0], dtype=torch.float64)
    tex = torch.where(w0[None] > 0, const.view(3, 1, 1), torch.randn(3, R, R, generator=g, dtype=torch.float64))
    vals, mags = V.pull(tex, wl, L)
    Fl, Mg, filled, reached = V.push(tex, wl, vals, mags, L)
    top = wl[L] > 0
    assert torch.equal(reached, top.repeat_interleave(1 << L, 0).repeat_interleave(1 << L, 1))
    assert torch.equal(filled, reached & (w0 != 1)) or L == 0
    assert torch.equal(Fl[0][:, ~filled], tex[:, ~filled])
    assert bool(((Fl[0] - const.view(3, 1, 1)).abs()[:, filled] < 1e-12).all())
    assert bool(((Mg[0] - const.abs().view(3, 1, 1)).abs()[:, filled] < 1e-12).all())


def test_push_reference_upsample_is_the_bilinear_one():
    """With everything reached and nothing known below the top, F_0 is F.interpolate(align_corners=False) of F_L,
    level by level."""
    R, L = 16, 2
    g = torch.Generator().manual_seed(3)
    wl = [torch.zeros(R >> l, R >> l) for l in range(L)] + [torch.ones(R >> L, R >> L)]
    top = torch.randn(1, 2, R >> L, R >> L, generator=g, dtype=torch.float64)
    vals = [torch.zeros(2, R >> l, R >> l, dtype=torch.float64) for l in range(L)] + [top[0]]
    Fl, _, filled, _ = V.push(vals[0], wl, vals, [v.abs() for v in vals], L)
    want = top
    for _ in range(L):
        want = F.interpolate(want, scale_factor=2, mode="bilinear", align_corners=False)
    assert torch.allclose(Fl[0], want[0], rtol=0, atol=1e-14) and bool(filled.all())


def test_lookup_reference_cases():
    R, L, C = 16, 4, 3
    g = torch.Generator().manual_seed(7)
    tex = torch.randn(C, R, R, generator=g)
    uv = torch.rand(400, 2, generator=g)
    lam = torch.rand(400, generator=g, dtype=torch.float64) * L
    lam[::5] = lam[::5].floor()
    cell = lam.floor().clamp(max=L).long()
    # all ones: case (a) everywhere, the plain trilinear reference
    wl = V.weight_levels_f32(torch.ones(R, R), L)
    look = V.Lookup(V.pull(tex, wl, L)[0], wl, uv)
    r = look.at(cell, lam - cell)
    vals, _, _ = M.bilinear_levels(M.pyramid(tex, L), uv)
    w, _, _ = M.level_weights(lam, L)
    assert bool(r["case_a"].all()) and torch.allclose(r["out"], (w[:, :, None] * vals).sum(0), rtol=0, atol=1e-14)
    # holes: out = sum coef V (linear in the values), the coefficients of a case (c) pixel sum to 1, a constant on the
    # covered set is looked up as that constant, and all three cases occur
    w0 = _coverage(R, "holes", g)
    wl = V.weight_levels_f32(w0, L)
    levels = V.pull(tex, wl, L)[0]
    look = V.Lookup(levels, wl, uv)
    r = look.at(cell, lam - cell)
    lin = sum((r["coef"][l][None] * levels[l].reshape(C, -1)[:, look.taps[l][0]]).sum(-1).T for l in range(L + 1))
    assert torch.allclose(lin, r["out"], rtol=0, atol=1e-13)
    case_c = ~r["case_a"] & ~r["case_b"]
    assert bool(r["case_a"].any()) and bool(r["case_b"].any()) and bool(case_c.any())
    total = sum(c.sum(-1) for c in r["coef"])
    assert torch.allclose(total[case_c], torch.ones(int(case_c.sum()), dtype=torch.float64), rtol=0, atol=1e-12)
    flat = torch.where(w0[None] > 0, torch.full((C, R, R), 2.5), torch.randn(C, R, R, generator=g))
    rc = V.Lookup(V.pull(flat, wl, L)[0], wl, uv).at(cell, lam - cell)
    assert torch.allclose(rc["out"][case_c], torch.full((int(case_c.sum()), C), 2.5, dtype=torch.float64), atol=1e-12)
    # the admissible lambdas: one piece away from an integer, three next to one; every pixel has a valid point
    pts, pieces = V.lambda_pieces(lam, torch.full_like(lam, 1e-6), L)
    valid = {n: v for n, _, _, v in pts}
    near = (lam - lam.round()).abs() <= 1e-6
    assert torch.equal(valid["a"], ~near) and torch.equal(valid["m"], near) and bool((valid["a"] | valid["m"]).all())
    assert {n for p in pieces for n in p} == set(valid)
    for n, l0, t, v in pts:
        assert bool(((t >= 0) & (t < 1) & (l0 >= 0) & (l0 <= L))[v].all()) and bool(((l0 < L) | (t == 0))[v].all()), n


# ------------------------------------------------------------------------------------------------------- configs
def test_config_surface_of_the_coverage_flag_and_the_fills():
    from src.latent_nerf.configs import train_config as nerf_cfg
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides, load_config

    def cfg(**kw):
        flat = {"log.exp_name": "x", "guide.shape_path": "s.obj"}
        flat.update(kw)
        return apply_overrides(TrainConfig(), flat).validate()

    g, lg = TrainConfig().guide, TrainConfig().log
    assert (g.texture_mip_coverage, g.texture_coverage_ring) == (False, 1)
    assert (lg.mesh_texture_fill, lg.mesh_bake_unseen) == ("dilate", "fallback")
    on = cfg(**{"guide.texture_interpolation_mode": "mipmap", "guide.texture_mip_coverage": True,
                "guide.texture_coverage_ring": 0}).guide
    assert (on.texture_mip_coverage, on.texture_coverage_ring) == (True, 0)
    for mode in ("nearest", "bilinear", "bicubic"):
        with pytest.raises(ValueError, match="texture_mip_coverage"):
            cfg(**{"guide.texture_interpolation_mode": mode, "guide.texture_mip_coverage": True})
        assert cfg(**{"guide.texture_interpolation_mode": mode}).guide.texture_mip_coverage is False
    with pytest.raises(ValueError, match="texture_coverage_ring"):
        cfg(**{"guide.texture_coverage_ring": -1})
    with pytest.raises(ValueError, match="mesh_texture_fill"):
        cfg(**{"log.mesh_texture_fill": "inpaint"})
    with pytest.raises(ValueError, match="mesh_bake_unseen"):
        cfg(**{"log.mesh_bake_unseen": "pullpush"})
    c = load_config(["--log.exp_name", "x", "--guide.shape_path", "s.obj", "--guide.texture_interpolation_mode", "mipmap",
                     "--guide.texture_mip_coverage", "true", "--log.mesh_texture_fill", "pullpush",
                     "--log.mesh_bake_unseen", "inpaint"])
    assert c.guide.texture_mip_coverage is True and (c.log.mesh_texture_fill, c.log.mesh_bake_unseen) == ("pullpush", "inpaint")
    # the NeRF tree has the two export fields
    n = nerf_cfg.TrainConfig()
    assert (n.log.mesh_texture_fill, n.log.mesh_bake_unseen) == ("dilate", "fallback")
    for name, bad in (("mesh_texture_fill", "push"), ("mesh_bake_unseen", "none")):
        n = nerf_cfg.TrainConfig()
        setattr(n.log, name, bad)
        with pytest.raises(ValueError, match=name):
            n.__post_init__()


def test_renderer_and_exports_refuse_bad_choices():
    from src import view_bake
    from src.latent_paint.models.render import Renderer
    r = Renderer("cpu", dim=(8, 8), interpolation_mode="mipmap", mip_coverage=True, coverage_ring=2)
    assert (r.mip_coverage, r.coverage_ring) == (True, 2)
    r = Renderer("cpu", dim=(8, 8), interpolation_mode="mipmap")
    assert (r.mip_coverage, r.coverage_ring) == (False, 1)
    with pytest.raises(ValueError, match="mip_coverage"):
        Renderer("cpu", dim=(8, 8), interpolation_mode="bilinear", mip_coverage=True)
    with pytest.raises(ValueError, match="coverage_ring"):
        Renderer("cpu", dim=(8, 8), interpolation_mode="mipmap", mip_coverage=True, coverage_ring=-1)
    assert view_bake.TEXTURE_FILLS == ("dilate", "pullpush") and view_bake.BAKE_UNSEEN == ("fallback", "inpaint")
    with pytest.raises(ValueError, match="fill"):
        view_bake.fill_atlas(torch.zeros(1, 2, 2), torch.zeros(2, 2, dtype=torch.uint8), "push")
    z = torch.zeros(1, 3)
    for kw, name in (({"fill": "push"}, "fill"), ({"unseen": "none"}, "unseen")):
        with pytest.raises(ValueError, match=name):
            view_bake.bake_views(z, z, z, z, torch.zeros(1, 3, 2, 2), z, 4, **kw)
    # "dilate" is the identity on both
    tex, mask = torch.rand(2, 4, 4), torch.zeros(4, 4, dtype=torch.uint8)
    a, b = view_bake.fill_atlas(tex, mask, "dilate")
    assert a is tex and b is mask


def test_coverage_refuses_a_side_above_the_raster_limit():
    from src.latent_paint.models.render import texture_coverage
    z = torch.zeros(1, 3, 2)
    with pytest.raises(ValueError, match="LNERF_UV_MAX_RES = %d" % B.UV_MAX_RES):
        texture_coverage(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), z, B.UV_MAX_RES * 2)


def test_wrappers_refuse_bad_shapes():
    from src.latent_nerf import raymarching as rm
    w = torch.zeros(8, 8)
    with pytest.raises(ValueError, match="weight must be"):
        rm.mipcov_weights(torch.zeros(8, 4))
    with pytest.raises(ValueError, match="L = 4 outside"):
        rm.mipcov_weights(w, 4)
    with pytest.raises(ValueError, match="texture must be"):
        rm.mipcov_pull(torch.zeros(3, 4, 4), w, None)
    with pytest.raises(ValueError, match="texture must be"):
        rm.pull_push_fill(torch.zeros(8, 8), w)


# ------------------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_exported_and_bound(built_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    exported = set(re.findall(r"\b(lnerf_[a-z0-9_]+)\b", out))
    declared = B.header_symbols()
    for name in NEW_SYMBOLS:
        assert name in exported and name in declared and name in B._SIGNATURES, name
    P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert B._SIGNATURES["lnerf_mipcov_weights"] == [P, I, I, P, P]
    assert B._SIGNATURES["lnerf_mipcov_pull"] == [P, P, P, I, I, I, P, P] == B._SIGNATURES["lnerf_mipcov_pull_backward"]
    assert B._SIGNATURES["lnerf_mipcov_push"] == [P, P, P, P, I, I, I, P, P]
    assert B._SIGNATURES["lnerf_texture_mipcov_forward"] == [P, P, P, P, P, P, P, I, I, I, I, Fl, P, P]
    assert B._SIGNATURES["lnerf_texture_mipcov_backward"] == [P, P, P, P, P, P, I, I, I, I, Fl, P, P, P]
    text = re.sub(r"/\*.*?\*/", "", open(B.HEADER_PATH).read(), flags=re.S)
    kinds = {P: "ptr", I: "int", Fl: "float"}
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

    def weights(w0=ok, R=8, L=2, wpyr=ok, C=None):
        return lib.lnerf_mipcov_weights(w0, R, L, wpyr, None), lib.lnerf_last_error()

    def pull(tex=ok, w0=ok, wpyr=ok, C=4, R=8, L=2, pyr=ok):
        return lib.lnerf_mipcov_pull(tex, w0, wpyr, C, R, L, pyr, None), lib.lnerf_last_error()

    def pull_bwd(dpyr=ok, w0=ok, wpyr=ok, C=4, R=8, L=2, dtex=ok):
        return lib.lnerf_mipcov_pull_backward(dpyr, w0, wpyr, C, R, L, dtex, None), lib.lnerf_last_error()

    def push(tex=ok, w0=ok, wpyr=ok, pyr=ok, C=4, R=8, L=2, filled=ok):
        return lib.lnerf_mipcov_push(tex, w0, wpyr, pyr, C, R, L, filled, None), lib.lnerf_last_error()

    def fwd(uv=ok, rho=ok, idx=ok, tex=ok, pyr=ok, w0=ok, wpyr=ok, n=16, C=4, R=8, L=2, bias=0.0, out=ok):
        return (lib.lnerf_texture_mipcov_forward(uv, rho, idx, tex, pyr, w0, wpyr, n, C, R, L, bias, out, None),
                lib.lnerf_last_error())

    def bwd(uv=ok, rho=ok, idx=ok, dout=ok, w0=ok, wpyr=ok, n=16, C=4, R=8, L=2, bias=0.0, dtex=ok, dpyr=ok):
        return (lib.lnerf_texture_mipcov_backward(uv, rho, idx, dout, w0, wpyr, n, C, R, L, bias, dtex, dpyr, None),
                lib.lnerf_last_error())

    calls = ((weights, b"mipcov_weights"), (pull, b"mipcov_pull"), (pull_bwd, b"mipcov_pull_backward"),
             (push, b"mipcov_push"), (fwd, b"texture_mipcov_forward"), (bwd, b"texture_mipcov_backward"))
    for call, who in calls:
        shapes = [({"R": 0}, b"R must be >= 1"), ({"L": -1}, b"L must be >= 0"),
                  ({"R": 12, "L": 3}, b"R must be divisible by 2^L"), ({"R": 8, "L": 4}, b"R must be divisible by 2^L"),
                  ({"R": 7, "L": 1}, b"R must be divisible by 2^L"), ({"R": 1 << 30, "L": 31}, b"R must be divisible by 2^L")]
        if call is not weights:
            shapes.append(({"C": 0}, b"C must be >= 1"))
        for kw, text in shapes:
            rc, msg = call(**kw)
            assert rc == -1 and text in msg and msg.startswith(who + b":"), (who, kw, msg)
    for call in (fwd, bwd):
        for bias in (nan, inf, -inf):
            rc, msg = call(bias=bias)
            assert rc == -1 and b"bias must be finite" in msg, (bias, msg)
        rc, msg = call(n=0)
        assert rc == -1 and b"n_pixels must be > 0" in msg
    for call, names in ((weights, ("w0", "wpyr")), (pull, ("tex", "w0", "wpyr", "pyr")),
                        (pull_bwd, ("dpyr", "w0", "wpyr", "dtex")), (push, ("tex", "w0", "wpyr", "pyr")),
                        (fwd, ("uv", "rho", "tex", "pyr", "w0", "wpyr", "out")),
                        (bwd, ("uv", "rho", "dout", "w0", "wpyr", "dtex", "dpyr"))):
        for name in names:
            rc, msg = call(**{name: None})
            assert rc == -1 and b"null pointer" in msg, (name, msg)
