"""The composited normal image and the 2D normal-smoothness term (optim.lambda_normal_smooth, render(normal_image=True),
lnerf_normal_image_*, lnerf_image_smooth_*) without a GPU.

1. tests/normal_image_reference.py validates itself: the op-level case of tests/test_gpu_normal_image.py meets its
   preconditions; in float64 the header's one-sweep form (chunks, carries, G_tot = N . dN) equals the plain form with the
   suffix sums written out; the plain form's backward equals float64 central differences of its forward on EVERY entry of
   every span (the six offsets of the degenerate and the NaN sample excepted: there the stated backward is a convention,
   asserted as such) within 1e-6 of the largest entry of its kind (centre rows / offset rows) -- step 1e-6: the
   round-off share is 1e-16 |L| / 1e-6 = 1e-10, the truncation share 1e-12 times the third derivative, which the
   normalisation 1 / |g| raises by a few powers of ten; measured 7e-11 of 2.5e-2 (centre) and 4.5e-8 of 2.4 (offsets).
   The stencil's gather backward equals the float64 scatter form, and central differences of its forward.
2. The float32 restatement's error against float64 is measured and printed per ray: the yardstick of the GPU tests.
3. The configuration: optim.lambda_normal_smooth defaults to 0, parses from YAML and the command line, refuses negative
   values and needs optim.start_shading_iter.
4. render(normal_image=True) refuses everything but a shaded training render of the marched renderer, before any tensor is
   touched.
5. The four ABI entry points are exported with the header's signatures (ABI 7), refuse bad arguments before any launch;
   raymarching.normal_image / image_smooth are exported and refuse CPU tensors."""
import ctypes
import re

import numpy as np
import pytest
import torch

from tests import normal_image_reference as R


@pytest.fixture(scope="module")
def case():
    k = R.op_case()
    return k, R.check_case(k)          # the preconditions, before anything is compared


def test_op_case_meets_its_preconditions(case):
    k, t = case
    assert k["M"] == sum(R.COUNTS) == 326 and k["cap"] == k["M"] + R.SENTINEL_ROWS
    assert sorted(set(range(R.N_IDS)) - set(R.IDS)) == [4]
    for ds in R.DENSITY_SCALES:
        assert len(t[ds]["w"]) == k["M"] and (t[ds]["w"] == 0).sum() >= 10 and (t[ds]["w"] > 0).sum() > 200
        # |n| <= 1 and sum w <= 1: the forward's natural magnitude is 1
        assert float(np.linalg.norm(t[ds]["n"], axis=-1).max()) <= 1 + 1e-12
        assert float(np.abs(t[ds]["image"]).max()) <= 1.0
        assert not t[ds]["image"][4].any() and not t[ds]["image"][R.IDS[R.R_EMPTY]].any()


@pytest.mark.parametrize("ds", R.DENSITY_SCALES)
def test_one_sweep_form_equals_the_plain_form_in_float64(case, ds):
    k, t = case
    r64 = R.restate(k["sig7"], k["deltas"], k["rays"], k["n_ids"], R.INV_2EPS, ds, R.T_THRESH, k["dN"], np.float64)
    e_f = float(np.abs(r64["image"] - t[ds]["image"]).max())
    gmax = np.abs(t[ds]["grad"]).max(0)
    e_b = float((np.abs(r64["grad"] - t[ds]["grad"]).max(0) / gmax).max())
    print("density_scale %.1f, float64: one-sweep form against the plain form, image %.3e, gradient rows %.3e (relative to "
          "the largest entry of the row kind)" % (ds, e_f, e_b))
    assert e_f <= 1e-14 and e_b <= 1e-12
    assert np.array_equal(r64["live"], t[ds]["live"])
    dead = ~t[ds]["live"]
    assert not t[ds]["grad"][dead].any() and not r64["grad"][dead].any()          # behind the cut: exact zeros, all 7 rows
    # the identity the one sweep rests on: sum_i g_i w_i = N . dN per ray
    at = 0
    for rid, _, cnt in k["rays"].tolist():
        go = k["dN"][rid].astype(np.float64)
        g = t[ds]["n"][at:at + cnt] @ go
        assert abs(float((g * t[ds]["w"][at:at + cnt]).sum()) - float(t[ds]["image"][rid] @ go)) <= 1e-14
        at += cnt


@pytest.mark.parametrize("ds", R.DENSITY_SCALES)
def test_float64_backward_equals_central_differences(case, ds):
    k, t = case
    rows, _ = R.span_rows(k["rays"])
    at = np.concatenate([[0], np.cumsum(k["rays"][:, 2])])
    special = {int(at[R.R_DEGENERATE] + R.I_DEGENERATE): "degenerate", int(at[R.R_NAN] + R.I_NAN): "nan"}
    entries, want = [], []
    for j, s in enumerate(rows.tolist()):
        for c in range(7):
            if c > 0 and j in special:
                continue
            entries.append(s * 7 + c)
            want.append(t[ds]["grad"][j, c])
    entries, want = np.array(entries), np.array(want)
    assert len(entries) == 7 * k["M"] - 12
    fd = R.central_difference(k["sig7"], k["deltas"], k["rays"], k["n_ids"], R.INV_2EPS, ds, k["dN"], entries)
    centre = entries % 7 == 0
    for what, sel in (("centre rows", centre), ("offset rows", ~centre)):
        err, big = float(np.abs(fd - want)[sel].max()), float(np.abs(want[sel]).max())
        print("density_scale %.1f, %s: central differences against the analytic backward %.3e, largest entry %.3e"
              % (ds, what, err, big))
        assert err <= 1e-6 * big and big > 1e-3
    # the two conventions: below the floor (and for a NaN s2) the projection is skipped, dg = -(r dn) with r = 1e10
    r = 1.0 / np.sqrt(float(R.FLOOR))
    for j in special:
        rid = int(k["rays"][np.searchsorted(at, j, side="right") - 1, 0])
        dn = t[ds]["w"][j] * k["dN"][rid].astype(np.float64)
        v = -(r * dn) * R.INV_2EPS
        stated = np.stack([v, -v], -1).reshape(-1)
        assert np.array_equal(t[ds]["grad"][j, 1:], stated) and np.abs(stated).min() > 1e6


@pytest.mark.parametrize("shape", R.SMOOTH_SHAPES)
def test_stencil_reference_validates_itself(shape):
    img, d_loss = R.smooth_case(shape)
    B, H, W, C = shape
    loss = R.smooth_forward(img, np.float64)
    x = img.astype(np.float64)
    for b in range(B):
        for y in range(H):
            for xx in range(W):
                h = ((x[b, y, xx + 1] - x[b, y, xx]) ** 2).sum() if xx + 1 < W else 0.0
                v = ((x[b, y + 1, xx] - x[b, y, xx]) ** 2).sum() if y + 1 < H else 0.0
                assert abs(loss[b, y, xx, 0] - h) <= 1e-14 * max(h, 1) and abs(loss[b, y, xx, 1] - v) <= 1e-14 * max(v, 1)
    g64 = R.smooth_backward(img, d_loss, np.float64)
    ref = R.smooth_truth_backward(img, d_loss)
    assert g64.shape == img.shape and float(np.abs(g64 - ref).max()) <= 1e-13 * max(float(np.abs(ref).max()), 1.0)
    # central differences of sum(loss * d_loss): the loss is quadratic, so they are exact up to round-off
    dl = d_loss.astype(np.float64)
    for idx in np.ndindex(*shape):
        up, dn = x.copy(), x.copy()
        up[idx] += 1e-3
        dn[idx] -= 1e-3
        fd = ((_smooth64(up) * dl).sum() - (_smooth64(dn) * dl).sum()) / 2e-3
        assert abs(fd - ref[idx]) <= 1e-9 * max(float(np.abs(ref).max()), 1.0)
    # float32 is stated operation for operation: the same values to float32 round-off
    g32 = R.smooth_backward(img, d_loss, np.float32)
    assert g32.dtype == np.float32 and float(np.abs(g32 - ref).max()) <= 64 * 2.0 ** -24 * max(float(np.abs(ref).max()), 1.0)
    if W == 1 and H == 1:
        assert not loss.any() and not ref.any()


def _smooth64(x):
    out = np.zeros(x.shape[:3] + (2,))
    out[:, :, :-1, 0] = ((x[:, :, 1:] - x[:, :, :-1]) ** 2).sum(-1)
    out[:, :-1, :, 1] = ((x[:, 1:] - x[:, :-1]) ** 2).sum(-1)
    return out


def test_float32_restatement_error_is_measured(case):
    k, t = case
    for ds in R.DENSITY_SCALES:
        e = R.f32_errors(k["sig7"], k["deltas"], k["rays"], k["n_ids"], R.INV_2EPS, ds, k["dN"])
        g = np.abs(e["t64"]["grad"])
        for rid, _, cnt in k["rays"].tolist():
            print("density_scale %.1f ray id %d (%3d samples): image f32 error %.3e; centre rows f32 error %.3e of %.3e; "
                  "offset rows %.3e of %.3e"
                  % (ds, rid, cnt, e["fwd"][rid], e["centre"][rid], R.per_ray_max(g[:, 0], k["rays"], k["n_ids"])[rid],
                     e["stencil"][rid], R.per_ray_max(g[:, 1:], k["rays"], k["n_ids"])[rid]))
        assert e["r32"]["image"].dtype == np.float32 and e["r32"]["grad"].dtype == np.float32
        assert np.isfinite(e["r32"]["image"]).all() and np.isfinite(e["r32"]["grad"]).all()
        assert np.array_equal(e["r32"]["live"], t[ds]["live"])   # float32 and float64 agree on which samples are live
        # the arithmetic is sound in float32: a few hundred ulps of the natural magnitudes
        assert float(e["fwd"].max()) < 1e-5
        cmax, smax = (R.per_ray_max(g[:, c], k["rays"], k["n_ids"]) for c in (0, slice(1, 7)))
        assert float((e["centre"][cmax > 0] / cmax[cmax > 0]).max()) < 1e-3
        assert float((e["stencil"][smax > 0] / smax[smax > 0]).max()) < 1e-3


# ------------------------------------------------------------------------------ 3. configuration
def test_config_field_parses_and_is_validated(tmp_path):
    from src.config_cli import load_config
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    assert TrainConfig().optim.lambda_normal_smooth == 0.0
    cfg = apply_overrides(TrainConfig(), {"optim.lambda_normal_smooth": 0.5, "optim.start_shading_iter": 10})
    assert cfg.optim.lambda_normal_smooth == 0.5 and cfg.optim.start_shading_iter == 10
    cfg = load_config(TrainConfig, ["--optim.lambda_normal_smooth", "0.25", "--optim.start_shading_iter=3", "--guide.text=x"])
    assert cfg.optim.lambda_normal_smooth == 0.25 and cfg.optim.start_shading_iter == 3
    # a YAML file, and a dotted flag over it
    path = tmp_path / "c.yaml"
    path.write_text("guide:\n  text: x\noptim:\n  lambda_normal_smooth: 0.125\n  start_shading_iter: 7\n")
    cfg = load_config(TrainConfig, ["--config_path", str(path)])
    assert cfg.optim.lambda_normal_smooth == 0.125 and cfg.optim.start_shading_iter == 7
    cfg = load_config(TrainConfig, ["--config_path", str(path), "--optim.lambda_normal_smooth=2"])
    assert cfg.optim.lambda_normal_smooth == 2.0
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="lambda_normal_smooth"):
            apply_overrides(TrainConfig(), {"optim.lambda_normal_smooth": bad, "optim.start_shading_iter": 1})
    with pytest.raises(ValueError, match="lambda_normal_smooth"):
        load_config(TrainConfig, ["--optim.lambda_normal_smooth=-0.5", "--optim.start_shading_iter=1"])
    with pytest.raises(ValueError, match="lambda_normal_smooth.*start_shading_iter"):
        apply_overrides(TrainConfig(), {"optim.lambda_normal_smooth": 0.5})
    apply_overrides(TrainConfig(), {"optim.lambda_normal_smooth": 0.0})          # 0 needs nothing


# ------------------------------------------------------------------------------ 4. renderer refusals
def _net(**over):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    return NeRFNetwork(RenderConfig(grid_size=16, train_h=8, train_w=8, **over), log2_hashmap_size=8)


def test_renderer_refuses_normal_image_outside_shaded_training_renders():
    """All before any tensor is touched (no GPU here: the rays are CPU tensors or None)."""
    from src.latent_nerf.models.nerf_utils import NeRFType
    z = torch.zeros(1, 4, 3)
    light = {"shading": "lambertian", "light_d": [0, 0, 1]}
    net = _net().eval()
    for kw in ({}, {"shading": "normal"}, light, {"shading": "textureless", "light_d": [0, 0, 1]}):      # evaluation mode
        with pytest.raises(ValueError, match="normal_image=True"):
            net.render(z, z, normal_image=True, **kw)
    net.train()
    for kw in ({}, {"shading": "albedo"}, {"shading": "normal"}):                                         # not shaded
        with pytest.raises(ValueError, match="normal_image=True"):
            net.render(z, z, normal_image=True, **kw)
    with pytest.raises(ValueError, match="normal_image=True"):
        net.render(None, None, normal_image=True, prepared=object())
    flat = _net(cuda_ray=False).train()                                                                   # uniform sampler
    for kw in ({}, light):
        with pytest.raises(ValueError, match="normal_image=True"):
            flat.render(z, z, normal_image=True, **kw)
    tune = _net(nerf_type=NeRFType("latent_tune")).train()
    with pytest.raises(ValueError, match="normal_image=True"):
        tune.render(z, z, normal_image=True, **light)


# ------------------------------------------------------------------------------ 5. ABI and bindings
NEW = {"lnerf_normal_image_forward": 9, "lnerf_normal_image_backward": 11, "lnerf_image_smooth_forward": 7,
       "lnerf_image_smooth_backward": 8}


def test_entry_points_are_exported_with_the_headers_signatures(built_lib):
    import os
    from src.latent_nerf.raymarching import backend as B
    assert set(NEW) <= set(B.header_symbols())
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "lnerf_hip.h")).read()
    kinds = {"float": ctypes.c_float, "int": ctypes.c_int, "int64_t": ctypes.c_int64}
    for name, n_args in NEW.items():
        assert hasattr(lib, name) and len(B._SIGNATURES[name]) == n_args
        decl = re.search(r"\bint %s\(([^;]*)\);" % name, header).group(1)
        params = [" ".join(p.split()) for p in decl.split(",")]
        assert len(params) == n_args
        for p, ctype in zip(params, B._SIGNATURES[name]):
            want = ctypes.c_void_p if ("*" in p or p.startswith("lnerf_stream_t")) else kinds[p.split()[0]]
            assert ctype is want, (name, p, ctype)


def test_abi_entry_points_refuse_bad_arguments(built_lib):
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    P = ctypes.c_void_p
    ok = P(4096)

    def fwd(sig=ok, deltas=ok, rays=ok, N=8, k=50.0, ds=1.0, T=1e-4, out=ok):
        return lib.lnerf_normal_image_forward(sig, deltas, rays, N, k, ds, T, out, None), lib.lnerf_last_error()

    def bwd(sig=ok, deltas=ok, rays=ok, N=8, k=50.0, ds=1.0, T=1e-4, d_out=ok, out=ok, grad=ok):
        return (lib.lnerf_normal_image_backward(sig, deltas, rays, N, k, ds, T, d_out, out, grad, None),
                lib.lnerf_last_error())

    for call, name, outputs in ((fwd, b"normal_image_forward", ("out",)),
                                (bwd, b"normal_image_backward", ("d_out", "out", "grad"))):
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
        for ds in (-1.0, float("nan")):
            rc, msg = call(ds=ds)
            assert rc == -1 and name in msg and b"density_scale" in msg, ds
        assert call(N=0)[0] == 0                        # nothing to do: no launch, no pointer read

    def sfwd(img=ok, B_=1, H=2, W=2, C=3, loss=ok):
        return lib.lnerf_image_smooth_forward(img, B_, H, W, C, loss, None), lib.lnerf_last_error()

    def sbwd(img=ok, B_=1, H=2, W=2, C=3, d_loss=ok, d_img=ok):
        return lib.lnerf_image_smooth_backward(img, B_, H, W, C, d_loss, d_img, None), lib.lnerf_last_error()

    for call, name, ptrs in ((sfwd, b"image_smooth_forward", ("img", "loss")),
                             (sbwd, b"image_smooth_backward", ("img", "d_loss", "d_img"))):
        for arg in ptrs:
            rc, msg = call(**{arg: None})
            assert rc == -1 and name in msg and b"null pointer" in msg, (arg, msg)
        for arg in ("B_", "H", "W"):
            rc, msg = call(**{arg: -1})
            assert rc == -1 and name in msg and b"negative size" in msg, arg
            assert call(**{arg: 0})[0] == 0             # an empty image: no launch, no pointer read
        for C in (0, 5, -1):
            rc, msg = call(C=C)
            assert rc == -1 and name in msg and b"C must be in 1..4" in msg, C
    with pytest.raises(B.LnerfError, match="normal_image_forward"):
        B.call("lnerf_normal_image_forward", None, None, None, 8, 50.0, 1.0, 1e-4, None, None)
    with pytest.raises(B.LnerfError, match="image_smooth_forward"):
        B.call("lnerf_image_smooth_forward", None, 1, 2, 2, 3, None, None)


def test_bindings_are_exported_and_refuse_cpu_tensors(case):
    from src.latent_nerf import raymarching
    from src.latent_nerf.raymarching import raymarching as rm
    k, _ = case
    assert raymarching.normal_image is rm.normal_image and raymarching.image_smooth is rm.image_smooth
    assert {"normal_image", "image_smooth"} <= set(raymarching.__all__)
    t = torch.from_numpy
    sig7 = np.nan_to_num(k["sig7"])
    with pytest.raises(ValueError, match="no CPU path"):
        rm.normal_image(t(sig7), t(k["deltas"]), t(k["rays"]), k["n_ids"], R.EPS, 1.0, R.T_THRESH)
    with pytest.raises(ValueError, match="n_ids"):
        rm.normal_image(t(sig7), t(k["deltas"]), t(k["rays"]), k["N"] - 1)
    with pytest.raises(ValueError, match="deltas"):
        rm.normal_image(t(sig7), t(k["deltas"][:k["cap"] - 1]), t(k["rays"]))
    with pytest.raises(ValueError, match="seven rows"):
        rm.normal_image(t(sig7[:-1]), t(k["deltas"]), t(k["rays"]))
    with pytest.raises(ValueError, match="no CPU path"):
        rm.image_smooth(torch.zeros(1, 2, 2, 3))
    for bad in (torch.zeros(2, 2, 3), torch.zeros(1, 2, 2, 5)):
        with pytest.raises(ValueError, match="image_smooth"):
            rm.image_smooth(bad)
