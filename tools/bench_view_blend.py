"""View-blend timing and effect: the three kernels of csrc/viewblend.hip and the whole view_bake.bake_views under each
option, and what the options do to a bake whose views disagree.  Prints ONE JSON line; records results, sets no threshold.

    python tools/bench_view_blend.py [--views 16] [--view-side 512] [--atlas 1024] [--windows 5] [--launches 200]

  timing  blub (tests/golden/shapes/blub.obj) on an --atlas^2 atlas, --views views at --view-side^2, random images, the
          low-pass at sigma = 8 (a 64 -> 512 decoder).  Kernels: HIP events around windows of --launches calls of the C
          entry point with every buffer reused (10 warm-up calls); bake_views: HIP events around each of --windows whole
          calls, which include the z-buffer, the allocations and, with exposure, the read-back of the statistics.
  effect  the painted sphere of tests/test_gpu_view_bake.py (an icosphere whose colour is its surface position, chart
          atlas, 256^2): 16 renders at 64^2 go through a stub decoder -- bilinear x 4 to 256^2, then a gain per view and
          channel in [0.8, 1.25] and a per-view sine pattern of 3 to 6 pixels' period and amplitude 0.08, the detail a
          decoder invents per view -- and are baked with each option at band_sigma = 4.  gradient: the mean magnitude of
          the forward-difference gradient of the baked image (per texel step, over covered texels with covered right and
          lower neighbours); `clean` is the bake of the views before the stub's gain and pattern, `one_view` the mean
          over the views of the gradient of that view alone.  disagreement: the mean over texels seen by two or more
          views of the standard deviation across those views of (gain x) what each shows."""
import argparse
import json
import math
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

BLUB = os.path.join(ROOT, "tests", "golden", "shapes", "blub.obj")


def _model(dev, shape, R, atlas, latent, exp_root):
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.models.textured_mesh import TexturedMeshModel
    flat = {"log.exp_name": "bench", "log.exp_root": exp_root, "guide.text": "a bench", "guide.shape_path": shape,
            "guide.texture_resolution": R, "guide.texture_interpolation_mode": "bilinear", "guide.uv_atlas": atlas}
    cfg = apply_overrides(TrainConfig(), flat).validate()
    return TexturedMeshModel(cfg, device=dev, render_grid_size=64, latent_mode=latent, texture_resolution=R), cfg


def _views(model, cfg, K):
    from src.latent_nerf.raymarching import bake_view_poses
    poses = bake_view_poses(K)
    view = model._view([t for t, _ in poses], [p for _, p in poses], [cfg.render.radius_range[1] * 1.2] * K)
    return view, model.renderer._cameras(view["elev"], view["azim"], view["radius"], view["look_at_height"])


def windows(fn, n_windows, launches, warmup=10):
    """ms per call: HIP events around each of n_windows runs of `launches` calls -> (median, [per window])."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / launches)
    return round(statistics.median(per), 4), [round(v, 4) for v in per]


def timing(dev, args, tmp):
    import ctypes

    from src import view_bake
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import gaussian_taps, uv_raster, view_zbuffer
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    K, side, R, sigma = args.views, args.view_side, args.atlas, 8.0
    model, cfg = _model(dev, BLUB, R, "triangle", True, tmp)
    verts, faces = model.mesh.vertices.float().contiguous(), model.mesh.faces
    _, cams = _views(model, cfg, K)
    torch.manual_seed(0)
    images = torch.rand(K, 3, side, side, device=dev)
    texel_face, texel_idx, pos = uv_raster(verts, faces, model.vt, model.ft, R)
    nrm = view_bake.face_normals(verts, faces.to(dev))[texel_face.reshape(-1)[texel_idx.long()].long()].contiguous()
    zbuf = view_zbuffer(verts, faces, cams, side, side)
    P = int(pos.shape[0])
    taps = gaussian_taps(sigma)
    taps_c = (ctypes.c_float * len(taps))(*taps)
    nbytes = int(B.get_lib().lnerf_view_lowpass_scratch_bytes(K, 3, side, side))
    scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    low = torch.empty_like(images)
    N = torch.zeros(K, K, device=dev, dtype=torch.int64)
    S = torch.zeros(K, K, 3, device=dev, dtype=torch.int64)
    out, weight = torch.zeros(P, 3, device=dev), torch.zeros(P, device=dev)
    count, best = torch.zeros(P, device=dev, dtype=torch.int32), torch.zeros(P, device=dev, dtype=torch.int32)
    gains = torch.ones(K, 3, device=dev)
    calls = {
        "view_lowpass": lambda: B.call("lnerf_view_lowpass", _p(images), _p(zbuf), K, 3, side, side, taps_c, len(taps) // 2,
                                       _p(scratch), nbytes, _p(low), _stream()),
        "view_overlap_stats": lambda: B.call("lnerf_view_overlap_stats", _p(pos), _p(nrm), P, _p(cams), K, side, side,
                                             _p(zbuf), _p(low), 3, 0.2, 2.0, _p(N), _p(S), _stream()),
        "uv_project_views_bands": lambda: B.call("lnerf_uv_project_views_bands", _p(pos), _p(nrm), P, _p(cams), K, side,
                                                 side, _p(zbuf), _p(images), _p(low), _p(gains), 3, 0.2, 4.0, 2.0, _p(out),
                                                 _p(weight), _p(count), _p(best), _stream()),
        "uv_project_views": lambda: B.call("lnerf_uv_project_views", _p(pos), _p(nrm), P, _p(cams), K, side, side, _p(zbuf),
                                           _p(images), 3, 0.2, 4.0, 2.0, _p(out), _p(weight), _p(count), _stream()),
    }
    res = {"mesh": "blub", "atlas": R, "views": K, "view_side": side, "sigma": sigma, "covered_texels": P,
           "accepted_pairs": None, "kernels_ms": {}, "bake_views_ms": {}}
    for name, fn in calls.items():
        med, per = windows(fn, args.windows, args.launches)
        res["kernels_ms"][name] = {"median": med, "windows": per}
    res["accepted_pairs"] = int(count.sum())
    for name, kw in (("mean", {}), ("mean+exposure", {"exposure": True}), ("bands", {"blend": "bands"}),
                     ("bands+exposure", {"blend": "bands", "exposure": True})):
        fn = lambda: view_bake.bake_views(verts, faces, model.vt, model.ft, images, cams, R, band_sigma=sigma, **kw)
        med, per = windows(fn, args.windows, 1, warmup=2)
        res["bake_views_ms"][name] = {"median": med, "windows": per}
    return res


def _gradient(rgb, mask):
    """Mean forward-difference gradient magnitude of rgb [3,R,R] over covered texels with covered right / lower neighbours."""
    cov = mask == 2
    ok = cov[:-1, :-1] & cov[:-1, 1:] & cov[1:, :-1]
    gx, gy = rgb[:, :-1, 1:] - rgb[:, :-1, :-1], rgb[:, 1:, :-1] - rgb[:, :-1, :-1]
    mag = torch.sqrt((gx * gx + gy * gy).sum(0))
    return round(float(mag[ok].mean()), 5)


def effect(dev, args, tmp):
    from src import view_bake
    from src.latent_nerf.raymarching import project_views, uv_dilate, uv_raster, view_zbuffer
    from src.latent_nerf.training.shape import make_icosphere
    v, f = make_icosphere(3, 1.0)
    obj = os.path.join(tmp, "sphere.obj")
    with open(obj, "w") as fh:
        fh.write("".join("v %r %r %r\n" % tuple(float(c) for c in p) for p in v.numpy())
                 + "".join("f %d %d %d\n" % tuple(int(i) + 1 for i in t) for t in f.numpy()))
    R, K, small, up = 256, 16, 64, 4
    side, sigma = small * up, float(up)
    model, cfg = _model(dev, obj, R, "charts", False, tmp)
    verts, faces = model.mesh.vertices.float().contiguous(), model.mesh.faces
    centre = torch.tensor([0.0, cfg.guide.dy, 0.0], device=dev)
    texel_face, texel_idx, pos = uv_raster(verts, faces, model.vt, model.ft, R)
    tex = torch.zeros(3, R * R, device=dev)
    tex[:, texel_idx.long()] = (0.5 + 0.6 * (pos - centre)).T
    mask = ((texel_face.reshape(-1) >= 0).to(torch.uint8) * 2).view(R, R)
    tex = tex.view(3, R, R).contiguous()
    uv_dilate(tex, mask, 4)
    with torch.no_grad():
        model.texture_img_rgb_finetune.copy_(tex[None])
        view, cams = _views(model, cfg, K)
        renders = model.render_test(view["elev"], view["azim"], view["radius"], dims=(small, small))["image"].clamp(0, 1)
    clean = torch.nn.functional.interpolate(renders, scale_factor=up, mode="bilinear", align_corners=False)
    rng = np.random.default_rng(1)
    gain = torch.tensor(rng.uniform(0.8, 1.25, (K, 3)), dtype=torch.float32, device=dev)
    i, j = torch.meshgrid(torch.arange(side, device=dev), torch.arange(side, device=dev), indexing="ij")
    pattern = torch.stack([0.08 * torch.sin(2 * math.pi * (i * math.cos(a) + j * math.sin(a)) / period + phase)
                           for a, period, phase in zip(rng.uniform(0, math.pi, K), rng.uniform(3, 6, K),
                                                       rng.uniform(0, 2 * math.pi, K))]).float()
    decoded = (clean * gain[:, :, None, None] + pattern[:, None]).clamp(0, 1).contiguous()
    bake = lambda images, **kw: view_bake.bake_views(verts, faces, model.vt, model.ft, images, cams, R, erode=up,
                                                     band_sigma=sigma, **kw)
    res = {"mesh": "icosphere 1280 faces, charts", "atlas": R, "views": K, "render_side": small, "decoded_side": side,
           "band_sigma": sigma, "gradient": {}, "disagreement": {}}
    base = bake(clean)
    res["seen_texels"] = int((base["view_count"] > 0).sum())
    res["mean_views_per_seen_texel"] = round(float(base["view_count"][base["view_count"] > 0].float().mean()), 2)
    res["gradient"]["clean"] = _gradient(base["rgb"], base["mask"])
    baked = {}
    for name, kw in (("mean", {}), ("mean+exposure", {"exposure": True}), ("bands", {"blend": "bands"}),
                     ("bands+exposure", {"blend": "bands", "exposure": True})):
        baked[name] = bake(decoded, **kw)
        res["gradient"][name] = _gradient(baked[name]["rgb"], baked[name]["mask"])
    # each view alone: its samples per texel, for the single-view gradient and the disagreement between views
    nrm = view_bake.face_normals(verts, faces.to(dev))[texel_face.reshape(-1)[texel_idx.long()].long()].contiguous()
    zbuf = view_zbuffer(verts, faces, cams, side, side, erode=up)
    samples, seen, grads = [], [], []
    for k in range(K):
        out, _, count = project_views(pos, nrm, cams[k:k + 1], zbuf[k:k + 1], decoded[k:k + 1])
        samples.append(out)
        seen.append(count > 0)
        img, m = torch.zeros(3, R * R, device=dev), torch.zeros(R * R, device=dev, dtype=torch.uint8)
        img[:, texel_idx.long()[count > 0]] = out[count > 0].T
        m[texel_idx.long()[count > 0]] = 2
        grads.append(_gradient(img.view(3, R, R), m.view(R, R)))
    res["gradient"]["one_view"] = round(float(np.mean(grads)), 5)
    samples, seen = torch.stack(samples, 1), torch.stack(seen, 1)                       # [P,K,3], [P,K]

    def disagreement(g):
        x = samples * g[None]
        n = seen.sum(1)
        many = n >= 2
        w = seen[many].float()[..., None]
        cnt = n[many][:, None].float()
        mean = (w * x[many]).sum(1) / cnt
        var = (w * (x[many] - mean[:, None]) ** 2).sum(1) / cnt
        return round(float(var.sqrt().mean()), 5)

    g = baked["bands+exposure"]["view_gains"]
    res["disagreement"] = {"without_exposure": disagreement(torch.ones_like(g)), "with_exposure": disagreement(g),
                           "texels_with_two_views": int((seen.sum(1) >= 2).sum())}
    res["gain_error"] = {"stub_spread": round(float((gain.max(0).values / gain.min(0).values).max()) - 1, 4),
                         "left_spread": round(float(((g * gain).max(0).values / (g * gain).min(0).values).max()) - 1, 4)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--view-side", type=int, default=512)
    ap.add_argument("--atlas", type=int, default=1024)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_view_blend needs the GPU"
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        res = {"tool": "bench_view_blend", "device": torch.cuda.get_device_name(0), "windows": args.windows,
               "launches": args.launches, "timing": timing(dev, args, tmp), "effect": effect(dev, args, tmp)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
