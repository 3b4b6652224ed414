"""What `guide.texture_interpolation_mode mipmap` costs: Renderer.render_views_texture forward + backward per call, mode
mipmap against mode bilinear of the same build, in ONE process on the same mesh, texture and views.

    python tools/bench_mipmap.py [--windows 7] [--window-ms 300] [--out profiles/mipmap_bench.jsonl]

Workload: blub.obj (14 208 faces), a 1024 x 1024 4-channel texture, 64 x 64 renders, B = 1 and B = 8 views per call.
A call is the whole host path: camera upload, prepare + rasterise, UV interpolation, the lookup (mipmap: footprint,
ten pyramid levels, trilinear lookup), then backward of an all-ones gradient (mipmap: the atomics into the level
gradients and the ten-level fold).  Per case one warm-up of both modes, then `--windows` (>= 5) alternating windows
bilinear / mipmap / bilinear / ...; a window is HIP events around enough back-to-back calls to last about --window-ms and
its figure is the time per call.  Reported: the median window of each mode and each mode's spread (max - min).  There is
no rule: the number is recorded.  Appends ONE JSON line to --out and prints it."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

VIEWS = [(math.radians(60.0), math.radians(30.0 + 41.0 * k), 1.25 + 0.03 * (k % 3)) for k in range(8)]


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mipmap_bench.jsonl"))
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mipmap needs a GPU: nothing is measured without one")
    from src.latent_nerf.raymarching import backend
    from src.latent_paint.models.mesh import Mesh
    from src.latent_paint.models.render import Renderer, mip_levels
    dev = torch.device("cuda:0")
    mesh = Mesh(os.path.join(ROOT, "tests", "golden", "shapes", "blub.obj"))
    mesh.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    verts, faces = mesh.vertices.to(dev), mesh.faces.to(dev)
    uv_attr = mesh.vt[mesh.ft.long()][None].to(dev)
    R, C, side = 1024, 4, 64
    torch.manual_seed(0)
    tex = torch.randn(1, C, R, R, device=dev, requires_grad=True)
    renderers = {m: Renderer(dev, dim=(side, side), interpolation_mode=m) for m in ("bilinear", "mipmap")}

    def call(mode, B):
        elev, azim, radius = zip(*VIEWS[:B])
        tex.grad = None
        img, _ = renderers[mode].render_views_texture(verts, faces, uv_attr, tex, elev, azim, radius, 0.25)
        img.backward(torch.ones_like(img))

    rows = []
    for B in (1, 8):
        fns = {m: (lambda m=m: call(m, B)) for m in renderers}
        texels = {}
        for m, fn in fns.items():                     # warm-up, and how many texels one call trains
            fn()
            torch.cuda.synchronize()
            texels[m] = int((tex.grad[0, 0] != 0).sum())
        iters = {m: int(min(max(math.ceil(args.window_ms / max(window(fn, 3), 1e-3)), 3), 5000)) for m, fn in fns.items()}
        times = {m: [] for m in fns}
        for _ in range(args.windows):
            for m, fn in fns.items():
                times[m].append(window(fn, iters[m]))
        med = {m: statistics.median(t) for m, t in times.items()}
        rows.append({"B": B, "bilinear_ms": round(med["bilinear"], 4), "mipmap_ms": round(med["mipmap"], 4),
                     "bilinear_spread_ms": round(max(times["bilinear"]) - min(times["bilinear"]), 4),
                     "mipmap_spread_ms": round(max(times["mipmap"]) - min(times["mipmap"]), 4),
                     "mipmap_minus_bilinear_ms": round(med["mipmap"] - med["bilinear"], 4),
                     "ratio": round(med["mipmap"] / med["bilinear"], 3),
                     "texels_with_gradient": texels, "iters": iters, "windows": args.windows})
    result = {"tool": "bench_mipmap", "build": backend.get_lib().lnerf_build_info().decode(),
              "device": torch.cuda.get_device_name(0), "mesh": "blub.obj", "faces": int(faces.shape[0]), "texture": R,
              "channels": C, "side": side, "levels": mip_levels(R), "what": "render_views_texture forward + backward, ms "
              "per call, median of alternating HIP-event windows", "cases": rows}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
