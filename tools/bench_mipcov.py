"""What the coverage-weighted pyramids cost, in the protocol of tools/bench_mipmap.py: both sides of a comparison of the
same build in ONE process, HIP events, medians of alternating windows after a warm-up.

    python tools/bench_mipcov.py [--windows 7] [--window-ms 300] [--out profiles/mipcov_bench.jsonl]

1. Renderer.render_views_texture forward + backward per call, mode mipmap against mode mipmap with mip_coverage, on
   blub.obj (its own UVs), a 1024 x 1024 4-channel texture, 64 x 64 renders, B = 1 and B = 8 views per call.  The
   coverage and its weight pyramid are cached by the renderer after the first call, as in training.  Also recorded: the
   share of the level-0 gradient's mass (sum |g|, all channels) that lands on texels outside the coverage, in both modes.
2. raymarching.pull_push_fill on a 1024 x 1024 3-channel atlas (blub's coverage without a ring, the rest empty) against
   raymarching.uv_dilate with 4 passes on the same atlas; each call includes the copy of its input.
There is no rule: the numbers are recorded.  Appends ONE JSON line to --out and prints it."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_mipmap import VIEWS, window  # noqa: E402


def alternate(fns, windows, window_ms):
    """name -> (median ms per call, spread) over `windows` alternating windows of about window_ms each."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    iters = {m: int(min(max(math.ceil(window_ms / max(window(fn, 3), 1e-3)), 3), 5000)) for m, fn in fns.items()}
    times = {m: [] for m in fns}
    for _ in range(windows):
        for m, fn in fns.items():
            times[m].append(window(fn, iters[m]))
    return {m: (statistics.median(t), max(t) - min(t)) for m, t in times.items()}, iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mipcov_bench.jsonl"))
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_mipcov needs a GPU: nothing is measured without one")
    from src.latent_nerf.raymarching import backend, pull_push_fill, uv_dilate
    from src.latent_paint.models.mesh import Mesh
    from src.latent_paint.models.render import Renderer, mip_levels, texture_coverage
    dev = torch.device("cuda:0")
    mesh = Mesh(os.path.join(ROOT, "tests", "golden", "shapes", "blub.obj"))
    mesh.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    verts, faces = mesh.vertices.to(dev), mesh.faces.to(dev)
    uv_attr = mesh.vt[mesh.ft.long()][None].to(dev).contiguous()
    R, C, side = 1024, 4, 64
    torch.manual_seed(0)
    tex = torch.randn(1, C, R, R, device=dev, requires_grad=True)
    renderers = {"mipmap": Renderer(dev, dim=(side, side), interpolation_mode="mipmap"),
                 "coverage": Renderer(dev, dim=(side, side), interpolation_mode="mipmap", mip_coverage=True)}
    covered = texture_coverage(verts, faces, uv_attr[0], R, ring=renderers["coverage"].coverage_ring)

    def call(mode, B):
        elev, azim, radius = zip(*VIEWS[:B])
        tex.grad = None
        img, _ = renderers[mode].render_views_texture(verts, faces, uv_attr, tex, elev, azim, radius, 0.25)
        img.backward(torch.ones_like(img))

    rows = []
    for B in (1, 8):
        fns = {m: (lambda m=m: call(m, B)) for m in renderers}
        share, texels = {}, {}
        for m, fn in fns.items():                     # where one call's level-0 gradient lands
            fn()
            torch.cuda.synchronize()
            g = tex.grad[0].abs()
            share[m] = float(g[:, ~covered].sum() / g.sum())
            texels[m] = int((tex.grad[0, 0] != 0).sum())
        med, iters = alternate(fns, args.windows, args.window_ms)
        rows.append({"B": B, "mipmap_ms": round(med["mipmap"][0], 4), "coverage_ms": round(med["coverage"][0], 4),
                     "mipmap_spread_ms": round(med["mipmap"][1], 4), "coverage_spread_ms": round(med["coverage"][1], 4),
                     "coverage_minus_mipmap_ms": round(med["coverage"][0] - med["mipmap"][0], 4),
                     "ratio": round(med["coverage"][0] / med["mipmap"][0], 3),
                     "gradient_mass_on_uncovered_texels": {m: round(v, 6) for m, v in share.items()},
                     "texels_with_gradient": texels, "iters": iters, "windows": args.windows})

    # ---- the fill against the gutter
    bare = texture_coverage(verts, faces, uv_attr[0], R, ring=0)
    atlas = torch.randn(3, R, R, device=dev) * bare[None]
    weight = bare.float()

    def dilate():
        uv_dilate(atlas.clone(), bare.to(torch.uint8) * 2, 4)

    def fill():
        pull_push_fill(atlas, weight)

    med, iters = alternate({"uv_dilate_4": dilate, "pull_push_fill": fill}, args.windows, args.window_ms)
    fill_row = {"texture": R, "channels": 3, "covered_texels": int(bare.sum()),
                "uv_dilate_4_ms": round(med["uv_dilate_4"][0], 4), "pull_push_fill_ms": round(med["pull_push_fill"][0], 4),
                "uv_dilate_4_spread_ms": round(med["uv_dilate_4"][1], 4),
                "pull_push_fill_spread_ms": round(med["pull_push_fill"][1], 4), "iters": iters, "windows": args.windows}
    result = {"tool": "bench_mipcov", "build": backend.get_lib().lnerf_build_info().decode(),
              "device": torch.cuda.get_device_name(0), "mesh": "blub.obj", "faces": int(faces.shape[0]), "texture": R,
              "channels": C, "side": side, "levels": mip_levels(R), "coverage_ring": renderers["coverage"].coverage_ring,
              "covered_share": round(float(covered.float().mean()), 6),
              "what": "render_views_texture forward + backward, ms per call, median of alternating HIP-event windows; "
                      "pull_push_fill against uv_dilate, ms per call, same protocol", "cases": rows, "fill": fill_row}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
