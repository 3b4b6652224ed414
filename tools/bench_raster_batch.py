"""Latent-Paint's rasteriser, parent path against the batched tile-culled path, in ONE process on the same buffers.

    python tools/bench_raster_batch.py [--windows 7] [--window-ms 60] [--sweep] [--out profiles/raster_batch_bench.json]

parent: B x (lnerf_raster_prepare + lnerf_rasterize), the brute-force kernel every pixel x every face.
new:    lnerf_raster_prepare_batch + lnerf_rasterize_batch, one call each for the B views.

Per case: one warm-up of both paths, torch.equal of their face_idx / bary (asserted at every timed size), then
`--windows` (>= 5) alternating windows parent / new / parent / ...  A window is HIP events around enough back-to-back
calls to last about --window-ms; its figure is the time per call.  Reported: the median window of each path, the parent's
own spread (max - min of its windows), and per-view times.  Cases and rules:

    (a) make_icosphere(6, 0.6): 81 920 faces, 512 x 512, B = 1     new median < parent median - parent spread
    (b) blub.obj, 64 x 64, B = 1 (every training step today)        new median <= parent median + parent spread
    (c) blub.obj, 64 x 64, B = 4 and 8                              per-view time, no rule

--sweep adds icospheres of 1 280 ... 81 920 faces at 64 / 128 / 256 / 512 pixels a side, B = 1 (where, in F * H * W, the
two paths cross).  Per-kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this tool.
Prints ONE JSON line and writes it to --out."""
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


class Case:
    def __init__(self, dev, name, verts, faces, side, B, dy):
        from src.latent_nerf.raymarching.raymarching import _p
        from src.latent_paint.models.render import Renderer
        self.name, self.B, self.H, self.W, self.F = name, B, side, side, faces.shape[0]
        self.verts = verts.float().contiguous().to(dev)
        self.faces = faces.to(torch.int32).contiguous().to(dev)
        self.cams = [Renderer.get_camera_from_view(t, p, r, dy) for t, p, r in VIEWS[:B]]
        self.cams_dev = torch.tensor([list(c) for c in self.cams], dtype=torch.float32).to(dev)
        F, P = self.F, side * side
        self.face_z = torch.empty(B, F, 3, device=dev)
        self.face_xy = torch.empty(B, F, 3, 2, device=dev)
        self.face_box = torch.empty(B, F, 4, device=dev, dtype=torch.int16)
        self.face_idx = torch.empty(B, P, device=dev, dtype=torch.int32)
        self.bary = torch.empty(B, P, 3, device=dev)
        self._p = _p

    def parent(self):
        from src.latent_nerf.raymarching import backend as _b
        p = self._p
        for b in range(self.B):
            _b.call("lnerf_raster_prepare", p(self.verts), self.verts.shape[0], p(self.faces), self.F, self.cams[b],
                    p(self.face_z[b]), p(self.face_xy[b]), None)
            _b.call("lnerf_rasterize", self.H, self.W, p(self.face_z[b]), p(self.face_xy[b]), self.F,
                    p(self.face_idx[b]), p(self.bary[b]), None)

    def new(self):
        from src.latent_nerf.raymarching import backend as _b
        p = self._p
        _b.call("lnerf_raster_prepare_batch", p(self.verts), self.verts.shape[0], p(self.faces), self.F,
                p(self.cams_dev), self.B, self.H, self.W, p(self.face_z), p(self.face_xy), p(self.face_box), None)
        _b.call("lnerf_rasterize_batch", self.B, self.H, self.W, p(self.face_z), p(self.face_xy), p(self.face_box),
                self.F, p(self.face_idx), p(self.bary), None)

    def outputs(self, fn):
        self.face_idx.fill_(-9)
        self.bary.fill_(7.0)
        fn()
        torch.cuda.synchronize()
        return self.face_idx.clone(), self.bary.clone()


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure(case, windows, window_ms):
    pidx, pbary = case.outputs(case.parent)       # warm-up of both paths, and the outputs they must share
    nidx, nbary = case.outputs(case.new)
    assert torch.equal(nidx, pidx) and torch.equal(nbary, pbary), "%s: the two paths differ" % case.name
    iters = {}
    for key, fn in (("parent", case.parent), ("new", case.new)):
        once = max(window(fn, 3), 1e-3)
        iters[key] = int(min(max(math.ceil(window_ms / once), 3), 5000))
    times = {"parent": [], "new": []}
    for _ in range(windows):
        times["parent"].append(window(case.parent, iters["parent"]))
        times["new"].append(window(case.new, iters["new"]))
    pm, nm = statistics.median(times["parent"]), statistics.median(times["new"])
    return {"case": case.name, "faces": case.F, "side": case.H, "B": case.B, "F_H_W": case.F * case.H * case.W,
            "covered": round(float((pidx >= 0).float().mean()), 4),
            "parent_ms": round(pm, 5), "new_ms": round(nm, 5),
            "parent_spread_ms": round(max(times["parent"]) - min(times["parent"]), 5),
            "new_spread_ms": round(max(times["new"]) - min(times["new"]), 5),
            "parent_ms_per_view": round(pm / case.B, 5), "new_ms_per_view": round(nm / case.B, 5),
            "speedup": round(pm / nm, 3), "iters": iters, "windows": windows, "outputs_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=60.0)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raster_batch_bench.json"))
    args = ap.parse_args()
    if args.windows < 5:
        ap.error("--windows must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("bench_raster_batch needs a GPU: nothing is measured without one")
    from src.latent_nerf.raymarching import backend
    from src.latent_nerf.training.shape import make_icosphere
    from src.latent_paint.models.mesh import Mesh
    dev = torch.device("cuda:0")
    blub = Mesh(os.path.join(ROOT, "tests", "golden", "shapes", "blub.obj"))
    blub.normalize_mesh(inplace=True, target_scale=0.6, dy=0.25)
    sphere = {lv: make_icosphere(lv, 0.6) for lv in ((3, 4, 5, 6) if args.sweep else (6,))}
    cases = [Case(dev, "a_icosphere6_512_B1", sphere[6][0], sphere[6][1], 512, 1, 0.0),
             Case(dev, "b_blub_64_B1", blub.vertices, blub.faces, 64, 1, 0.25),
             Case(dev, "c_blub_64_B4", blub.vertices, blub.faces, 64, 4, 0.25),
             Case(dev, "c_blub_64_B8", blub.vertices, blub.faces, 64, 8, 0.25)]
    rows = [measure(c, args.windows, args.window_ms) for c in cases]
    a, b = rows[0], rows[1]
    result = {"tool": "bench_raster_batch", "build": backend.get_lib().lnerf_build_info().decode(),
              "device": torch.cuda.get_device_name(0), "cases": rows,
              "rule_a_new_below_parent_minus_spread": a["new_ms"] < a["parent_ms"] - a["parent_spread_ms"],
              "rule_b_new_within_parent_plus_spread": b["new_ms"] <= b["parent_ms"] + b["parent_spread_ms"]}
    if args.sweep:
        result["sweep"] = [measure(Case(dev, "sweep_ico%d_%d" % (lv, side), sphere[lv][0], sphere[lv][1], side, 1, 0.0),
                                   args.windows, args.window_ms / 2)
                           for lv in (3, 4, 5, 6) for side in (64, 128, 256, 512) if not (lv == 6 and side == 512)]
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
