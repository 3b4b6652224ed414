"""Field-normal timing on the bench's field: NeRFNetwork.normal on 2^20 points (analytic: gather, MLP forward, MLP
backward with dsigmas == 1, the encoder's position-gradient kernel, the elementwise finish) against seven field() calls
on the same points -- the finite-difference route (centre + six offsets, the upstream renderer's `normal()`).  Both
precisions in ONE process.  Prints ONE JSON line.

    python tools/bench_normals.py [--points 1048576] [--reps 9]

Times are HIP events around the call (median of --reps after one warm-up call); `input_grad_ms` is the position-gradient
kernel alone on a recorded dfeat, `input_grad_GBps` its algorithmic traffic over that time: per sample 8 rows x 16 levels
x row bytes (8 f32, 4 bf16) + dfeat (16 x 8 B) + xyzs (12 B) + dxyz (12 B)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    from bench_mesh_export import field
    from src.latent_nerf.models import encoding as E
    assert torch.cuda.is_available(), "bench_normals needs the GPU"
    dev = torch.device("cuda:0")
    M = args.points
    x = (torch.rand(M, 3, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    res = []
    for precision in ("f32", "bf16"):
        net, _ = field(dev, precision)
        enc = net.encoder
        with torch.no_grad():
            t_n = timed(lambda: net.normal(x), args.reps)
            t_7 = timed(lambda: [net.field(x, M) for _ in range(7)], args.reps)
            shadow = enc.shadow()
            src = enc.embeddings.detach() if shadow is None else shadow
            dfeat = torch.randn(enc.levels.num_levels, M, 2, device=dev)
            out = torch.empty(M, 3, device=dev)
            t_k = timed(lambda: E.grid_encode_backward_input(x, net.bound, src, enc.levels, dfeat, M, None, M, out=out),
                        args.reps)
        row_bytes = 8 if src.dtype == torch.float32 else 4
        nbytes = M * (8 * enc.levels.num_levels * row_bytes + enc.levels.num_levels * 8 + 12 + 12)
        res.append({"precision": precision, "gridtype": enc.levels.gridtype, "normal_ms": round(t_n, 4),
                    "field_x7_ms": round(t_7, 4), "ratio": round(t_7 / t_n, 2), "input_grad_ms": round(t_k, 4),
                    "input_grad_bytes": nbytes, "input_grad_GBps": round(nbytes / (t_k * 1e-3) / 1e9, 1)})
        del net
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_normals", "points": M, "reps": args.reps,
                      "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
