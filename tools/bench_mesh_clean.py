"""Mesh cleaning timing: raymarching.clean_mesh (components + filter, at the upstream exporter's 8 faces / 0.05 of the
diagonal), raymarching.smooth_mesh (10 iterations) and, beside them, raymarching.decimate_mesh, on
  bumpy   the 64^3 "bumpy" sphere of tests/test_gpu_decimate.py (decimated to 2000 faces, as there), and
  export  the marching-cubes mesh of the bench's field at 128^3 (tools/bench_mesh_export.py; decimated to a quarter).
Prints ONE JSON line.

    python tools/bench_mesh_clean.py [--precision bf16|f32] [--reps 5]

Times are HIP events around the whole call (median of --reps after one warm-up call); clean_mesh and decimate_mesh read
a count back per round, so their times include those synchronisations."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _export_bench():
    spec = importlib.util.spec_from_file_location("bench_mesh_export", os.path.join(ROOT, "tools", "bench_mesh_export.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bumpy(dev):
    from src.latent_nerf.raymarching import marching_cubes
    x = torch.linspace(-1, 1, 64, device=dev)
    X, Y, Z = torch.meshgrid(x, x, x, indexing="ij")
    sdf = 0.6 - torch.sqrt(X * X + Y * Y + Z * Z) + 0.04 * torch.sin(9 * X) * torch.sin(9 * Y) * torch.sin(9 * Z)
    v, f, _ = marching_cubes(sdf.contiguous(), 0.0, (-1, -1, -1), (1, 1, 1))
    return v, f


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from src.latent_nerf.raymarching import clean_mesh, decimate_mesh, marching_cubes, smooth_mesh
    assert torch.cuda.is_available(), "bench_mesh_clean needs the GPU"
    dev = torch.device("cuda:0")
    E = _export_bench()
    net, cfg = E.field(dev, args.precision)
    b = net.bound
    ev, ef, _ = marching_cubes(net.density_lattice(128, S=128), float(cfg.density_thresh), (-b,) * 3, (b,) * 3)
    bv, bf = bumpy(dev)
    res = []
    for name, v, f, target in (("bumpy", bv, bf, 2000), ("export", ev, ef, int(ef.shape[0]) // 4)):
        st, ds = {}, {}
        t_c, (cv, cf, _) = E.timed(lambda: clean_mesh(v, f, 8, 0.05, stats=st), args.reps)
        t_s, _ = E.timed(lambda: smooth_mesh(v, f, 10), args.reps)
        t_d, (dv, df, _) = E.timed(lambda: decimate_mesh(v, f, target, stats=ds), args.reps)
        res.append({"mesh": name, "V": int(v.shape[0]), "F": int(f.shape[0]), "clean_ms": round(t_c, 3),
                    "components": st["components"], "kept": st["kept"], "label_rounds": st["rounds"],
                    "F_clean": int(cf.shape[0]), "smooth10_ms": round(t_s, 3), "decimate_ms": round(t_d, 3),
                    "decimate_target": target, "F_decimated": int(df.shape[0]), "decimate_rounds": ds["rounds"]})
    print(json.dumps({"tool": "bench_mesh_clean", "precision": args.precision, "reps": args.reps,
                      "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
