"""Mesh export timing on the bench's field: the density lattice query (NeRFRenderer.density_lattice, S = 128 chunks) and
marching cubes (raymarching.marching_cubes: count pass, scan, one host read of the counts, emit pass) at 128^3, 256^3
and 512^3.  Prints ONE JSON line.

    python tools/bench_mesh_export.py [--precision bf16|f32] [--reps 5]

Field: bench.py's (seed 0, Linear-default MLP, table N(0, 0.1), density blob; bf16 runs the blocked bf16 default), iso =
density_thresh (10).  Times are HIP events around the call (median of --reps after one warm-up call per size).
mc_bytes is the marching-cubes traffic model: the volume read by the count and the emit pass (2 x 4 B per working point),
the per-point words (written, rewritten and read: 4 x 4 B), and the outputs (24 B per vertex with its normal, 12 B per
triangle); mc_GBps = mc_bytes / mc time.
--target-faces N[,N...]: also time the decimation of each marching-cubes mesh to N faces (raymarching.decimate_mesh: one
host read per round, so the time includes those synchronisations) with its round and collapse counts, and, on the
largest lattice, Latent-Paint's rasteriser (lnerf_raster_prepare + lnerf_rasterize at 512 x 512, one view) on the
undecimated and on each decimated mesh.
--atlas charts [--atlas-resolution 1024]: also time raymarching.chart_atlas on each marching-cubes mesh and on each
decimated one (the whole call: label rounds with one host read each, the host-side packing, the fold check), with
its chart, round, shrink (k) and eviction counts and the share of the texture's texels that a face covers.  Only
sizes >= 256 are run, to keep the leg short.
--clean: also time raymarching.clean_mesh (the upstream exporter's 8 faces / 0.05 of the diagonal: label rounds with one
host read each, the host-side keep rule, the filter) and smooth_mesh(iterations=10) on each marching-cubes mesh."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def field(dev, precision):
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models.network_grid import NeRFNetwork
    torch.manual_seed(0)
    cfg = RenderConfig(grid_size=128, train_h=64, train_w=64, mlp_precision=precision, table_dtype=precision,
                       gridtype="blocked" if precision == "bf16" else "hash")
    net = NeRFNetwork(cfg)
    net.encoder.embeddings.data.normal_(0, 0.1)
    return net.to(dev).eval(), cfg


def timed(fn, reps):
    fn()   # warm-up
    torch.cuda.synchronize()
    times, out = [], None
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), out


def raster_ms(dev, verts, faces, reps):
    """Latent-Paint's rasteriser on one view of the mesh, scaled into the unit box: prepare + rasterize, 512 x 512."""
    from src.latent_paint.models.render import Renderer
    r = Renderer(dev, dim=(512, 512))
    v = (verts / verts.abs().max()).contiguous()
    t, _ = timed(lambda: r._rasterize(v, faces, 1.0, 0.5, 2.0, 0.0, (512, 512)), reps)
    return t


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="128,256,512")
    ap.add_argument("--target-faces", default="", help="comma-separated face targets of a decimation leg (empty: none)")
    ap.add_argument("--atlas", default="", choices=["", "charts"], help="charts: also time the chart atlas of every mesh")
    ap.add_argument("--atlas-resolution", type=int, default=1024)
    ap.add_argument("--clean", action="store_true", help="also time clean_mesh and 10 smoothing iterations of every mesh")
    args = ap.parse_args()
    from src.latent_nerf.raymarching import chart_atlas, clean_mesh, decimate_mesh, marching_cubes, smooth_mesh, uv_raster
    assert torch.cuda.is_available(), "bench_mesh_export needs the GPU"
    dev = torch.device("cuda:0")
    net, cfg = field(dev, args.precision)
    iso = float(cfg.density_thresh)
    b = net.bound
    targets = [int(t) for t in args.target_faces.split(",") if t.strip()]
    sizes = [int(s) for s in args.sizes.split(",")]
    res = []
    for R in sizes:
        t_q, vol = timed(lambda: net.density_lattice(R, S=128), args.reps)
        t_mc, (v, f, n) = timed(lambda: marching_cubes(vol, iso, (-b,) * 3, (b,) * 3, close_boundary=True), args.reps)
        N = (R + 2) ** 3
        V, F = int(v.shape[0]), int(f.shape[0])
        mc_bytes = 8 * N + 16 * N + 24 * V + 12 * F
        row = {"resolution": R, "points": R ** 3, "query_ms": round(t_q, 4), "mc_ms": round(t_mc, 4), "V": V, "F": F,
               "mc_bytes": mc_bytes, "mc_GBps": round(mc_bytes / (t_mc * 1e-3) / 1e9, 1),
               "query_Mpts_per_s": round(R ** 3 / (t_q * 1e-3) / 1e6, 1)}
        del vol
        if args.clean:
            st = {}
            t_c, (_, cf, _) = timed(lambda: clean_mesh(v, f, 8, 0.05, stats=st), args.reps)
            t_s, _ = timed(lambda: smooth_mesh(v, f, 10), args.reps)
            row["clean"] = {"ms": round(t_c, 3), "components": st["components"], "kept": st["kept"],
                            "rounds": st["rounds"], "F_out": int(cf.shape[0])}
            row["smooth"] = {"iterations": 10, "ms": round(t_s, 3)}
        meshes = [(F, v, f)]
        for N in targets:
            if N >= F:
                continue
            st = {}
            t_d, (dv, df, _) = timed(lambda: decimate_mesh(v, f, N, stats=st), args.reps)
            row.setdefault("decimate", []).append({"target": N, "ms": round(t_d, 3), "F_out": int(df.shape[0]),
                                                   "V_out": int(dv.shape[0]), "rounds": st["rounds"],
                                                   "collapses": st["collapses"]})
            meshes.append((N, dv, df))
        if args.atlas == "charts" and R >= 256:
            for label, mv, mf in meshes:
                st = {}
                t_a, (vt, ft, _) = timed(lambda: chart_atlas(mv, mf, args.atlas_resolution, stats=st), args.reps)
                covered = int(uv_raster(mv, mf, vt, ft, args.atlas_resolution)[1].shape[0])
                row.setdefault("atlas", []).append(
                    {"F": int(mf.shape[0]), "resolution": args.atlas_resolution, "ms": round(t_a, 3), "charts": st["charts"],
                     "rounds": st["rounds"], "k": st["k"], "evicted": st["evicted"], "n_vt": int(vt.shape[0]),
                     "scale": round(st["scale"], 3), "covered": round(covered / args.atlas_resolution ** 2, 4)})
        if targets and R == sizes[-1]:
            row["raster_512_ms"] = {str(int(m[2].shape[0])): round(raster_ms(dev, m[1], m[2], args.reps), 3)
                                    for m in meshes}
        res.append(row)
        del v, f, n, meshes
        torch.cuda.empty_cache()
    print(json.dumps({"tool": "bench_mesh_export", "precision": args.precision, "iso": iso, "reps": args.reps,
                      "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
