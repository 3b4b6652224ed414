"""Cost of a shaded training step (optim.start_shading_iter) on the bench configuration: 64 x 64 rays, 128^3 occupancy (the
analytic sphere), the bench's fixed view, sample capacity and learning rate, one view per step, the seeded synthetic
guidance, sparsity term on -- bf16 and f32 in ONE process.  Prints ONE JSON line (and writes it to --out).

    python tools/bench_shading.py [--steps 200] [--reps 5] [--out profiles/shading_bench.json]

What is timed.  The trainer's captured steps (Trainer._graphed_step: pose upload + one graph launch), plain and shaded, in
alternating windows of --steps steps between two HIP events on the trainer's stream, after both forms have run eagerly,
been captured and replayed --steps times; the median of --reps windows per form.  No occupancy refresh falls inside a
window.  The kind inside the shaded form (lambertian / textureless) is data of the same graph: one figure serves both.
The three new launches (lnerf_fd_points, lnerf_shade_fd_forward, lnerf_shade_fd_backward) are then timed alone on the
last step's own march and field outputs: 20 launches of one entry point captured into a graph of their own (a launch
from Python costs more host time than these kernels run), the graph replayed between two events, median of --reps:
`new_kernels_ms` and their share of the shaded step.  `field_forward_ms` / `field_forward_x7_rows_ms` time the field's
forward (gather + MLP) alone at the plain and at the shaded row count, the same way: the seven-fold part of the step as
far as it can be timed outside the step."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _window(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def _captured_ms(fn, n, reps):
    """ms per call of fn(): n calls captured into one graph (fn only enqueues launches), replayed between two events."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    _window(g.replay, 3)   # warm-up
    return statistics.median(_window(g.replay, 5) for _ in range(reps)) / n


def _trainer(bench, dev, precision, root):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    cfg = apply_overrides(TrainConfig(), {
        "log.exp_name": "shading_%s" % precision, "log.exp_root": root, "render.train_h": bench.H, "render.train_w": bench.W,
        "render.grid_size": bench.GRID, "render.eval_h": 8, "render.eval_w": 8, "log.eval_size": 1, "log.full_eval_size": 1,
        "log.save_interval": 10 ** 9, "log.quiet": True, "optim.lr": bench.LR, "optim.fp16": precision == "bf16",
        "guide.text": "bench", "optim.start_shading_iter": 1})
    cfg.render.train_pose = (60.0, 0.0, 1.25, bench.FOVY)
    cfg.render.max_samples = bench.BENCH_CAPACITY
    tr = Trainer(cfg, device=dev)
    bench.sphere_scene(tr.nerf)
    tr.nerf.iter_density = 16
    tr.nerf.train()
    return tr


def measure(bench, dev, precision, steps, reps, root):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as rm
    tr = _trainer(bench, dev, precision, root)
    net = tr.nerf

    def eager(shaded):
        tr._shaded = shaded
        tr.train_step += 1
        tr.optimizer.zero_grad()
        tr._eager_step()

    def replay(shaded):
        tr._shaded = shaded
        tr.train_step += 1
        tr._graphed_step()

    tr.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(tr.stream):
        for shaded in (False, True):
            for _ in range(2):
                eager(shaded)
            tr._shaded = shaded
            tr._capture()
        tr._gstep_ws = tr._scatter_ws_state()
        for shaded in (False, True):
            _window(lambda: replay(shaded), steps)
        plain, shaded_w = [], []
        for _ in range(reps):            # alternating windows: drift of the shared host hits both forms alike
            plain.append(_window(lambda: replay(False), steps))
            shaded_w.append(_window(lambda: replay(True), steps))
        plain_ms, shaded_ms = statistics.median(plain), statistics.median(shaded_w)
        # the three new launches alone, on the last step's own buffers
        march = net._march
        cap, N = march.capacity, march.rays.shape[0]
        M = int(march.counter[0].item())
        shade = tr._static["shade"]
        eps = 1e-2
    torch.cuda.current_stream().wait_stream(tr.stream)
    torch.cuda.synchronize()
    with torch.no_grad():
        m_dev = march.counter[0:1]
        pts7, m7 = rm.fd_points(march.xyzs, net.bound, eps, cap, m_dev)
        s7, c7 = net.field(pts7, 7 * cap, m7, 7 * cap)
        C, inv = c7.shape[1], 1.0 / (2.0 * eps)
        sc, co = torch.empty(cap, device=dev), torch.empty(cap, C, device=dev)
        dsc, dco = torch.randn(cap, device=dev), torch.randn(cap, C, device=dev)
        d7, dr7 = torch.empty_like(s7), torch.empty_like(c7)
        P, call = rm._p, B.call
        t_pts = _captured_ms(lambda: call("lnerf_fd_points", P(march.xyzs), float(net.bound), eps, cap, P(m_dev), P(pts7), P(m7),
                                     rm._stream()), 20, reps)
        t_fwd = _captured_ms(lambda: call("lnerf_shade_fd_forward", P(s7), P(c7), C, P(march.rays), N, N, P(shade), 1, inv, P(sc),
                                     P(co), rm._stream()), 20, reps)
        t_bwd = _captured_ms(lambda: call("lnerf_shade_fd_backward", P(s7), P(c7), C, P(march.rays), N, N, P(shade), 1, inv,
                                     P(dsc), P(dco), P(d7), P(dr7), rm._stream()), 20, reps)
        # (two launches of 0.07 ms and more per call: plain windows of 20 calls are device-bound)
        t_field7 = statistics.median(_window(lambda: net.field(pts7, 7 * cap, m7, 7 * cap), 20) for _ in range(reps + 1))
        t_field1 = statistics.median(_window(lambda: net.field(march.xyzs, cap, m_dev, cap), 20) for _ in range(reps + 1))
    new = t_pts + t_fwd + t_bwd
    return {"precision": precision, "gridtype": net.encoder.levels.gridtype, "samples_per_view": M, "sample_capacity": cap,
            "plain_step_ms": round(plain_ms, 4), "shaded_step_ms": round(shaded_ms, 4),
            "shaded_over_plain": round(shaded_ms / plain_ms, 3),
            "plain_windows_ms": [round(v, 4) for v in plain], "shaded_windows_ms": [round(v, 4) for v in shaded_w],
            "fd_points_ms": round(t_pts, 4), "shade_forward_ms": round(t_fwd, 4),
            "shade_backward_ms": round(t_bwd, 4),
            "new_kernels_ms": round(new, 4), "new_kernels_share_of_shaded_step": round(new / shaded_ms, 4),
            "field_forward_ms": round(t_field1, 4), "field_forward_x7_rows_ms": round(t_field7, 4),
            "captures": tr.graph_stats["captures"], "whole_step_graph": bool(tr._whole)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shading_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_shading needs the GPU"
    import bench
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="lnerf_bench_shading_")
    try:
        res = [measure(bench, dev, precision, args.steps, args.reps, root) for precision in ("bf16", "f32")]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    line = json.dumps({"tool": "bench_shading", "steps_per_window": args.steps, "reps": args.reps,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
