"""Cost of the orientation regulariser (optim.lambda_orient) on the bench configuration: 64 x 64 rays (4 096), 128^3
occupancy (the analytic sphere), the bench's fixed view, sample capacity and learning rate, one view per step, the seeded
synthetic guidance -- in ONE process.  Prints ONE JSON line (and writes it to --out).

    python tools/bench_orient.py [--steps 200] [--reps 5] [--out profiles/orient_bench.json]

What is timed.
1. The kernels, on a shaded step's own march and field outputs: lnerf_shade_fd_forward / _backward (the baseline) against
   lnerf_shade_fd_orient_forward / _backward with a gradient for the term, 20 launches of one entry point captured into
   a graph of their own (a launch from Python costs more host time than these kernels run), the graph replayed between
   two HIP events after a warm-up, median of --reps.
2. One SHADED captured trainer step (Trainer._graphed_step: pose upload + one graph launch) with lambda_orient = 0 against
   1e-2: windows of --steps steps between two HIP events on the trainer's stream, after the form has run eagerly, been
   captured and replayed --steps times; median of --reps windows.  The trainers run one after the other (they share the
   device's scatter workspace), the baseline once before and once after: the two baseline figures show the drift."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "latent-nerf-test_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_shading import _captured_ms, _window  # noqa: E402


def _trainer(bench, dev, precision, root, name, lambda_orient):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    cfg = apply_overrides(TrainConfig(), {
        "log.exp_name": name, "log.exp_root": root, "render.train_h": bench.H, "render.train_w": bench.W,
        "render.grid_size": bench.GRID, "render.eval_h": 8, "render.eval_w": 8, "log.eval_size": 1, "log.full_eval_size": 1,
        "log.save_interval": 10 ** 9, "log.quiet": True, "optim.lr": bench.LR, "optim.fp16": precision == "bf16",
        "guide.text": "bench", "optim.start_shading_iter": 1, "optim.lambda_orient": lambda_orient})
    cfg.render.train_pose = (60.0, 0.0, 1.25, bench.FOVY)
    cfg.render.max_samples = bench.BENCH_CAPACITY
    tr = Trainer(cfg, device=dev)
    bench.sphere_scene(tr.nerf)
    tr.nerf.iter_density = 16
    tr.nerf.train()
    return tr


def shaded_step_ms(bench, dev, precision, root, name, lambda_orient, steps, reps, kernels=False):
    """Median ms of a captured shaded step; kernels=True: also the four entry points on the last step's buffers."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as rm
    tr = _trainer(bench, dev, precision, root, name, lambda_orient)
    net = tr.nerf
    tr._shaded = True

    def replay():
        tr.train_step += 1
        tr._graphed_step()

    tr.stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(tr.stream):
        for _ in range(2):
            tr.train_step += 1
            tr.optimizer.zero_grad()
            tr._eager_step()
        tr._capture()
        _window(replay, steps)
        windows = [_window(replay, steps) for _ in range(reps)]
    torch.cuda.current_stream().wait_stream(tr.stream)
    torch.cuda.synchronize()
    res = {"lambda_orient": lambda_orient, "shaded_step_ms": round(statistics.median(windows), 4),
           "windows_ms": [round(v, 4) for v in windows], "captures": tr.graph_stats["captures"]}
    if kernels:
        march = net._march
        cap, N = march.capacity, march.rays.shape[0]
        rays_d = next(b for b in net._ray_slots if b is not None)[2]
        shade, eps = tr._static["shade"], 1e-2
        with torch.no_grad():
            m_dev = march.counter[0:1]
            pts7, m7 = rm.fd_points(march.xyzs, net.bound, eps, cap, m_dev)
            s7, c7 = net.field(pts7, 7 * cap, m7, 7 * cap)
            C, inv = c7.shape[1], 1.0 / (2.0 * eps)
            sc, co, ori = torch.empty(cap, device=dev), torch.empty(cap, C, device=dev), torch.empty(N, device=dev)
            dsc, dco, dori = torch.randn(cap, device=dev), torch.randn(cap, C, device=dev), torch.randn(N, device=dev)
            d7, dr7 = torch.empty_like(s7), torch.empty_like(c7)
            P, call = rm._p, B.call
            head = (P(s7), P(c7), C, P(march.rays), N, N, P(shade), 1, inv)
            tail = (P(march.deltas), P(rays_d), float(net.density_scale), 1e-4)
            t = {
                "shade_forward_ms": _captured_ms(
                    lambda: call("lnerf_shade_fd_forward", *head, P(sc), P(co), rm._stream()), 20, reps),
                "shade_orient_forward_ms": _captured_ms(
                    lambda: call("lnerf_shade_fd_orient_forward", *head, *tail, P(sc), P(co), P(ori), rm._stream()), 20, reps),
                "shade_backward_ms": _captured_ms(
                    lambda: call("lnerf_shade_fd_backward", *head, P(dsc), P(dco), P(d7), P(dr7), rm._stream()), 20, reps),
                "shade_orient_backward_ms": _captured_ms(
                    lambda: call("lnerf_shade_fd_orient_backward", *head, P(dsc), P(dco), *tail, P(dori), P(d7), P(dr7),
                                 rm._stream()), 20, reps),
            }
        res["kernels"] = dict({k: round(v, 4) for k, v in t.items()}, rays=N, sample_capacity=cap,
                              samples=int(march.counter[0].item()), channels=C)
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_orient needs the GPU"
    import bench
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="lnerf_bench_orient_")
    try:
        runs = [shaded_step_ms(bench, dev, args.precision, root, "off_a", 0.0, args.steps, args.reps),
                shaded_step_ms(bench, dev, args.precision, root, "on", 1e-2, args.steps, args.reps, kernels=True),
                shaded_step_ms(bench, dev, args.precision, root, "off_b", 0.0, args.steps, args.reps)]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    off = statistics.mean([runs[0]["shaded_step_ms"], runs[2]["shaded_step_ms"]])
    line = json.dumps({"tool": "bench_orient", "precision": args.precision, "steps_per_window": args.steps, "reps": args.reps,
                       "device": torch.cuda.get_device_name(0), "kernels": runs[1].pop("kernels"),
                       "shaded_step_ms_lambda_0": [runs[0]["shaded_step_ms"], runs[2]["shaded_step_ms"]],
                       "shaded_step_ms_lambda_1e-2": runs[1]["shaded_step_ms"],
                       "step_ratio": round(runs[1]["shaded_step_ms"] / off, 4), "runs": runs})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
