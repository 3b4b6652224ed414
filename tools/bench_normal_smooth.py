"""Cost of the 2D normal-smoothness term (optim.lambda_normal_smooth) on a SHADED step of the bench configuration: 64 x 64
rays (4 096), 128^3 occupancy (the analytic sphere), the bench's fixed view, sample capacity and learning rate, one view
per step, the seeded synthetic guidance -- in ONE process.  Prints ONE JSON line (and writes it to --out).  The cost is
recorded, not gated.

    python tools/bench_normal_smooth.py [--steps 200] [--reps 5] [--out profiles/normal_smooth_bench.json]

What is timed (the method of tools/bench_distortion.py).
1. The kernels alone, on a shaded step's own march and 7-point field outputs: lnerf_normal_image_forward / _backward and
   lnerf_image_smooth_forward / _backward, beside lnerf_shade_fd_forward on the same samples for scale, the fill of the
   node's dsigmas7 and the one add over the 7 cap rows that autograd makes where the term's gradient meets the shade
   node's; 20 launches of one entry point captured into a graph of their own, the graph replayed between two HIP events
   after a warm-up, median of --reps.
2. One captured SHADED trainer step (Trainer._graphed_step with start_shading_iter = 1) with lambda_normal_smooth = 0
   against 0.5: windows of --steps steps between two HIP events on the trainer's stream, after the step has run eagerly,
   been captured and replayed --steps times; median of --reps windows.  The trainers run one after the other (they share
   the device's scatter workspace), the baseline once before and once after: the two baseline figures show the drift."""
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

EPS = 1e-2


def _trainer(bench, dev, precision, root, name, lam):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    cfg = apply_overrides(TrainConfig(), {
        "log.exp_name": name, "log.exp_root": root, "render.train_h": bench.H, "render.train_w": bench.W,
        "render.grid_size": bench.GRID, "render.eval_h": 8, "render.eval_w": 8, "log.eval_size": 1, "log.full_eval_size": 1,
        "log.save_interval": 10 ** 9, "log.quiet": True, "optim.lr": bench.LR, "optim.fp16": precision == "bf16",
        "guide.text": "bench", "optim.start_shading_iter": 1, "optim.lambda_normal_smooth": lam})
    cfg.render.train_pose = (60.0, 0.0, 1.25, bench.FOVY)
    cfg.render.max_samples = bench.BENCH_CAPACITY
    tr = Trainer(cfg, device=dev)
    bench.sphere_scene(tr.nerf)
    tr.nerf.iter_density = 16
    tr.nerf.train()
    return tr


def step_ms(bench, dev, precision, root, name, lam, steps, reps, kernels=False):
    """Median ms of a captured shaded step; kernels=True: also the entry points on the last step's buffers."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as rm
    tr = _trainer(bench, dev, precision, root, name, lam)
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
    res = {"lambda_normal_smooth": lam, "step_ms": round(statistics.median(windows), 4),
           "windows_ms": [round(v, 4) for v in windows], "captures": tr.graph_stats["captures"]}
    if kernels:
        march = net._march
        cap, N = march.capacity, march.rays.shape[0]
        H, W = bench.H, bench.W
        with torch.no_grad():
            m_dev = march.counter[0:1]
            pts7, m7 = rm.fd_points(march.xyzs, net.bound, EPS, cap, m_dev)
            s7, c7 = net.field(pts7, 7 * cap, m7, 7 * cap)
            C, inv, ds = c7.shape[1], 1.0 / (2.0 * EPS), float(net.density_scale)
            image, d_image = torch.empty(N, 3, device=dev), torch.randn(N, 3, device=dev) / N
            d7, other = torch.empty_like(s7), torch.randn_like(s7)
            pairs, d_pairs = torch.empty(1, H, W, 2, device=dev), torch.full((1, H, W, 2), 0.5 / (H * (W - 1) * 3), device=dev)
            sc, co = torch.empty(cap, device=dev), torch.empty(cap, C, device=dev)
            P, call = rm._p, B.call
            head = (P(s7), P(march.deltas), P(march.rays), N, inv, ds, 1e-4)
            call("lnerf_normal_image_forward", *head, P(image), rm._stream())           # (the backward reads its output)
            t = {
                "normal_image_forward_ms": _captured_ms(
                    lambda: call("lnerf_normal_image_forward", *head, P(image), rm._stream()), 20, reps),
                "normal_image_backward_ms": _captured_ms(
                    lambda: call("lnerf_normal_image_backward", *head, P(d_image), P(image), P(d7), rm._stream()), 20, reps),
                "image_smooth_forward_ms": _captured_ms(
                    lambda: call("lnerf_image_smooth_forward", P(image), 1, H, W, 3, P(pairs), rm._stream()), 20, reps),
                "image_smooth_backward_ms": _captured_ms(
                    lambda: call("lnerf_image_smooth_backward", P(image), 1, H, W, 3, P(d_pairs), P(d_image), rm._stream()),
                    20, reps),
                "shade_fd_forward_ms": _captured_ms(
                    lambda: call("lnerf_shade_fd_forward", P(s7), P(c7), C, P(march.rays), N, N, P(tr._static["shade"]), 1,
                                 inv, P(sc), P(co), rm._stream()), 20, reps),
                "dsigmas7_fill_ms": _captured_ms(lambda: d7.zero_(), 20, reps),
                "dsigmas7_add_ms": _captured_ms(lambda: torch.add(d7, other), 20, reps),
            }
        res["kernels"] = dict({k: round(v, 4) for k, v in t.items()}, rays=N, sample_capacity=cap,
                              samples=int(march.counter[0].item()), channels=C,
                              mean_abs_normal=float(image.norm(dim=-1).mean().item()))
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normal_smooth_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_normal_smooth needs the GPU"
    import bench
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="lnerf_bench_normal_smooth_")
    try:
        runs = [step_ms(bench, dev, args.precision, root, "off_a", 0.0, args.steps, args.reps),
                step_ms(bench, dev, args.precision, root, "on", 0.5, args.steps, args.reps, kernels=True),
                step_ms(bench, dev, args.precision, root, "off_b", 0.0, args.steps, args.reps)]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    off = statistics.mean([runs[0]["step_ms"], runs[2]["step_ms"]])
    line = json.dumps({"tool": "bench_normal_smooth", "precision": args.precision, "steps_per_window": args.steps,
                       "reps": args.reps, "device": torch.cuda.get_device_name(0), "kernels": runs[1].pop("kernels"),
                       "shaded_step_ms_lambda_0": [runs[0]["step_ms"], runs[2]["step_ms"]],
                       "shaded_step_ms_lambda_0.5": runs[1]["step_ms"],
                       "step_ratio": round(runs[1]["step_ms"] / off, 4), "runs": runs})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
