"""Cost of the distortion loss (optim.lambda_distortion) on the bench configuration: 64 x 64 rays (4 096), 128^3 occupancy
(the analytic sphere), the bench's fixed view, sample capacity and learning rate, one view per step, the seeded synthetic
guidance -- in ONE process.  Prints ONE JSON line (and writes it to --out).  The cost is recorded, not gated.

    python tools/bench_distortion.py [--steps 200] [--reps 5] [--out profiles/distortion_bench.json]

What is timed.
1. The kernels alone, on a step's own march and field outputs: lnerf_distortion_forward and lnerf_distortion_backward,
   beside lnerf_composite_rays_train_forward on the same samples for scale and the one add over the densities' gradient
   that autograd makes where the term's gradient meets the compositing's; 20 launches of one entry point captured into a
   graph of their own (a launch from Python costs more host time than these kernels run), the graph replayed between two
   HIP events after a warm-up, median of --reps.
2. One captured trainer step (Trainer._graphed_step: pose upload + one graph launch) with lambda_distortion = 0 against
   1e-2: windows of --steps steps between two HIP events on the trainer's stream, after the step has run eagerly, been
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


def _trainer(bench, dev, precision, root, name, lambda_distortion):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    from src.latent_nerf.training.trainer import Trainer
    cfg = apply_overrides(TrainConfig(), {
        "log.exp_name": name, "log.exp_root": root, "render.train_h": bench.H, "render.train_w": bench.W,
        "render.grid_size": bench.GRID, "render.eval_h": 8, "render.eval_w": 8, "log.eval_size": 1, "log.full_eval_size": 1,
        "log.save_interval": 10 ** 9, "log.quiet": True, "optim.lr": bench.LR, "optim.fp16": precision == "bf16",
        "guide.text": "bench", "optim.lambda_distortion": lambda_distortion})
    cfg.render.train_pose = (60.0, 0.0, 1.25, bench.FOVY)
    cfg.render.max_samples = bench.BENCH_CAPACITY
    tr = Trainer(cfg, device=dev)
    bench.sphere_scene(tr.nerf)
    tr.nerf.iter_density = 16
    tr.nerf.train()
    return tr


def step_ms(bench, dev, precision, root, name, lambda_distortion, steps, reps, kernels=False):
    """Median ms of a captured step; kernels=True: also the entry points on the last step's buffers."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as rm
    tr = _trainer(bench, dev, precision, root, name, lambda_distortion)
    net = tr.nerf
    tr._shaded = False

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
    res = {"lambda_distortion": lambda_distortion, "step_ms": round(statistics.median(windows), 4),
           "windows_ms": [round(v, 4) for v in windows], "captures": tr.graph_stats["captures"]}
    if kernels:
        march = net._march
        cap, N = march.capacity, march.rays.shape[0]
        with torch.no_grad():
            sig, rgb = net.field(march.xyzs, cap, march.counter[0:1], cap)
            sig = (net.density_scale * sig).contiguous()
            C = rgb.shape[1]
            loss, sums = torch.empty(N, device=dev), torch.empty(N, 2, device=dev)
            d_loss, dsig, other = torch.full((N,), 1e-2 / N, device=dev), torch.empty_like(sig), torch.randn_like(sig)
            ws, depth, image = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, C, device=dev)
            P, call = rm._p, B.call
            head = (P(sig), P(march.deltas), P(march.rays), N, 1e-4)
            call("lnerf_distortion_forward", *head, P(loss), P(sums), rm._stream())      # (the backward reads its outputs)
            t = {
                "distortion_forward_ms": _captured_ms(
                    lambda: call("lnerf_distortion_forward", *head, P(loss), P(sums), rm._stream()), 20, reps),
                "distortion_backward_ms": _captured_ms(
                    lambda: call("lnerf_distortion_backward", *head, P(d_loss), P(loss), P(sums), P(dsig), rm._stream()),
                    20, reps),
                "composite_forward_ms": _captured_ms(
                    lambda: call("lnerf_composite_rays_train_forward", P(sig), P(rgb), P(march.deltas), P(march.rays), N, C,
                                 1e-4, None, P(ws), P(depth), P(image), rm._stream()), 20, reps),
                "dsigmas_add_ms": _captured_ms(lambda: torch.add(dsig, other), 20, reps),
            }
        res["kernels"] = dict({k: round(v, 4) for k, v in t.items()}, rays=N, sample_capacity=cap,
                              samples=int(march.counter[0].item()), channels=C,
                              mean_loss=float(loss.mean().item()))
    del tr
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "f32"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distortion_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_distortion needs the GPU"
    import bench
    dev = torch.device("cuda:0")
    root = tempfile.mkdtemp(prefix="lnerf_bench_distortion_")
    try:
        runs = [step_ms(bench, dev, args.precision, root, "off_a", 0.0, args.steps, args.reps),
                step_ms(bench, dev, args.precision, root, "on", 1e-2, args.steps, args.reps, kernels=True),
                step_ms(bench, dev, args.precision, root, "off_b", 0.0, args.steps, args.reps)]
    finally:
        shutil.rmtree(root, ignore_errors=True)
    off = statistics.mean([runs[0]["step_ms"], runs[2]["step_ms"]])
    line = json.dumps({"tool": "bench_distortion", "precision": args.precision, "steps_per_window": args.steps,
                       "reps": args.reps, "device": torch.cuda.get_device_name(0), "kernels": runs[1].pop("kernels"),
                       "step_ms_lambda_0": [runs[0]["step_ms"], runs[2]["step_ms"]],
                       "step_ms_lambda_1e-2": runs[1]["step_ms"],
                       "step_ratio": round(runs[1]["step_ms"] / off, 4), "runs": runs})
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
