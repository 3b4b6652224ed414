"""Step time of the Latent-Paint trainer (render, synthetic guidance, backward, Adam) on tests/golden/shapes/blub.obj.

    python tools/bench_paint_step.py [--root TREE] [--shading albedo|lambertian] [--batch 8] [--geometry] [--tag NAME]

Prints one JSON line: the median and the spread of `--windows` HIP-event windows of `--steps` trainer steps each, after
`--warmup` steps.  `--root` names the checkout whose package is imported (default: this one), so that a parent commit
can be timed by the same tool; `--shading` is only passed on to a tree that knows it.  profiles/meshshade_step.jsonl."""
import argparse
import json
import os
import statistics
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--shading", default="albedo")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--geometry", action="store_true", help="optim.disp_lr 5e-5 with render.antialias and the bilinear lookup")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    for p in (os.path.join(root, "latent-nerf-test_amd"), root):
        sys.path.insert(0, p)
    import torch
    from src.latent_nerf.raymarching import backend
    from src.latent_paint.configs.train_config import TrainConfig, apply_overrides
    from src.latent_paint.training.trainer import Trainer

    flat = {"log.exp_name": "bench", "log.exp_root": tempfile.mkdtemp(), "guide.text": "a goldfish",
            "guide.shape_path": os.path.join(HERE, "tests", "golden", "shapes", "blub.obj"),
            "render.batch_size": args.batch}
    if args.shading != "albedo":
        flat["render.shading"] = args.shading
    if args.geometry:
        flat.update({"optim.disp_lr": 5e-5, "render.antialias": True, "guide.texture_interpolation_mode": "bilinear"})
    tr = Trainer(apply_overrides(TrainConfig(), flat).validate(), device=torch.device("cuda:0"))
    tr.mesh_model.train()
    batches = iter(())

    def step():
        nonlocal batches
        data = next(batches, None)
        if data is None:
            batches = iter(tr.dataloaders["train"])
            data = next(batches)
        tr.optimizer.zero_grad()
        tr.train_render(data)
        tr.optimizer.step()

    for _ in range(args.warmup):
        step()
    times = []
    for _ in range(args.windows):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.steps):
            step()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / args.steps)
    print(json.dumps({"tool": "bench_paint_step", "tag": args.tag, "build": backend.get_lib().lnerf_build_info().decode(),
                      "shading": args.shading, "batch": args.batch, "geometry": bool(args.geometry),
                      "steps_per_window": args.steps, "ms_per_step_median": round(statistics.median(times), 4),
                      "ms_per_step_min": round(min(times), 4), "ms_per_step_max": round(max(times), 4)}))


if __name__ == "__main__":
    main()
