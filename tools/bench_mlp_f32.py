"""GPU time of the exact-f32 MLP (csrc/mlp.hip) at the benchmark's step: one JSON line.

    LNERF_HIP_LIB=<library> python tools/bench_mlp_f32.py [--tag NAME]

lnerf_mlp_forward and lnerf_mlp_backward (backward kernel + slab reduction), precision f32, out_dim 5, f32 features,
430 423 valid samples (*m_dev) of capacity 655 360 (m_host = level_stride): 20 warm-up calls, then 200 calls of each
with a pair of HIP events around every call; median, minimum and mean per call in microseconds.  Inputs are seeded and
ordinary (randn weights at the initialiser's scale, randn features, positions uniform in the box).  Compare libraries
by running one fresh process each, alternately (the library is chosen through LNERF_HIP_LIB)."""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "latent-nerf-test_amd")]

import torch  # noqa: E402
from src.latent_nerf.raymarching import backend as B  # noqa: E402
from src.latent_nerf.raymarching.raymarching import _stream  # noqa: E402

M, CAPACITY, OUT_DIM = 430423, 655360, 5
WARMUP, CALLS = 20, 200

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="")
args = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(7)


def p(t):
    return ctypes.c_void_p(t.data_ptr())


feat = torch.randn(16, CAPACITY, 2, generator=g).to(dev)
xyz = (torch.rand(CAPACITY, 3, generator=g) * 2.0 - 1.0).to(dev)
W = []
for n_out, n_in in ((64, 32), (64, 64), (OUT_DIM, 64)):
    W += [(torch.randn(n_out, n_in, generator=g) / math.sqrt(n_in)).to(dev),
          (torch.randn(n_out, generator=g) / math.sqrt(n_in)).to(dev)]
dsigmas, drgbs = torch.randn(CAPACITY, generator=g).to(dev), torch.randn(CAPACITY, OUT_DIM - 1, generator=g).to(dev)
sigmas, rgbs = torch.zeros(CAPACITY, device=dev), torch.zeros(CAPACITY, OUT_DIM - 1, device=dev)
dfeat = torch.zeros(16, CAPACITY, 2, device=dev)
grads = [torch.zeros_like(t) for t in W]
ws = torch.zeros(int(B.get_lib().lnerf_mlp_backward_workspace_bytes(OUT_DIM)), dtype=torch.uint8, device=dev)
m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
head = (p(feat), B.F32, CAPACITY, p(xyz), *[p(t) for t in W], OUT_DIM, 5.0, 0.2, CAPACITY, p(m_dev))


def forward():
    B.call("lnerf_mlp_forward", *head, p(sigmas), p(rgbs), B.F32, None, 0, _stream())


def backward():
    B.call("lnerf_mlp_backward", *head, p(sigmas), p(dsigmas), p(drgbs), p(dfeat), *[p(t) for t in grads], 0, p(ws),
           ws.numel(), B.F32, None, 0, _stream())


def per_call_us(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(CALLS)]
    for e0, e1 in events:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    ts = [e0.elapsed_time(e1) * 1e3 for e0, e1 in events]
    return {"median": round(statistics.median(ts), 2), "min": round(min(ts), 2), "mean": round(statistics.fmean(ts), 2)}


out = {"tag": args.tag, "build": B.get_lib().lnerf_build_info().decode(), "m": M, "capacity": CAPACITY,
       "warmup": WARMUP, "calls": CALLS, "forward_us": per_call_us(forward), "backward_us": per_call_us(backward)}
assert bool(torch.isfinite(rgbs[:M]).all()) and all(bool(torch.isfinite(t).all()) for t in grads)
print(json.dumps(out))
