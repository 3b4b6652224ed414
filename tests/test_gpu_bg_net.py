"""lnerf_bg_forward / lnerf_bg_backward (csrc/bg.hip) against the float64 background net of tests/bg_reference.py, through
the C entry points: C = 1, 3, 4; one thread, the block edges and the grid-stride trips of the forward (more than
1024 * 256 rays) and of the backward (more than 1024 * 64 rays); a last tile of 1, 63, 64 live rows; accumulation into
non-zero gradient buffers; and the compositor's grad_bg fed straight into the backward.

The directions keep every hidden pre-activation clear of zero (tests/bg_reference.py, asserted in
tests/test_bg_reference_cpu.py and again here on the reference alone), so the f32 kernel takes the float64 branches.

Forward: |out - out64| <= 2^-24 (39 + 64 + 8) B,  B = sum_h |w2_ch| A_h + |b2_c|,  A_h the sum of the magnitudes of the
40 terms of pre-activation h: one rounding per accumulated term (39 + 64) plus the sine / cosine and product roundings.
Backward: every element of dw1, db1, dw2, db2 within 2^-24 (111 + 64 + number of 64-ray tiles) S, S the float64 sum over
rays of the magnitudes of that element's per-ray terms, every term expanded down to the products the kernel forms
(bg_reference.bg_backward_ref: hid enters with A, dh with sum_c |w2_ch dout_c|): 111 for the recomputed forward, 64 for the
tile's LDS sum, one per tile for the atomics, whatever their order.  Onto a non-zero buffer each of the atomics also
rounds relative to the prefill: + 2^-24 (tiles + 1) |prefill|.
Chained: dout is what lnerf_composite_rays_train_backward wrote, within COMPOSITE_TOL(k) |di_c| of the float64 grad_bg
(tests/test_gpu_composite.py); S is linear in |dout|, so the bound grows by S evaluated at that error.

Measured on an MI355X, worst error / tolerance (each test prints its own; run with -s):
  forward, every C and N (1 ... 262401):                          0.003
  backward into zeros, N = 1 ... 65601, (dw1, db1, dw2, db2):     0.017, 0.014, 0.006, 0.005  (N = 65601: 0.001 and below)
  backward onto a prefill, N = 1000:                              0.096, 0.028, 0.001, 0.001
  compositor's grad_bg -> backward (C = 3, N = 10):               0.008, 0.002, 0.003, 0.000
"""
import pytest
import torch

from oracle import nerf_oracle as O
from tests import bg_reference as R
from tests.composite_reference import COMPOSITE_TOL, composite_case, composite_reference

pytestmark = pytest.mark.gpu

POISON = 777.0
EXTRA = 3
FORWARD_N = (1, 255, 256, 257, 262144 + 257)
BACKWARD_N = (1, 63, 64, 65, 1000, 65536 + 65)
KEYS = ("w1", "b1", "w2", "b2")


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _relu_ok(C):
    assert R.relu_margin(R.bg_params(C)) > R.RELU_MARGIN


def _gpu_forward(dev, dirs, p, C, rows):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    out = torch.full((rows, C), POISON, device=dev)
    B.call("lnerf_bg_forward", _p(dirs), dirs.shape[0], _p(p["w1"]), _p(p["b1"]), _p(p["w2"]), _p(p["b2"]), C, _p(out),
           _stream())
    return out


def _gpu_backward(dev, dirs, N, p, C, dout, into):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    B.call("lnerf_bg_backward", _p(dirs), N, _p(p["w1"]), _p(p["b1"]), _p(p["w2"]), _p(p["b2"]), C, _p(dout),
           *[_p(into[k]) for k in KEYS], _stream())
    return {k: into[k].cpu() for k in KEYS}


def _ratios(got, want, tol):
    out = {}
    for k in KEYS:
        err = (got[k].double() - want[k]).abs()
        t = tol[k].reshape(err.shape)
        r = torch.where(t > 0, err / t.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err),
                                                                      torch.full_like(err, float("inf"))))
        out[k] = float(r.max())
    return out


@pytest.mark.parametrize("N", FORWARD_N)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_forward_matches_float64(dev, C, N):
    _relu_ok(C)
    p = R.bg_params(C)
    D = R.distinct_directions().shape[0]
    want, B = R.bg_forward_ref(R.distinct_directions(), p)                         # per distinct direction
    dirs = R.bg_directions(N).to(dev)
    out = _gpu_forward(dev, dirs, {k: v.to(dev) for k, v in p.items()}, C, N + EXTRA).cpu()
    assert bool((out[N:] == POISON).all())                                         # rows beyond N are untouched
    which = torch.arange(N) % D
    err = (out[:N].double() - want[which]).abs()
    tol = R.ULP * (39 + 64 + 8) * B[which]
    worst = float((err / tol).max())
    print("bg forward C=%d N=%d: worst error / tolerance %.3f" % (C, N, worst))
    assert worst <= 1.0, worst


def _backward_case(C, N):
    g = torch.Generator().manual_seed(100 * C + N % 97)
    dirs, p = R.bg_directions(N), R.bg_params(C)
    dout = torch.randn(N, C, generator=g)
    grads, S = R.bg_backward_ref(dirs, p, dout)
    return dirs, p, dout, grads, S


@pytest.mark.parametrize("N", BACKWARD_N)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_backward_matches_float64_autograd(dev, C, N):
    _relu_ok(C)
    dirs, p, dout, want, S = _backward_case(C, N)
    tiles = (N + 63) // 64
    pd = {k: v.to(dev) for k, v in p.items()}
    got = _gpu_backward(dev, dirs.to(dev), N, pd, C, dout.to(dev), {k: torch.zeros_like(pd[k]) for k in KEYS})
    worst = _ratios(got, want, {k: R.ULP * (111 + 64 + tiles) * S[k] for k in KEYS})
    print("bg backward C=%d N=%d (%d tiles): error / tolerance %s" % (C, N, tiles, {a: "%.3f" % b for a, b in worst.items()}))
    for k, r in worst.items():
        assert r <= 1.0, (k, r)


@pytest.mark.parametrize("C", [1, 3, 4])
def test_backward_accumulates_into_its_buffers(dev, C):
    """Into buffers pre-filled with a known non-zero tensor the result is prefill + gradient (include/lnerf_hip.h)."""
    _relu_ok(C)
    N = 1000
    dirs, p, dout, want, S = _backward_case(C, N)
    tiles = (N + 63) // 64
    g = torch.Generator().manual_seed(C)
    prefill = {k: torch.randn(p[k].shape, generator=g) * 3 for k in KEYS}
    pd = {k: v.to(dev) for k, v in p.items()}
    got = _gpu_backward(dev, dirs.to(dev), N, pd, C, dout.to(dev), {k: prefill[k].to(dev) for k in KEYS})
    tol = {k: R.ULP * ((111 + 64 + tiles) * S[k].reshape(p[k].shape) + (tiles + 1) * prefill[k].double().abs()) for k in KEYS}
    worst = _ratios(got, {k: prefill[k].double() + want[k] for k in KEYS}, tol)
    print("bg backward onto a prefill C=%d N=%d: error / tolerance %s" % (C, N, {a: "%.3f" % b for a, b in worst.items()}))
    for k, r in worst.items():
        assert r <= 1.0, (k, r)
        assert float((got[k] - prefill[k]).abs().max()) > 0


def test_composite_grad_bg_feeds_the_bg_backward(dev):
    """C = 3: bg = net(dirs) on the GPU -> composite forward -> composite backward -> its grad_bg buffer straight into
    lnerf_bg_backward; the four parameter gradients against float64 autograd of the composed expression."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    C, T_thresh = 3, 1e-4
    _relu_ok(C)
    case = composite_case("benign", C, True, T_thresh)
    inp = case["inp"]
    N, M = inp["N"], inp["M"]
    p = R.bg_params(C)
    dirs = R.bg_directions(N + 200)[200:].contiguous()                                # by ray id
    # float64: the composed expression
    p64 = {k: v.double().requires_grad_() for k, v in p.items()}
    ref = composite_reference(inp["sigmas"].double(), inp["rgbs"].double(), inp["deltas"].double(), inp["rays"], T_thresh,
                              O.bg_mlp(dirs.double(), p64))
    assert ref["margin"] > 1e-3
    sel = ("image", "weights_sum", "depth")
    di = inp["grads"]["image"][:N].double()
    want = dict(zip(KEYS, torch.autograd.grad(ref["image"], [p64[k] for k in KEYS], di)))   # only image depends on the net
    dout64 = (1.0 - ref["weights_sum"].detach())[:, None] * di
    _, S = R.bg_backward_ref(dirs, p, dout64)
    _, S_err = R.bg_backward_ref(dirs, p, COMPOSITE_TOL(ref["count"].double())[:, None] * di.abs())
    # the GPU chain
    pd = {k: v.to(dev) for k, v in p.items()}
    dd = dirs.to(dev)
    bg = _gpu_forward(dev, dd, pd, C, N)
    d = {k: inp[k].to(dev).contiguous() for k in ("sigmas", "rgbs", "deltas", "rays")}
    ws, depth, image = torch.empty(N, device=dev), torch.empty(N, device=dev), torch.empty(N, C, device=dev)
    B.call("lnerf_composite_rays_train_forward", _p(d["sigmas"]), _p(d["rgbs"]), _p(d["deltas"]), _p(d["rays"]), N, C,
           T_thresh, _p(bg), _p(ws), _p(depth), _p(image), _stream())
    g = {k: inp["grads"][k][:N].to(dev).contiguous() for k in sel}
    ds, drgb, dbg = torch.empty(M, device=dev), torch.empty(M, C, device=dev), torch.empty(N, C, device=dev)
    B.call("lnerf_composite_rays_train_backward", _p(g["weights_sum"]), _p(g["depth"]), _p(g["image"]), _p(d["sigmas"]),
           _p(d["rgbs"]), _p(d["deltas"]), _p(d["rays"]), _p(ws), _p(depth), _p(image), _p(bg), N, C, T_thresh, _p(ds),
           _p(drgb), _p(dbg), _stream())
    got = _gpu_backward(dev, dd, N, pd, C, dbg, {k: torch.zeros_like(pd[k]) for k in KEYS})
    tiles = (N + 63) // 64
    worst = _ratios(got, want, {k: R.ULP * (111 + 64 + tiles) * S[k] + S_err[k] for k in KEYS})
    print("composite grad_bg -> bg backward: error / tolerance %s" % {a: "%.3f" % b for a, b in worst.items()})
    for k, r in worst.items():
        assert r <= 1.0, (k, r)
