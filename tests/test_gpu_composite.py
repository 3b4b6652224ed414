"""lnerf_composite_rays_train_forward / _backward (csrc/composite.hip, C = 3 and C = 4) against the float64 compositor of
tests/composite_reference.py, through the C entry points with caller-allocated, poisoned, over-long buffers, on the
cases of composite_reference.composite_inputs (tests/test_composite_reference_cpu.py asserts, without a GPU, that every
case keeps each reference T 1e-3 away from T_thresh, stops where intended and is finite).

Tolerances.  COMPOSITE_TOL(k) = 32 * 2^-24 (k + 1), the compositing bound of tests/test_gpu_inference.py: a weight
w_i = alpha_i T_i carries the rounding of alpha (a few ulp of 1, absolute: 1 - expf(-tau)), of expf, and of the prefix
sum in front of sample i (i + 1 roundings of at most 2^-24 excl each; a kept sample has excl <= ln(1 / T_thresh) <= 9.3),
so |w_i - w64_i| <= COMPOSITE_TOL(i + 1) T64_i, and a ray's k-term sums are within COMPOSITE_TOL(k) of
    weights_sum: 1 (sum_i T_i alpha_i <= 1),   depth: max_k t_k,   image_c: max_k |rgb_kc| + |bg_c|.
None of this grows with the largest sigma dt: the prefix of a sample never passes through the sample's own tau (the
kernel takes it from the neighbouring lane's inclusive sum; with `inc - tau` the error was 2^-24 tau, see below).
Backward: grad_rgbs[s][c] = di_c w_s inherits the weight's bound, |di_c| COMPOSITE_TOL(i + 1) T64_s;  grad_bg_c =
(1 - ws) di_c inherits weights_sum's, COMPOSITE_TOL(k) |di_c|;  grad_sigmas[s] = dt_s (g_s T_{s+1} - (total - pinc_s))
is a difference of sums of g_k w_k with |g_k| <= S_ray = |dws| + |ddp| max t + sum_c |di_c| (max_k |rgb_kc| + |bg_c|),
and `total` is rebuilt from the forward's outputs (image - (1 - ws) bg, whose terms S_ray bounds as well), so it is
within dt_s COMPOSITE_TOL(k) S_ray.  Kill decisions are exact: samples behind the stop get exact zeros.
One term the per-sample scale needs beyond T64: the prefix sum's rounding is relative to excl (delta T / T = delta excl
<= (i + 1) 2^-24 excl), and the constant 32 covers excl <= ln(1e4) = 9.2 only.  With T_thresh > 0 every kept sample
satisfies that; with T_thresh = 0 nothing is dropped and samples deep inside a dense ray have excl in the hundreds, so
there the scale is T64 max(1, excl64 / ln(1e4)) (unchanged wherever excl64 <= ln(1e4)), plus 2^-126 (f32's smallest
normal number) because T64 itself may lie below what f32 holds.

Measured on an MI355X, worst error / tolerance over all cases (each test prints its own; run with -s):
                       benign   one     empty   edge    saturated  large bg
  forward weights_sum  0.008    0.001   0.011   0.002   0.004      0.009
  forward depth        0.007    0.001   0.010   0.001   0.003      0.007
  forward image        0.010    0.000   0.010   0.001   0.001      0.010
  per-sample weight    0.017    0.007   0.008   0.034   0.005      0.061
  grad_sigmas          0.025    0.001   0.021   0.001   0.004      0.015
  grad_rgbs            0.018    0.008   0.008   0.037   0.005      0.062
  grad_bg              0.014    0.001   0.015   0.002   0.004      0.010
(backward rows: the larger of the direct calls and the four selections through the autograd wrapper); the largest
weights_sum is 1 + 5.96e-07 (saturated, k = 77).
What these show for the two forms that are kept as they are: `total - pinc` (grad_sigmas) stays at 0.025 of
dt COMPOSITE_TOL(k) S_ray and below, also behind a saturated sample at T_thresh = 0 where the float64 gradient is exactly
0 and the kernel's is the rounding residue of total - pinc (0.004), and with |bg| up to 100 (0.015); alpha = 1 - expf(-tau)
in empty space (alpha a few ulp of 1, sigma dt <= 3.4e-6) costs 0.008 of the per-sample bound and 0.011 of weights_sum's.
The parent of this change (excl = (inc - tau) + carry) fails all 48 saturated cases and no other.  Its saturated rays
at T_thresh = 1e-4, C = 3, as error / tolerance of (weights_sum, the surface sample's weight); true weight 0.135335 behind
a prefix of optical depth 2.0:
  sigma     position 0    position 20           position 63           position 64
  exp(15)   0, 0          2.0, 23.3             0, 0                  0, 0
  exp(18)   0, 0          32.9, 375             0, 0                  0, 0
  exp(30)   0, 0          13333, 152259         5887, 51534           0, 0         (weight 1.0, weights_sum 1.8647)
  3e38      0, 0          13333, 152259         5887, 51534           0, 0         (weight 1.0, weights_sum 1.8647)
  +inf      37449, 262144 2087, 23831           922, 8066             910, 7944    (weight 0: inf - inf = NaN)
Position 0 has no prefix to lose; at position 64 (lane 0 of the second chunk) inc - tau is exactly 0 and the prefix arrives
through the carry; at position 63 it reaches the lane as three pre-summed pieces (32, 16 and 15 lanes) whose values
happen to be representable next to exp(15) dt and exp(18) dt (an f32 emulation of the scan gives the same zeros).  After
the change every row is at most 0.004.
"""
import math

import pytest
import torch

from tests.composite_reference import CASES, COMPOSITE_TOL, EXTRA, GRAD_SELECTIONS, composite_case

pytestmark = pytest.mark.gpu

POISON = 777.0
TINY = 2.0 ** -126        # f32's smallest normal number: a smaller result may be flushed to zero


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _ratio(err, tol):
    """error / tolerance, elementwise; a zero tolerance admits a zero error only."""
    r = torch.where(tol > 0, err / tol.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err),
                                                                       torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0


def _poisoned(dev, *shape):
    return torch.full(shape, POISON, device=dev, dtype=torch.float32)


def _dev_inputs(dev, inp, with_bg):
    d = {k: inp[k].to(dev).contiguous() for k in ("sigmas", "rgbs", "deltas", "rays")}
    d["bg"] = inp["bg"].to(dev).contiguous() if with_bg else None
    return d


def _forward(dev, inp, d, T_thresh):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    N, C = inp["N"], inp["C"]
    ws, depth, image = _poisoned(dev, N + EXTRA), _poisoned(dev, N + EXTRA), _poisoned(dev, N + EXTRA, C)
    B.call("lnerf_composite_rays_train_forward", _p(d["sigmas"]), _p(d["rgbs"]), _p(d["deltas"]), _p(d["rays"]), N, C,
           float(T_thresh), _p(d["bg"]), _p(ws), _p(depth), _p(image), _stream())
    return ws, depth, image


def _backward(dev, inp, d, T_thresh, fwd, g_ws, g_depth, g_image, want_bg):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    N, M, C = inp["N"], inp["M"], inp["C"]
    ds, drgb = _poisoned(dev, M + EXTRA), _poisoned(dev, M + EXTRA, C)
    dbg = _poisoned(dev, N + EXTRA, C) if want_bg else None
    B.call("lnerf_composite_rays_train_backward", _p(g_ws), _p(g_depth), _p(g_image), _p(d["sigmas"]), _p(d["rgbs"]),
           _p(d["deltas"]), _p(d["rays"]), _p(fwd[0]), _p(fwd[1]), _p(fwd[2]), _p(d["bg"]), N, C, float(T_thresh),
           _p(ds), _p(drgb), _p(dbg), _stream())
    return ds.cpu(), drgb.cpu(), None if dbg is None else dbg.cpu()


def _weight_scale(T):
    """The scale of a sample's weight error: T64, times excl / ln(1e4) where the optical depth in front, excl = -ln T64,
    exceeds ln(1e4) (only possible for T_thresh = 0: the prefix sum's rounding is relative to excl, see the docstring)."""
    excl = -torch.log(T.clamp(min=1e-300))
    return T * (excl / math.log(1e4)).clamp(min=1.0)


def _sample_k(ref):
    """count of the ray of every in-span sample, [M] (0 outside)."""
    ray = ref["ray"].clamp(min=0)
    return torch.where(ref["in_span"], ref["count"][ray], torch.zeros(1, dtype=torch.int64))


def _backward_ratios(inp, ref, want, with_bg, sel, ds, drgb, dbg):
    """error / tolerance of grad_sigmas, grad_rgbs, grad_bg (rows of the spans / of the N named ids) for the gradients
    `sel` of inp['grads'], plus the exact-zero and (when the buffers are the poisoned ones) untouched-row checks."""
    N, M = inp["N"], inp["M"]
    span, keep, ray = ref["in_span"], ref["keep"], ref["ray"].clamp(min=0)
    g = {k: (inp["grads"][k][:N].double() if k in sel else torch.zeros_like(inp["grads"][k][:N].double()))
         for k in ("image", "weights_sum", "depth")}
    di = g["image"].abs()                                                           # [N,C] by id
    bgabs = inp["bg"][:N].double().abs() if with_bg else torch.zeros_like(di)
    S = g["weights_sum"].abs() + g["depth"].abs() * ref["tmax"] + (di * (ref["rgbmax"] + bgabs)).sum(-1)
    k = ref["count"].double()
    out = {}
    # grad_sigmas
    err = (ds[:M].double() - want["sigmas"]).abs()[span]
    tol = (inp["deltas"][:, 0].double() * COMPOSITE_TOL(_sample_k(ref).double()) * S[ray])[span]
    out["dsigma"] = _ratio(err, tol)
    # grad_rgbs
    err = (drgb[:M].double() - want["rgbs"]).abs()[span]
    tol = (di[ray] * (COMPOSITE_TOL(ref["pos"].double() + 1) * _weight_scale(ref["T"]) + TINY)[:, None])[span]
    out["drgb"] = _ratio(err, tol)
    dead = span & ~keep
    assert bool((ds[:M][dead] == 0).all()) and bool((drgb[:M][dead] == 0).all())
    if dbg is not None:
        err = (dbg[:N].double() - want["bg"]).abs()
        out["dbg"] = _ratio(err, COMPOSITE_TOL(k)[:, None] * di)
    return out


@pytest.mark.parametrize("regime,C,with_bg,T_thresh", CASES)
def test_forward_matches_float64(dev, regime, C, with_bg, T_thresh):
    case = composite_case(regime, C, with_bg, T_thresh)
    inp, ref = case["inp"], case["ref"]
    assert ref["margin"] > 1e-3
    N = inp["N"]
    d = _dev_inputs(dev, inp, with_bg)
    ws, depth, image = [t.cpu() for t in _forward(dev, inp, d, T_thresh)]
    for t in (ws, depth, image):
        assert bool((t[N:] == POISON).all())                                       # ids named by no ray
        assert bool(torch.isfinite(t).all())
    k = ref["count"].double()
    tol = COMPOSITE_TOL(k)
    bgabs = inp["bg"][:N].double().abs() if with_bg else torch.zeros(N, C, dtype=torch.float64)
    worst = {"weights_sum": _ratio((ws[:N].double() - ref["weights_sum"]).abs(), tol),
             "depth": _ratio((depth[:N].double() - ref["depth"]).abs(), tol * ref["tmax"]),
             "image": _ratio((image[:N].double() - ref["image"]).abs(), tol[:, None] * (ref["rgbmax"] + bgabs))}
    print("composite forward %s C=%d bg=%s T_thresh=%g: error / tolerance %s, largest weights_sum - 1 = %.3e"
          % (regime, C, with_bg, T_thresh, {a: "%.3f" % b for a, b in worst.items()}, float(ws[:N].max()) - 1.0))
    # empty spans: exactly 0, 0, bg (before the bound, which is 0 there without a background anyway)
    empty = ref["count"] == 0
    if bool(empty.any()):
        assert bool((ws[:N][empty] == 0).all()) and bool((depth[:N][empty] == 0).all())
        assert torch.equal(image[:N][empty], inp["bg"][:N][empty] if with_bg else torch.zeros(int(empty.sum()), C))
    assert bool((ws[:N].double() <= 1.0 + tol).all()), float(ws[:N].max())
    for key, r in worst.items():
        assert r <= 1.0, (key, r)


@pytest.mark.parametrize("regime,C,with_bg,T_thresh", CASES)
def test_per_sample_weights_match_float64(dev, regime, C, with_bg, T_thresh):
    """grad_image = one channel's unit vector and no other gradient: grad_rgbs[s][c] is w_s itself (1 * w_s), the other
    channels exactly 0.  |w_s - w64_s| <= COMPOSITE_TOL(i + 1) T64_s for sample i of its ray."""
    case = composite_case(regime, C, with_bg, T_thresh)
    inp, ref = case["inp"], case["ref"]
    N, M = inp["N"], inp["M"]
    d = _dev_inputs(dev, inp, with_bg)
    fwd = _forward(dev, inp, d, T_thresh)
    span = ref["in_span"]
    tol = (COMPOSITE_TOL(ref["pos"].double() + 1) * _weight_scale(ref["T"]) + TINY)[span]
    worst = 0.0
    for c in range(C):
        g_image = torch.zeros(N + EXTRA, C, device=dev)
        g_image[:, c] = 1.0
        ds, drgb, _ = _backward(dev, inp, d, T_thresh, fwd, None, None, g_image, False)
        assert bool(torch.isfinite(ds).all()) and bool(torch.isfinite(drgb).all())
        assert bool((drgb[:M][~span] == POISON).all()) and bool((drgb[M:] == POISON).all())
        assert bool((ds[:M][~span] == POISON).all()) and bool((ds[M:] == POISON).all())
        others = [j for j in range(C) if j != c]
        assert bool((drgb[:M][span][:, others] == 0).all())
        w = drgb[:M, c].double()
        assert bool((w[span & ~ref["keep"]] == 0).all())
        worst = max(worst, _ratio((w - ref["w"]).abs()[span], tol))
    print("composite per-sample weights %s C=%d bg=%s T_thresh=%g: worst error / tolerance %.3f"
          % (regime, C, with_bg, T_thresh, worst))
    assert worst <= 1.0, worst


@pytest.mark.parametrize("regime,C,with_bg,T_thresh", CASES)
def test_backward_matches_float64_autograd(dev, regime, C, with_bg, T_thresh):
    """All three gradients given; poisoned over-long buffers; grad_bg = NULL accepted; the same bits on a second call."""
    case = composite_case(regime, C, with_bg, T_thresh)
    inp, ref = case["inp"], case["ref"]
    N, M = inp["N"], inp["M"]
    sel = GRAD_SELECTIONS[0]
    d = _dev_inputs(dev, inp, with_bg)
    fwd = _forward(dev, inp, d, T_thresh)
    g = {k: inp["grads"][k].to(dev).contiguous() for k in sel}
    ds, drgb, dbg = _backward(dev, inp, d, T_thresh, fwd, g["weights_sum"], g["depth"], g["image"], with_bg)
    for t in (ds, drgb) + ((dbg,) if with_bg else ()):
        assert bool(torch.isfinite(t).all())
    span = ref["in_span"]
    assert bool((ds[:M][~span] == POISON).all()) and bool((ds[M:] == POISON).all())
    assert bool((drgb[:M][~span] == POISON).all()) and bool((drgb[M:] == POISON).all())
    if with_bg:
        assert bool((dbg[N:] == POISON).all())
    worst = _backward_ratios(inp, ref, case["ref_grads"][sel], with_bg, sel, ds, drgb, dbg)
    print("composite backward %s C=%d bg=%s T_thresh=%g: error / tolerance %s"
          % (regime, C, with_bg, T_thresh, {a: "%.3f" % b for a, b in worst.items()}))
    ds2, drgb2, dbg2 = _backward(dev, inp, d, T_thresh, fwd, g["weights_sum"], g["depth"], g["image"], with_bg)
    assert torch.equal(ds2, ds) and torch.equal(drgb2, drgb) and (not with_bg or torch.equal(dbg2, dbg))
    ds3, drgb3, dbg3 = _backward(dev, inp, d, T_thresh, fwd, g["weights_sum"], g["depth"], g["image"], False)
    assert dbg3 is None and torch.equal(ds3, ds) and torch.equal(drgb3, drgb)      # grad_bg = NULL
    for key, r in worst.items():
        assert r <= 1.0, (key, r)


@pytest.mark.parametrize("regime,C,with_bg,T_thresh", CASES)
def test_gradient_selections_through_the_autograd_wrapper(dev, regime, C, with_bg, T_thresh):
    """raymarching.composite_rays_train with each selection of GRAD_SELECTIONS (an unused output arrives as None) against
    the float64 autograd of the same selection, same bounds."""
    from src.latent_nerf.raymarching import raymarching as rm
    case = composite_case(regime, C, with_bg, T_thresh)
    inp, ref = case["inp"], case["ref"]
    N = inp["N"]
    worst = {}
    for sel in GRAD_SELECTIONS:
        sg = inp["sigmas"].to(dev).requires_grad_()
        rgb = inp["rgbs"].to(dev).requires_grad_()
        bg = inp["bg"][:N].to(dev).requires_grad_() if with_bg else None
        ws, depth, image = rm.composite_rays_train(sg, rgb, inp["deltas"].to(dev), inp["rays"].to(dev), T_thresh, bg)
        out = {"weights_sum": ws, "depth": depth, "image": image}
        torch.autograd.backward([out[k] for k in sel], [inp["grads"][k][:N].to(dev) for k in sel])
        got = _backward_ratios(inp, ref, case["ref_grads"][sel], with_bg, sel, sg.grad.cpu(), rgb.grad.cpu(),
                               bg.grad.cpu() if with_bg else None)
        for key, r in got.items():
            worst[key] = max(worst.get(key, 0.0), r)
    print("composite selections %s C=%d bg=%s T_thresh=%g: error / tolerance %s"
          % (regime, C, with_bg, T_thresh, {a: "%.3f" % b for a, b in worst.items()}))
    for key, r in worst.items():
        assert r <= 1.0, (key, r)
