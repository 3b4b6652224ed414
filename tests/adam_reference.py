"""Float64 Adam, the error model of the f32 kernels against it, and the inputs both are tested on.

Nothing here imports the package under test: `adam_ref` is the definition of Adam (Kingma & Ba, with the bias
corrections of torch.optim.Adam), `adam_bounds` says how far a correctly working f32 implementation of
csrc/adam_shared.h `adam_one` may be from it, element by element, and `adam_emulate_f32` is that implementation in numpy
float32 (every operation correctly rounded, the kernel's expression order), which tests/test_adam_reference_cpu.py holds
against the bounds without a GPU.  tests/test_gpu_adam.py holds the kernels against the same bounds.

Sign convention: `update` is what is SUBTRACTED, p' = p - update.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of f32 (round to nearest): |fl(x) - x| <= U |x| for normal results
TINY = 2.0 ** -149      # the smallest f32 subnormal: the most a result in the subnormal range is off by
F32_MIN_NORMAL = 2.0 ** -126
POW_ULP = 16            # accuracy the OpenCL C specification requires of pow(), which the device library is written to

# the optimiser of the trainers: Adam(betas=(0.9, 0.99), eps=1e-15)
BETA1, BETA2, EPS = 0.9, 0.99, 1e-15
STEPS = (1, 2, 3, 10, 100, 1000, 20000)
GRAD_SCALES = (1.0, 1.0 / 8.0, 1.0 / 3.0)


def f32(x):
    """A hyperparameter as the kernel receives it: rounded to f32, widened again."""
    return float(np.float32(x))


def bias_correction(beta, step):
    """1 - beta^step in float64 without the cancellation of the literal form (beta: already an f32 value)."""
    if beta == 0.0:
        return 1.0
    return -math.expm1(step * math.log(beta))


def _hyper(lr, beta1, beta2, eps, grad_scale):
    return f32(lr), f32(beta1), f32(beta2), f32(eps), f32(grad_scale)


def adam_ref(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0):
    """One Adam step in float64.  p, g, m, v: f32 (or bf16, for g) tensors, taken as the exact numbers they hold.
    lr, beta1, beta2, eps, grad_scale are rounded to f32 first, as the C ABI passes them (so 1 - beta is exact, as it is
    in f32: Sterbenz); the bias corrections are the exact 1 - beta^step.  Returns float64 p', m', v', update."""
    lr, b1, b2, eps, s = _hyper(lr, beta1, beta2, eps, grad_scale)
    p, g, m, v = (x.detach().cpu().to(torch.float64) for x in (p, g, m, v))
    gs = g * s
    m1 = b1 * m + (1.0 - b1) * gs
    v1 = b2 * v + (1.0 - b2) * gs * gs
    vhat = v1 / bias_correction(b2, step)
    upd = lr * (m1 / bias_correction(b1, step)) / (vhat.sqrt() + eps)
    return p - upd, m1, v1, upd


def adam_bounds(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0, device_step=False):
    """Per-element bounds E_m, E_v, E_upd, E_p (float64 tensors) on |kernel - adam_ref| for m', v', the update and p'.

    The count of roundings in `adam_one` (u = 2^-24; a result in the subnormal range is off by up to 2^-149 instead):

      gs = g * s                                   1
      m' = fma(b1, m, (1 - b1) * gs)               (1 - b1) exact; the product 1; the fma 1, of the SUM
         => E_m = 3u (|b1 m| + |(1 - b1) g s|) + 2^-149           (2u on the g term, 1u on the sum: 3u of the magnitudes)
      v' = fma(b2, v, (1 - b2) * gs * gs)          gs twice 2; two products 2; the fma 1; all terms positive
         => E_v = 5u v' + 2 * 2^-149                              (the second product and the fma can each be subnormal)
      inv_bc = 1 / bc                              bc rounded to f32 1; the division 1
      mhat = m' * inv_bc1                          1            => 3u on top of m's own error
      vhat = v' * inv_bc2                          5 + 2 + 1 = 8u
      sqrt(vhat)                                   halves 8u to 4u; v_sqrt_f32 1 ulp (as the ISA documents it) => 5u
      ... + eps                                    1            => 6u (both terms positive)
      rcp(...)                                     v_rcp_f32 1 ulp (as the ISA documents it)              => 7u
      lr * mhat                                    1
      (lr * mhat) * rcp                            1
         => 7 + 3 + 1 + 1 = 12u of the update from its own operations; stated as 14u (second-order terms, and room for
            sqrt / rcp results that are 1 ulp rather than 1/2)
         => E_upd = 14u |upd| + lr E_m / (bc1 (sqrt(vhat) + eps)) + 2^-149        (m's error, carried through)
      p' = p - upd                                 1, of the result
         => E_p = E_upd + u |p'|

    Two allowances, each only where it applies:
      * vhat < 2^-126 (subnormal): v_sqrt_f32 may read its input as zero.  sqrt(vhat) < 2^-63 then, and the denominator
        is at least eps, so the update changes by at most |upd| 2^-63 / eps.
      * device_step (bias corrections from the device step counter, 1 - powf(beta, t)): powf may be off by P = 16 ulp of
        beta^t, i.e. 2 P u beta^t (an ulp is up to 2u of the value) absolutely, which is 2 P u beta^t / (1 - beta^t) of
        the bias correction; bc1 enters the update linearly, bc2 under the square root (half).  Zero at t = 1:
        powf(beta, 1) is beta.
    """
    return adam_expect(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale, device_step)[4:]


def adam_expect(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0, device_step=False):
    """adam_ref and adam_bounds in one pass: p', m', v', update, E_m, E_v, E_upd, E_p."""
    lr_, b1, b2, eps_, s = _hyper(lr, beta1, beta2, eps, grad_scale)
    p1, m1, v1, upd = adam_ref(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale)
    g64, m64 = (x.detach().cpu().to(torch.float64) for x in (g, m))
    bc1, bc2 = bias_correction(b1, step), bias_correction(b2, step)
    vhat = v1 / bc2
    e_m = 3.0 * U * ((b1 * m64).abs() + ((1.0 - b1) * g64 * s).abs()) + TINY
    e_v = 5.0 * U * v1 + 2.0 * TINY
    e_upd = 14.0 * U * upd.abs() + lr_ * e_m / (bc1 * (vhat.sqrt() + eps_)) + TINY
    e_upd = e_upd + torch.where(vhat < F32_MIN_NORMAL, upd.abs() * (2.0 ** -63 / eps_), torch.zeros_like(upd))
    if device_step and step != 1:
        pw1, pw2 = 1.0 - bc1, 1.0 - bc2
        e_upd = e_upd + upd.abs() * (POW_ULP * 2.0 * U * (pw1 / bc1 + 0.5 * pw2 / bc2))
    e_p = e_upd + U * p1.abs()
    return p1, m1, v1, upd, e_m, e_v, e_upd, e_p


def adam_emulate_f32(p, g, m, v, step, lr, beta1=BETA1, beta2=BETA2, eps=EPS, grad_scale=1.0, device_step=False,
                     sqrt_flush=False):
    """`adam_one` in numpy float32: the kernel's operations in the kernel's order, each correctly rounded (the library is
    built with -ffp-contract=off: the source order is the instruction order).  device_step: bias corrections as
    adam_bias_at forms them (1 - powf(beta, t) in f32, powf correctly rounded) instead of the host's double pow.
    sqrt_flush: the square root reads a subnormal input as zero.  Returns f32 arrays p', m', v'."""
    F = np.float32
    lr, b1, b2, eps, s = (F(x) for x in (lr, beta1, beta2, eps, grad_scale))
    p, g, m, v = (x.detach().cpu().to(torch.float32).numpy() for x in (p, g, m, v))
    if device_step:
        bc1 = F(1) - F(np.float64(b1) ** np.float64(step))
        bc2 = F(1) - F(np.float64(b2) ** np.float64(step))
    else:
        bc1 = F(1.0 - np.float64(b1) ** np.float64(step))
        bc2 = F(1.0 - np.float64(b2) ** np.float64(step))
    inv1, inv2 = F(1) / bc1, F(1) / bc2

    def fma(a, x, y):   # (the double product of two f32 is exact; the one double rounding of the sum is 2^-29 u)
        return (np.float64(a) * x.astype(np.float64) + y.astype(np.float64)).astype(F)

    with np.errstate(under="ignore", over="ignore"):
        gs = g * s
        m1 = fma(b1, m, (F(1) - b1) * gs)
        v1 = fma(b2, v, (F(1) - b2) * gs * gs)
        mhat = m1 * inv1
        vhat = v1 * inv2
        if sqrt_flush:
            vhat = np.where(vhat < F(F32_MIN_NORMAL), F(0), vhat)
        p1 = p - (lr * mhat) * (F(1) / (np.sqrt(vhat) + eps))
    return p1, m1, v1


def adam_inputs(n, seed, warm):
    """p, g, m, v (f32 CPU tensors of n elements) spanning what the kernels meet and what no O(1) gradient shows:
    g log-uniform in 1e-30 .. 1e4 with random sign; warm: m and v drawn the same way (v positive), else zero.  p uniform
    in +-1e-4 (the table's initial range).  Planted by index, (7 i + seed) mod 32, so that every n >= 1 and every tail gets
    some of them:
      0, 1   g = +0, -0
      2      |g| in 1e-30 .. 3e-20: |g s| < 1e-19, vhat subnormal at step 1 from zero moments
      3      warm: g = 0 with m != 0, v != 0 (a row that decays)
      4      warm: v subnormal, m = 0; g = 0 (even i) or tiny as in 2 (odd i)
      5      |p| ~ 1
      6      warm: g = 0, v around the subnormal threshold (1e-45 .. 1e-37) with |m| in 1e-25 .. 1e-19
    """
    rng = np.random.default_rng(1000003 * seed + n)
    F = np.float32

    def logu(lo, hi, size):
        return (10.0 ** rng.uniform(lo, hi, size)).astype(F)

    def sign(size):
        return rng.choice(np.array([-1.0, 1.0], dtype=F), size)

    i = np.arange(n)
    kind = (7 * i + seed) % 32
    p = rng.uniform(-1e-4, 1e-4, n).astype(F)
    g = sign(n) * logu(-30, 4, n)
    tiny = sign(n) * logu(-30, -19.5, n)
    g = np.where(kind == 0, F(0.0), g)
    g = np.where(kind == 1, F(-0.0), g)
    g = np.where(kind == 2, tiny, g)
    p = np.where(kind == 5, sign(n) * rng.uniform(0.5, 1.5, n).astype(F), p)
    if warm:
        m = sign(n) * logu(-30, 4, n)
        v = logu(-30, 4, n)
        g = np.where((kind == 3) | (kind == 6), F(0.0), g)
        sub = rng.integers(1, 0x800000, n, dtype=np.int64).astype(np.uint32).view(F)   # every subnormal bit pattern
        m = np.where(kind == 4, F(0.0), m)
        v = np.where(kind == 4, sub, v)
        g = np.where(kind == 4, np.where(i % 2 == 0, F(0.0), tiny), g)
        m = np.where(kind == 6, sign(n) * logu(-25, -19, n), m)
        v = np.where(kind == 6, (10.0 ** rng.uniform(-45, -37, n)).astype(F), v)
    else:
        m = np.zeros(n, F)
        v = np.zeros(n, F)
    return tuple(torch.from_numpy(np.ascontiguousarray(x.astype(F))) for x in (p, g, m, v))


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (got: any float tensor or array; ref, bound: float64 tensors)."""
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got
    if ref.numel() == 0:
        return 0.0
    err = (got.detach().cpu().to(torch.float64) - ref).abs()
    return float((err / bound).max())
