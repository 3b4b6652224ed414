"""The float64 Adam reference of tests/adam_reference.py against torch.optim.Adam, and its error model against an f32
emulation of csrc/adam_shared.h `adam_one` -- without a GPU.  tests/test_gpu_adam.py holds the kernels to the same
bounds; the refusal cases of the Adam entry points are in tests/test_abi_cpu.py."""
import pytest
import torch

from tests import adam_reference as A


@pytest.mark.parametrize("grad_scale", A.GRAD_SCALES)
def test_adam_ref_is_torch_adam_in_float64(grad_scale):
    """adam_ref, applied five times, is torch.optim.Adam on float64 tensors (same f32-rounded hyperparameters, gradient
    times grad_scale) to 1e-12 relative: an implementation that shares no line with the reference."""
    n, lr = 4096, 1e-2
    p0, _, _, _ = A.adam_inputs(n, 3, False)
    lr_, b1, b2, eps, s = A._hyper(lr, A.BETA1, A.BETA2, A.EPS, grad_scale)
    ref = p0.double().clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=lr_, betas=(b1, b2), eps=eps)
    p, m, v = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for step in range(1, 6):
        _, g, _, _ = A.adam_inputs(n, 10 + step, False)
        ref.grad = g.double() * s
        opt.step()
        # (float64 in: adam_ref takes the numbers as they are)
        p, m, v, _ = A.adam_ref(p, g, m, v, step, lr, grad_scale=grad_scale)
    st = opt.state[ref]
    torch.testing.assert_close(p, ref.detach(), rtol=1e-12, atol=0.0)
    torch.testing.assert_close(m, st["exp_avg"], rtol=1e-12, atol=0.0)
    torch.testing.assert_close(v, st["exp_avg_sq"], rtol=1e-12, atol=0.0)
    assert float((p - p0.double()).abs().max()) > 1e-3     # (the five steps moved something)


@pytest.mark.parametrize("device_step", [False, True])
@pytest.mark.parametrize("warm", [False, True])
def test_f32_emulation_stays_inside_every_bound(warm, device_step):
    """numpy float32, each operation correctly rounded, the kernel's expression order -- with the square root honouring
    subnormal inputs and reading them as zero: inside E_m, E_v, E_upd (through p' on elements with p = 0) and E_p at
    every step and grad_scale of the GPU test.  The margin printed here is what the bounds leave a kernel whose sqrt and
    rcp are 1 ulp rather than 1/2."""
    n, lr = 65537, 1e-2
    p, g, m, v = A.adam_inputs(n, 7 + warm, warm)
    pz = torch.zeros_like(p)
    worst = {"m": 0.0, "v": 0.0, "upd": 0.0, "p": 0.0}
    for step in A.STEPS:
        for s in A.GRAD_SCALES:
            p1, m1, v1, upd = A.adam_ref(p, g, m, v, step, lr, grad_scale=s)
            e_m, e_v, e_upd, e_p = A.adam_bounds(p, g, m, v, step, lr, grad_scale=s, device_step=device_step)
            for flush in (False, True):
                kp, km, kv = A.adam_emulate_f32(p, g, m, v, step, lr, grad_scale=s, device_step=device_step,
                                                sqrt_flush=flush)
                ku, _, _ = A.adam_emulate_f32(pz, g, m, v, step, lr, grad_scale=s, device_step=device_step,
                                              sqrt_flush=flush)     # p = 0: p' is the update itself, no final rounding
                r = {"m": A.worst_ratio(km, m1, e_m), "v": A.worst_ratio(kv, v1, e_v),
                     "upd": A.worst_ratio(-ku, upd, e_upd), "p": A.worst_ratio(kp, p1, e_p)}
                for k in r:
                    assert r[k] <= 1.0, (k, r[k], step, s, flush)
                    worst[k] = max(worst[k], r[k])
    print("f32 emulation, warm=%d device_step=%d: worst err / bound  m %.3f  v %.3f  upd %.3f  p %.3f"
          % (warm, device_step, worst["m"], worst["v"], worst["upd"], worst["p"]))


def test_adam_inputs_plants_the_edges():
    """What adam_inputs promises is there, at a size as small as the tests use."""
    p, g, m, v = A.adam_inputs(4097, 0, True)
    gz = g == 0
    assert bool((gz & torch.signbit(g)).any()) and bool((gz & ~torch.signbit(g)).any())
    assert bool(((g.abs() < 1e-19) & ~gz).any())
    assert bool((gz & (m != 0) & (v != 0)).any())
    sub = (v > 0) & (v < A.F32_MIN_NORMAL)
    assert bool((sub & (m == 0)).any())
    assert bool((p.abs() > 0.4).any()) and float(p.abs().median()) <= 1e-4
    p, g, m, v = A.adam_inputs(5, 0, False)
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    # vhat subnormal at step 1 from zero moments
    _, _, v1, _ = A.adam_ref(*A.adam_inputs(4097, 0, False), 1, 1e-2)
    vhat = v1 / A.bias_correction(A.f32(A.BETA2), 1)
    assert bool(((vhat > 0) & (vhat < A.F32_MIN_NORMAL)).any())
