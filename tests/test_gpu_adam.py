"""The Adam kernels (csrc/optim.hip: k_adam, k_adam_multi) and lnerf_cast_f32_to_bf16, element by element.

Every parameter update of the project goes through `adam_one` (csrc/adam_shared.h); the scatter's fused table update
and the step tail are held bit for bit to lnerf_adam_step elsewhere, so what holds lnerf_adam_step to Adam holds all of
them.  Here every launch is compared with tests/adam_reference.py `adam_ref` -- float64 Adam on the inputs the launch
read -- inside the per-element bounds of `adam_bounds` (a count of the kernel's roundings, with two stated allowances:
a subnormal vhat, and powf in the device step counter's bias corrections).  The only comparisons between two kernel
outputs are the project's own bit-for-bit claims: bf16 gradients == the same values as f32, the multi-tensor launch ==
lnerf_adam_step, the bf16 shadow == the rounding of the launch's own p'.

Every buffer is 64 elements longer than n with a sentinel bit pattern behind it that must survive.  Inputs
(adam_inputs): gradients from 1e-30 to 1e4, exact and signed zeros, warm moments, rows that only decay, subnormal v.
Run with `-s` to see the worst err / bound of every case.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import adam_reference as A

pytestmark = pytest.mark.gpu

PAD = 64
SENT32 = 0x7FC5A5A5      # a NaN as f32, an unlikely integer as int32
SENT16 = 0x7FA5          # a NaN as bf16
LR = 1e-2                # the table's learning rate in the benched configuration
MID = 4097               # the size that runs every step of A.STEPS
SIZES = (1, 3, 4, 5, 1023, MID, 2098179)   # 2 098 179 = 2048 blocks x 256 lanes x 4 + 1027: the grid wraps, n % 4 = 3
TICK = 2                 # LNERF_ADAM_TICK


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    return torch.device("cuda:0")


def _ivw(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _padded(x, dev):
    """x (CPU, f32 / bf16 / int32) at the head of a device buffer PAD elements longer, the sentinel behind it."""
    n = x.numel()
    buf = torch.empty(n + PAD, dtype=x.dtype, device=dev)
    _ivw(buf)[n:] = SENT32 if x.element_size() == 4 else SENT16
    buf[:n] = x.to(dev)
    return buf


def _sentinel_intact(buf, n, what):
    tail = _ivw(buf)[n:].cpu()
    assert tail.numel() == PAD and bool((tail == (SENT32 if buf.element_size() == 4 else SENT16)).all()), \
        "%s: written past n = %d" % (what, n)


def _same_bits(a, b):
    return torch.equal(_ivw(a.contiguous()).cpu(), _ivw(b.contiguous()).cpu())


@functools.lru_cache(maxsize=8)
def _inputs(n, warm, bf16, seed=0):
    """adam_inputs, shared by every case that reads them (never modified: launches work on device copies)."""
    p, g, m, v = A.adam_inputs(n, seed, warm)
    if bf16:
        g = g.to(torch.bfloat16)
    return p, g, m, v


def _expect(n, warm, bf16, t, gs, device_step, seed=0, lr=LR):
    return A.adam_expect(*_inputs(n, warm, bf16, seed), t, lr, grad_scale=gs, device_step=device_step)


def _half_ulp(x):
    """Half the spacing of f32 at x (float64 tensor): the most a correctly rounded f32 result x is from its exact value."""
    return torch.from_numpy(np.spacing(np.abs(x.numpy())).astype(np.float64) * 0.5)


def _check(kp, km, kv, p0, exp, what, worst):
    """Kernel p', m', v' (CPU f32) against the reference: m', v', p' - p and p', each inside its bound."""
    p1, m1, v1, upd, e_m, e_v, e_upd, e_p = exp
    if kp.numel() == 0:
        return
    # p' - p as the buffers hold it: the update's own error plus the one rounding of the stored p', which is at most half
    # the spacing of f32 at the stored value (tighter than the u |p'| inside E_p by up to a factor of two)
    dp = kp.double() - p0.double()
    r = {"m": A.worst_ratio(km, m1, e_m), "v": A.worst_ratio(kv, v1, e_v),
         "dp": A.worst_ratio(dp, -upd, e_upd + _half_ulp(kp)), "p": A.worst_ratio(kp, p1, e_p)}
    for k, x in r.items():
        worst[k] = max(worst.get(k, 0.0), x) if x == x else float("nan")
    for k, x in r.items():
        assert x <= 1.0, "%s: %s is %.3f of its bound" % (what, k, x)


def _launch_step(dev, inp, gdt, t, src, gs, shadow_on, zero, lr=LR):
    """One lnerf_adam_step on device copies of inp.  Returns the padded device buffers P, G, M, V, S (or None)."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    p0, g0, m0, v0 = inp
    n = p0.numel()
    P, G, M, V = (_padded(x, dev) for x in (p0, g0, m0, v0))
    S = _padded(torch.zeros(n, dtype=torch.bfloat16), dev) if shadow_on else None
    if S is not None:
        _ivw(S)[:] = SENT16
    sd = torch.tensor([t, 0], dtype=torch.int32, device=dev) if src == "dev" else None
    # (with the counter the host step is ignored: 0 would be refused without one)
    B.call("lnerf_adam_step", _p(P), _p(G), gdt, _p(M), _p(V), _p(S), n, lr, A.BETA1, A.BETA2, A.EPS,
           0 if src == "dev" else t, _p(sd), gs, zero, _stream())
    torch.cuda.synchronize()
    if sd is not None:
        assert sd.cpu().tolist() == [t, 0], "lnerf_adam_step moved the step counter"
    return P, G, M, V, S


# ------------------------------------------------------------------------------ lnerf_adam_step
@pytest.mark.parametrize("gs", A.GRAD_SCALES, ids=["s1", "s1_8", "s1_3"])
@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("gname", ["f32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_adam_step_against_float64(dev, n, gname, src, gs):
    """lnerf_adam_step == float64 Adam inside the derived bounds, at every size class of k_adam (n < 4: tail only; n % 4
    tails; one block; several; the wrapped grid), f32 and bf16 gradients, host step and device step counter, t from 1 to
    20000 (all of them at n = 4097, t = 1 and 100 elsewhere), from zero moments (t = 1) and from warm ones."""
    from src.latent_nerf.raymarching import backend as B
    bf16 = gname == "bf16"
    gdt = B.BF16 if bf16 else B.F32
    worst, ulp = {}, 0.0
    for t in (A.STEPS if n == MID else (1, 100)):
        for warm in ((False, True) if t == 1 else (True,)):
            inp = _inputs(n, warm, bf16)
            p0, g0, m0, v0 = inp
            exp = _expect(n, warm, bf16, t, gs, src == "dev")
            what = "n=%d %s %s t=%d warm=%d s=%.3f" % (n, gname, src, t, warm, gs)
            outs = []
            for shadow_on, zero in ((True, 1), (False, 0)):
                P, G, M, V, S = _launch_step(dev, inp, gdt, t, src, gs, shadow_on, zero)
                for buf, name in ((P, "p"), (G, "g"), (M, "m"), (V, "v")) + (((S, "shadow"),) if shadow_on else ()):
                    _sentinel_intact(buf, n, what + " " + name)
                kp, km, kv = P[:n].cpu(), M[:n].cpu(), V[:n].cpu()
                _check(kp, km, kv, p0, exp, what, worst)
                if shadow_on:   # the shadow is the rounding of the launch's own p', vector body and tail alike
                    assert _same_bits(S[:n], kp.to(torch.bfloat16)), what + ": shadow != bf16(p')"
                if zero:
                    assert bool((_ivw(G)[:n] == 0).all()), what + ": zero_grad = 1 left something"
                else:
                    assert _same_bits(G[:n], g0), what + ": zero_grad = 0 changed the gradient"
                outs.append((kp, km, kv))
            # with or without shadow / clearing: the same numbers
            assert all(_same_bits(a, b) for a, b in zip(*outs)), what + ": shadow / zero_grad changed the update"
            if bf16:   # the project's claim: bf16 gradients == the same values widened to f32, bit for bit
                P, G, M, V, _ = _launch_step(dev, (p0, g0.float(), m0, v0), B.F32, t, src, gs, False, 1)
                assert _same_bits(P[:n], outs[0][0]) and _same_bits(M[:n], outs[0][1]) and _same_bits(V[:n], outs[0][2]), \
                    what + ": bf16 gradients != the same gradients as f32"
            if n <= MID:
                # p = 0: p' = -update exactly (no final rounding), so the update term itself is measured, in units of
                # u = 2^-24 of the reference update, where vhat is normal and m' does not cancel
                P, _, _, _, _ = _launch_step(dev, (torch.zeros_like(p0), g0, m0, v0), gdt, t, src, gs, False, 0)
                p1, m1, v1, upd, e_m, e_v, e_upd, e_p = exp
                ku = -P[:n].cpu().double()
                r = A.worst_ratio(ku, upd, e_upd)
                worst["upd"] = max(worst.get("upd", 0.0), r)
                assert r <= 1.0, "%s: update term is %.3f of its bound" % (what, r)
                s32 = A.f32(gs)
                b1 = A.f32(A.BETA1)
                parts = (b1 * m0.double()).abs() + ((1.0 - b1) * g0.double() * s32).abs()
                vhat = v1 / A.bias_correction(A.f32(A.BETA2), t)
                normal = vhat >= A.F32_MIN_NORMAL
                if bool(normal.any()):   # (the rest is within the subnormal allowance, which a flushing sqrt uses up)
                    worst["upd, normal vhat"] = max(worst.get("upd, normal vhat", 0.0),
                                                    A.worst_ratio(ku[normal], upd[normal], e_upd[normal]))
                sel = normal & (m1.abs() >= 0.5 * parts) & (upd != 0)
                if bool(sel.any()):
                    ulp = max(ulp, float(((ku - upd).abs() / (A.U * upd.abs()))[sel].max()))
    print("\nadam_step n=%d %s %s s=%.3f: worst err / bound  %s;  update term (normal vhat, no cancellation) %.2f u"
          % (n, gname, src, gs, "  ".join("%s %.3f" % kv for kv in sorted(worst.items())), ulp))


# ------------------------------------------------------------------------------ lnerf_adam_step_multi(_shadow)
MULTI_SIZES = {1: (40001,),
               6: (0, 1, 5, 64, 16385, 2496),
               16: (0, 1, 5, 64, 2496, 2048, 16385, 40001, 5, 0, 64, 1, 2048, 2496, 3, 16385)}


def _multi_lrs(count):
    return [1e-3 * (1.0 + 0.37 * k) for k in range(count)]     # a distinct lr per tensor


def _multi_inputs(count, warm):
    return [_inputs_small(n, warm, 100 + k) for k, n in enumerate(MULTI_SIZES[count])]


@functools.lru_cache(maxsize=64)
def _inputs_small(n, warm, seed):
    return A.adam_inputs(n, seed, warm)


def _launch_multi(dev, bufs, ns, lrs, step, sd, gs, flags, maps=None, shadow=None, shadow_entry=True):
    """One multi-tensor launch over the padded device buffers bufs[k] = [P, G, M, V]."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    c = len(bufs)
    arr = [(ctypes.c_void_p * c)(*[b[j].data_ptr() for b in bufs]) for j in range(4)]
    n_arr = (ctypes.c_int64 * c)(*ns)
    lr_arr = (ctypes.c_float * c)(*lrs)
    if shadow_entry:
        mp = None if maps is None else (ctypes.c_void_p * c)(*[None if x is None else x.data_ptr() for x in maps])
        B.call("lnerf_adam_step_multi_shadow", c, *arr, n_arr, lr_arr, A.BETA1, A.BETA2, A.EPS, step, _p(sd), gs, flags,
               mp, _p(shadow), _stream())
    else:
        B.call("lnerf_adam_step_multi", c, *arr, n_arr, lr_arr, A.BETA1, A.BETA2, A.EPS, step, _p(sd), gs, flags,
               _stream())
    torch.cuda.synchronize()


def _device_copies(dev, inputs):
    return [[_padded(x, dev) for x in inp] for inp in inputs]


@pytest.mark.parametrize("src", ["host", "dev"])
@pytest.mark.parametrize("count", [1, 6, 16])
def test_adam_multi_against_float64(dev, count, src):
    """k_adam_multi: 1, 6 and 16 tensors of 0 .. 40 001 elements (above 64 x 256 the grid wraps), a distinct lr each,
    inside the same bounds per tensor; with the host step, bit for bit what lnerf_adam_step gives for each tensor.  Without
    LNERF_ADAM_TICK the device counter keeps its bits."""
    from src.latent_nerf.raymarching import backend as B
    ns, lrs, gs = MULTI_SIZES[count], _multi_lrs(count), 1.0 / 3.0
    worst = {}
    for t, warm in ((1, False), (100, True)):
        inputs = _multi_inputs(count, warm)
        bufs = _device_copies(dev, inputs)
        sd = torch.tensor([t, 0], dtype=torch.int32, device=dev) if src == "dev" else None
        _launch_multi(dev, bufs, ns, lrs, 0 if src == "dev" else t, sd, gs, 1, shadow_entry=(count != 6))
        if sd is not None:
            assert sd.cpu().tolist() == [t, 0]
        for k, (n, inp, (P, G, M, V)) in enumerate(zip(ns, inputs, bufs)):
            what = "multi count=%d %s t=%d tensor %d (n=%d)" % (count, src, t, k, n)
            for buf, name in ((P, "p"), (G, "g"), (M, "m"), (V, "v")):
                _sentinel_intact(buf, n, what + " " + name)
            assert bool((_ivw(G)[:n] == 0).all()), what + ": gradient not cleared"
            exp = A.adam_expect(*inp, t, lrs[k], grad_scale=gs, device_step=(src == "dev"))
            _check(P[:n].cpu(), M[:n].cpu(), V[:n].cpu(), inp[0], exp, what, worst)
            if src == "host" and n > 0:
                Ps, _, Ms, Vs, _ = _launch_step(dev, inp, B.F32, t, "host", gs, False, 1, lr=lrs[k])
                assert _same_bits(Ps[:n], P[:n]) and _same_bits(Ms[:n], M[:n]) and _same_bits(Vs[:n], V[:n]), \
                    what + ": != lnerf_adam_step"
    print("\nadam_multi count=%d %s: worst err / bound  %s" % (count, src, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize("t0", [1, 98])
def test_adam_multi_tick_counts_and_each_launch_is_its_own_step(dev, t0):
    """LNERF_ADAM_TICK over 16 x 64 workgroups: five launches in a row from step_dev = [t, 0] leave [t + 5, 0], and every
    launch is float64 Adam at ITS t from the state read back before it (a workgroup that read the counter after the tick
    would be one step ahead: at t = 1 that is a factor 1.9 in the update)."""
    count = 16
    ns, lrs, gs = MULTI_SIZES[count], _multi_lrs(count), 1.0 / 8.0
    inputs = _multi_inputs(count, True)
    bufs = _device_copies(dev, inputs)
    sd = torch.tensor([t0, 0], dtype=torch.int32, device=dev)
    worst = {}
    state = [tuple(x.clone() for x in inp) for inp in inputs]           # (p, g, m, v) on the CPU, as launch j reads them
    for j in range(5):
        for (P, G, M, V), st in zip(bufs, state):
            G[:st[1].numel()] = st[1].to(dev)                             # the previous launch cleared it
        _launch_multi(dev, bufs, ns, lrs, 0, sd, gs, 1 | TICK)
        assert sd.cpu().tolist() == [t0 + j + 1, 0], "after launch %d" % j
        for k, (n, (P, G, M, V)) in enumerate(zip(ns, bufs)):
            what = "tick t0=%d launch %d tensor %d (n=%d)" % (t0, j, k, n)
            p0, g0, m0, v0 = state[k]
            exp = A.adam_expect(p0, g0, m0, v0, t0 + j, lrs[k], grad_scale=gs, device_step=True)
            kp, km, kv = P[:n].cpu(), M[:n].cpu(), V[:n].cpu()
            _check(kp, km, kv, p0, exp, what, worst)
            for buf, name in ((P, "p"), (G, "g"), (M, "m"), (V, "v")):
                _sentinel_intact(buf, n, what + " " + name)
            state[k] = (kp, g0, km, kv)
    print("\nadam_multi tick t0=%d: worst err / bound  %s" % (t0, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_adam_multi_mirrors_through_the_maps(dev):
    """lnerf_adam_step_multi_shadow's maps: two int32 positions per element -- both set, one of them -1, or both -1.
    Mapped positions of the bf16 image hold bf16(p') of the launch's own p'; every other position keeps the sentinel, a
    tensor with a null map is not mirrored, and the parameters are inside the bounds as without maps."""
    ns = (5, 64, 2496, 16385, 1, 0)
    lrs, gs, t = _multi_lrs(len(ns)), 1.0, 3
    inputs = [_inputs_small(n, True, 200 + k) for k, n in enumerate(ns)]
    bufs = _device_copies(dev, inputs)
    image = 2 * sum(ns) + 1000                                         # more positions than are ever mapped
    rng = np.random.default_rng(5)
    free = rng.permutation(image)
    maps_cpu, at = [], 0
    for k, n in enumerate(ns):
        if k == 1:                                                     # null map: this tensor is stepped but not mirrored
            maps_cpu.append(None)
            continue
        mp = np.full((n, 2), -1, np.int32)
        for i in range(n):
            kind = i % 4
            if kind == 0:
                mp[i] = free[at:at + 2]; at += 2
            elif kind == 1:
                mp[i, 0] = free[at]; at += 1
            elif kind == 2:
                mp[i, 1] = free[at]; at += 1
        maps_cpu.append(mp)
    maps = [None if mp is None else _padded(torch.from_numpy(mp.reshape(-1)), dev) for mp in maps_cpu]
    S = torch.empty(image + PAD, dtype=torch.bfloat16, device=dev)
    _ivw(S)[:] = SENT16
    _launch_multi(dev, bufs, ns, lrs, t, None, gs, 1, maps=maps, shadow=S)
    want = np.full(image + PAD, SENT16, np.int16)
    worst = {}
    for k, (n, inp, (P, G, M, V)) in enumerate(zip(ns, inputs, bufs)):
        what = "maps tensor %d (n=%d)" % (k, n)
        exp = A.adam_expect(*inp, t, lrs[k], grad_scale=gs)
        _check(P[:n].cpu(), M[:n].cpu(), V[:n].cpu(), inp[0], exp, what, worst)
        for buf, name in ((P, "p"), (G, "g"), (M, "m"), (V, "v")):
            _sentinel_intact(buf, n, what + " " + name)
        if maps_cpu[k] is None or n == 0:
            continue
        h = _ivw(P[:n].cpu().to(torch.bfloat16)).numpy()
        for col in (0, 1):
            on = maps_cpu[k][:, col] >= 0
            want[maps_cpu[k][on, col]] = h[on]
    got = _ivw(S).cpu().numpy()
    assert at > 0 and int((want != SENT16).sum()) == at                # (p' is never NaN, so never the sentinel)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "bf16 image differs at %d positions, first %s" % (bad.size, bad[:8])
    print("\nadam_multi maps: worst err / bound  %s" % "  ".join("%s %.3f" % kv for kv in sorted(worst.items())))


# ------------------------------------------------------------------------------ lnerf_cast_f32_to_bf16
def _cast_inputs(n):
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)         # every class of f32, NaNs included
    special = np.array([
        0x3F808000, 0x3F818000,            # ties: to even downwards (-> 0x3F80), upwards (-> 0x3F82)
        0xBF808000, 0xBF818000,            # the same, negative
        0x3F808001, 0x3F807FFF,            # just above / below a tie
        0x7F7FFFFF, 0xFF7FFFFF,            # largest finite: rounds to +-inf
        0x7F7F7FFF, 0x7F7F8000,            # largest that stays finite; the tie that rounds to inf
        0x00000001, 0x007FFFFF, 0x80000001, 0x00008000, 0x00018000, 0x007F8000,   # subnormals (ties among them)
        0x00000000, 0x80000000, 0x7F800000, 0xFF800000,                           # +-0, +-inf
        0x7FC00000, 0x7F800001, 0xFFFFFFFF, 0x7F80FFFF,                           # NaNs, one with payload below bit 16 only
    ], dtype=np.uint32)
    k = min(n, special.size)
    # at the head, and again so that they end in the last elements (the scalar tail)
    bits[:k] = special[:k]
    if n > k:
        bits[n - k:] = special[:k][::-1]
    return torch.from_numpy(bits.view(np.float32).copy())


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027, 2098179])
def test_cast_f32_to_bf16_is_round_to_nearest_even(dev, n):
    """lnerf_cast_f32_to_bf16 == tensor.to(torch.bfloat16) bit for bit (NaNs: NaN for NaN) on random bit patterns, ties
    in both directions, the overflow to inf, subnormals, zeros and infinities -- vector body, tail and the wrapped grid;
    nothing written past n."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    src_cpu = _cast_inputs(n)
    src = _padded(src_cpu, dev)
    dst = _padded(torch.zeros(n, dtype=torch.bfloat16), dev)
    _ivw(dst)[:] = SENT16
    B.call("lnerf_cast_f32_to_bf16", _p(src), _p(dst), n, _stream())
    torch.cuda.synchronize()
    _sentinel_intact(dst, n, "cast dst")
    _sentinel_intact(src, n, "cast src")
    assert _same_bits(src[:n], src_cpu)
    got = dst[:n].cpu()
    want = src_cpu.to(torch.bfloat16)                     # (the CPU's rounding: the reference)
    nan = torch.isnan(src_cpu)
    assert torch.equal(torch.isnan(got), nan)
    assert torch.equal(_ivw(got)[~nan], _ivw(want)[~nan])
    if n >= 1027:
        assert int(nan.sum()) > 0 and int((~nan).sum()) > n // 2
