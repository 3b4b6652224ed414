"""The coverage-weighted pyramids (csrc/texmip.hip) on the GPU against the float64 references of tests/cov_reference.py.

ULP = 2^-24, the relative error of one f32 operation.  Every bound below is a count of the kernel's roundings times
ULP times the magnitude the reference propagates (the same rule as the value on absolute values).  The branch decisions
of the kernels (s > 0, k == 1, k == 0, every W == 1, D == 0) are functions of the f32 weights alone; the references take
them from the same f32 weights with the same f32 operations (cov_reference._s32), so no texel or pixel is excluded.

* lnerf_mipcov_weights: (wa + wb) + (wc + wd) and an exact * 0.25.  For 0/1 weights every sum is exact: torch.equal to
  the float64 pyramid.  For any weights the same three f32 additions on the CPU give the same bits: torch.equal too.
* lnerf_mipcov_pull: a level is four products (1 rounding each), a sum of depth 2 (2), the sum s (2, relative) and a
  division (1): 6 ULP of sum w |v| / s, plus the children's own errors, which the weighted mean averages along.  Level l
  is within (6 l + 1) ULP of the magnitude (the 1 for the second-order terms).  All ones: lnerf_mip_build's bits.
* lnerf_mipcov_pull_backward: per level q = w / s (s 2, the division 1), the product 1 and the add 1: 5 ULP of the
  folded absolute gradients per level, (5 L + 1) ULP in all.
* lnerf_mipcov_push: up = four products (1), a sum of depth 2 (2) and, where a tap is not reached, a division by an
  exact multiple of 1/16 (1): 4 ULP of up(M).  F = k v + (1 - k) up: (1 - k) 1, two products 1, the add 1: 3 ULP of
  M_l = k |v| + (1 - k) up(M_{l+1}).  With K_L = 6 L + 1 from the pull, K_l = K_{l+1} + 7 (v_l's own 6 l + 1 is below
  K_{l+1}), so level l is within (6 L + 1 + 7 (L - l) + 1) ULP of M_l, level 0 within (13 L + 2) ULP.
* lnerf_texture_mipcov_forward: case (a) and (b) are the plain mode: its bound, (4 + 2) ULP of the absolute tap sums of
  the levels read (tests/test_gpu_mip.py).  Case (c): a term (b W) V has b's 3 roundings, the two products 2, the sum of
  four 3 (<= 7 with the plain mode's tap analysis 4 + 2 plus one for W), the mix (1 - t) 1, a product 1, the add 1: N is
  within 10 ULP of Nabs = sum mix b W |V|, D (all terms >= 0) within 10 ULP of itself; the quotient adds 1:
  |out - N / D| <= (10 Nabs / D + 10 |N| / D + |N| / D) ULP <= 21 ULP Nabs / D, and 22 with the second-order terms.
  The error of lambda (dlam as tests/test_gpu_mip.py: log2f's 1 ulp, the product rho R and the bias add) is NOT a
  Lipschitz term here, because the normalised lookup jumps at an integer lambda where one level's denominator is 0.
  Instead the result must be within its rounding bound of the exact lookup at SOME lambda within dlam of the float64
  one: cov_reference.lambda_pieces cuts [lambda - dlam, lambda + dlam] at the integer it may contain; inside an open
  piece the lookup is a ratio of two functions linear in t, monotone, so its values lie between the piece's two ends.
* lnerf_texture_mipcov_backward + lnerf_mipcov_pull_backward, per texel of level 0 after the fold: an addend
  (b W) ((m g) / D) has b 3, b W 1, m = 1 - t 1, m g 1, D 10 (above), the division 1, the product 1: 18; n atomic adds
  n; the fold 5 per level: (n + 18 + 5 L + 2) ULP of the folded absolute addends (2 for second order).  The error of
  lambda enters as the largest change of the pixel's coefficients over the admissible lambdas, |g| times it, folded;
  the roundings are counted and scaled for the largest admissible coefficients (the reference's plus that change),
  since the kernel's addends are those of its own lambda."""
import pytest
import torch

from tests import cov_reference as V
from tests import mip_reference as M
from tests.test_gpu_mip import _dlam, _rho_cases
from tests.test_gpu_raster_ops import _uv_cases

pytestmark = pytest.mark.gpu

ULP = M.ULP
SIDES = [2, 8, 12, 64]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _levels_for(R):
    full = M.full_levels(R)
    return sorted({full, full // 2})


def _rects(R, gap):
    """Two rectangles `gap` texels apart (clipped to the texture)."""
    w = torch.zeros(R, R)
    a = max(R // 8, 1)
    w[a:R // 2, a:R // 2 - gap // 2] = 1
    w[a:R // 2 + 1, R // 2 - gap // 2 + gap:R - a] = 1
    return w


def patterns(R, g):
    """name -> w0 [R,R] f32: the coverage patterns every test here runs over."""
    k = torch.arange(R)
    one = torch.zeros(R, R)
    one[R // 3, R // 2] = 1
    blocks = torch.ones(R, R)
    for n, (i, j) in enumerate((a, b) for a in range(0, R, 4) for b in range(0, R, 4)):
        if n % 3 == 0:
            blocks[i:i + 4, j:j + 4] = 0                     # a whole empty 4 x 4 block beside full ones
        elif n % 3 == 1:
            blocks[i:i + 2, j:j + 2] = 0                     # whole empty 2 x 2 blocks inside a 4 x 4 block
            blocks[i + 2:i + 4, j + 2:j + 4] = 0
    return {"ones": torch.ones(R, R), "zeros": torch.zeros(R, R), "one": one,
            "checker": ((k[:, None] + k[None, :]) % 2).float(), "rects1": _rects(R, 1), "rects2": _rects(R, 2),
            "rects4": _rects(R, 4), "blocks": blocks, "random": torch.rand(R, R, generator=g)}


EXACT = ("ones", "zeros", "one", "checker")      # 0/1 patterns on which every weighted mean of integers is exact


def _weights(dev, w0, R, L):
    """The GPU's weights of levels 0..L as f32 CPU tensors, and the device tensors."""
    from src.latent_nerf.raymarching import mipcov_weights
    w0_d = w0.to(dev).contiguous()
    wpyr = mipcov_weights(w0_d, L)
    return V.unpack_weights(w0, wpyr.cpu() if L else None, R, L), w0_d, wpyr


@pytest.mark.parametrize("R", SIDES)
def test_weights_are_exact(dev, R):
    g = torch.Generator().manual_seed(R)
    for L in _levels_for(R):
        for name, w0 in patterns(R, g).items():
            wl, _, wpyr = _weights(dev, w0, R, L)
            assert (wpyr is None) == (L == 0)
            if name != "random":
                for got, ref in zip(wl, V.weight_levels(w0, L)):
                    assert torch.equal(got.double(), ref), (name, L)
                    assert float(got.max()) <= 1.0
            for got, ref in zip(wl, V.weight_levels_f32(w0, L)):
                assert torch.equal(got, ref), (name, L)


@pytest.mark.parametrize("R", [2, 12, 64])
def test_weights_are_the_plain_build_of_one_channel(dev, R):
    """lnerf_mipcov_weights runs lnerf_mip_build's kernel on a [1,R,R] texture: the two entry points agree bit for bit."""
    from src.latent_nerf.raymarching import mipcov_weights
    from src.latent_paint.models.render import mip_build
    g = torch.Generator().manual_seed(R + 3)
    for L in _levels_for(R):
        for name, w0 in patterns(R, g).items():
            w0_d = w0.to(dev).contiguous()
            got, want = mipcov_weights(w0_d, L), mip_build(w0_d[None], L)
            if L == 0:
                assert got is None and want is None
            else:
                assert torch.equal(got, want[0]), (name, L)


@pytest.mark.parametrize("R", SIDES)
def test_pull_forward_and_backward(dev, R):
    from src.latent_nerf.raymarching import mipcov_pull, mipcov_pull_backward
    from src.latent_paint.models.render import mip_build
    g = torch.Generator().manual_seed(R + 1)
    worst_f = worst_b = 0.0
    for C in (1, 3, 4):
        for L in _levels_for(R):
            for name, w0 in patterns(R, g).items():
                tex = torch.randn(C, R, R, generator=g)
                ints = torch.randint(-8, 9, (C, R, R), generator=g).float()
                wl, w0_d, wpyr = _weights(dev, w0, R, L)
                if L == 0:
                    assert mipcov_pull(tex.to(dev), w0_d, wpyr, 0) is None
                    continue
                got_d = mipcov_pull(tex.to(dev), w0_d, wpyr, L)
                got = M.unpack(got_d.cpu(), R, L)
                vals, mags = V.pull(tex, wl, L)
                for l in range(1, L + 1):
                    err = (got[l - 1].double() - vals[l]).abs()
                    bound = (6 * l + 1) * ULP * mags[l]
                    worst_f = max(worst_f, float((err / bound.clamp(min=1e-300)).max()))
                    assert bool((err <= bound).all()), (C, L, name, l, worst_f)
                    assert bool((got[l - 1][:, V._s32(wl[l - 1]) == 0] == 0).all())     # nothing covered: exactly 0
                if name == "ones":
                    assert torch.equal(got_d, mip_build(tex.to(dev), L))
                if name in EXACT:
                    exact = M.unpack(mipcov_pull(ints.to(dev), w0_d, wpyr, L).cpu(), R, L)
                    for a, b in zip(exact, V.pull(ints, wl, L)[0][1:]):
                        assert torch.equal(a.double(), b), (C, L, name)
                # the backward folds dpyr into dtex, which it accumulates into
                dtex0 = torch.randn(C, R, R, generator=g)
                dlev = [torch.randn(C, R >> l, R >> l, generator=g) for l in range(1, L + 1)]
                dtex = dtex0.to(dev)
                mipcov_pull_backward(M.pack(dlev).contiguous().to(dev), w0_d, wpyr, dtex, L)
                want = V.pull_transpose([dtex0] + dlev, wl)
                s = V.pull_transpose([dtex0.abs()] + [d.abs() for d in dlev], wl)
                err = (dtex.cpu().double() - want).abs()
                bound = (5 * L + 1) * ULP * s
                worst_b = max(worst_b, float((err / bound.clamp(min=1e-300)).max()))
                assert bool((err <= bound).all()), (C, L, name, worst_b)
                if name == "zeros":
                    assert torch.equal(dtex.cpu(), dtex0)
    print("pull R=%d: max forward err / bound = %.3g, max backward err / bound = %.3g" % (R, worst_f, worst_b))


def test_pull_is_the_adjoint_of_its_backward_on_the_gpu(dev):
    """<pull x, y> = <x, pull^T y> with the GPU's own two kernels, R = 12 (levels of side 6 and 3), to f32 accuracy:
    both sides are sums of C (R^2 + S) products of unit normals, each within (6 L + 1) resp. (5 L + 1) ULP."""
    from src.latent_nerf.raymarching import mipcov_pull, mipcov_pull_backward
    R, L, C = 12, 2, 3
    g = torch.Generator().manual_seed(5)
    w0 = patterns(R, g)["random"]
    _, w0_d, wpyr = _weights(dev, w0, R, L)
    x = torch.randn(C, R, R, generator=g).to(dev)
    y = torch.randn(C, M.level_offsets(R, L)[1], generator=g).to(dev)
    lhs = float((mipcov_pull(x, w0_d, wpyr, L).double() * y.double()).sum())
    fold = mipcov_pull_backward(y.clone(), w0_d, wpyr, torch.zeros_like(x), L)
    rhs = float((x.double() * fold.double()).sum())
    scale = float((mipcov_pull(x.abs(), w0_d, wpyr, L).double() * y.double().abs()).sum())
    assert abs(lhs - rhs) <= (6 * L + 1 + 5 * L + 1) * ULP * scale, (lhs, rhs, scale)


@pytest.mark.parametrize("R", SIDES)
def test_push_fills_from_the_covered_texels(dev, R):
    from src.latent_nerf.raymarching import mipcov_pull, mipcov_push, pull_push_fill
    g = torch.Generator().manual_seed(R + 2)
    worst = 0.0
    for C in (1, 3, 4):
        const = torch.tensor([0.75, -1.5, 3.0, 0.1])[:C]
        for L in _levels_for(R):
            for name, w0 in patterns(R, g).items():
                wl, w0_d, wpyr = _weights(dev, w0, R, L)
                covered = w0 > 0
                noise = torch.randn(C, R, R, generator=g)
                flat = torch.where(covered[None], const.view(C, 1, 1).expand(C, R, R), noise)
                for kind, tex in (("noise", noise), ("const", flat)):
                    tex_d = tex.to(dev).clone()
                    pyr = mipcov_pull(tex_d, w0_d, wpyr, L)
                    out, filled = mipcov_push(tex_d, w0_d, wpyr, pyr, L)
                    assert out.data_ptr() == tex_d.data_ptr() and filled.dtype == torch.uint8
                    out, filled = out.cpu(), filled.cpu().bool()
                    vals, mags = V.pull(tex, wl, L)
                    F, Mg, ref_filled, reached = V.push(tex, wl, vals, mags, L)
                    assert torch.equal(filled, ref_filled), (C, L, name)
                    assert bool(torch.isfinite(out).all())
                    assert torch.equal(out[:, w0 == 1], tex[:, w0 == 1])              # covered: bit for bit
                    assert torch.equal(out[:, ~filled], tex[:, ~filled])              # not written at all
                    K = 13 * L + 2
                    err = (out.double() - F[0]).abs()
                    bound = K * ULP * Mg[0]
                    worst = max(worst, float((err / bound.clamp(min=1e-300)).max()))
                    assert bool((err <= bound).all()), (C, L, name, kind, worst)
                    if L > 0:                                                         # the filled levels on exit
                        for l, lev in enumerate(M.unpack(pyr.cpu(), R, L), start=1):
                            assert bool(((lev.double() - F[l]).abs() <= K * ULP * Mg[l]).all()), (C, L, name, kind, l)
                    if not bool(covered.any()):                  # "zeros", and the rectangles that do not fit in R = 2
                        assert torch.equal(out, tex) and not bool(filled.any())
                        continue
                    if L == M.full_levels(R) and R & (R - 1) == 0 and L > 0:          # one coarsest texel: all reached
                        assert bool(reached.all()) and torch.equal(filled, w0 != 1)
                    # every written value lies between the covered minimum and maximum, give or take the bound
                    lo = torch.where(covered[None], tex, torch.full((), float("inf"))).amin(dim=(1, 2)).double()
                    hi = torch.where(covered[None], tex, torch.full((), -float("inf"))).amax(dim=(1, 2)).double()
                    o = out.double()
                    inside = (o >= lo.view(C, 1, 1) - bound) & (o <= hi.view(C, 1, 1) + bound)
                    assert bool(inside[:, filled].all()), (C, L, name, kind)
                    if kind == "const":                                               # ... so a constant comes back
                        dev_c = (o - const.double().view(C, 1, 1)).abs()
                        assert bool((dev_c <= K * ULP * const.double().abs().view(C, 1, 1))[:, filled | covered].all())
    # the one-call form: a new texture, every level the side allows
    w0 = patterns(64, g)["rects2"]
    tex = torch.randn(3, 64, 64, generator=g).to(dev)
    keep = tex.clone()
    out, filled = pull_push_fill(tex, w0.to(dev))
    assert torch.equal(tex, keep) and out.data_ptr() != tex.data_ptr()
    assert torch.equal(filled.cpu().bool(), w0 != 1) and torch.equal(out[:, w0.to(dev) == 1], tex[:, w0.to(dev) == 1])
    # a side that is no power of two (12: two levels of its own) is padded to one for the fill: a single known texel
    # still fills everything, within the bound of the padded side's four levels
    w0 = patterns(12, g)["one"]
    tex = torch.randn(3, 12, 12, generator=g).to(dev)
    out, filled = pull_push_fill(tex, w0.to(dev))
    value = tex[:, w0.to(dev) == 1]                                                   # [3,1]
    assert out.shape == (3, 12, 12) and torch.equal(filled.cpu().bool(), w0 != 1)
    assert torch.equal(out[:, w0.to(dev) == 1], value)
    assert bool(((out - value[:, :, None]).abs() <= (13 * 4 + 2) * ULP * value.abs()[:, :, None]).all())
    print("push R=%d: max err / bound = %.3g" % (R, worst))


# ------------------------------------------------------------------------------------------------------- lookup
def _between(got, ends):
    """got within the interval spanned by the piece's end values, widened by the larger of their bounds."""
    (v1, b1), (v2, b2) = ends
    b = torch.maximum(b1, b2)
    return (got >= torch.minimum(v1, v2) - b) & (got <= torch.maximum(v1, v2) + b)


@pytest.mark.parametrize("bias", [0.0, 0.75])
@pytest.mark.parametrize("R", SIDES)
def test_lookup_forward_backward(dev, R, bias):
    from src.latent_nerf.raymarching import mipcov_pull
    from src.latent_paint.models.render import mip_lookup, mip_lookup_backward
    g = torch.Generator().manual_seed(R * 13 + int(bias * 4))
    worst_b, seen_b, seen_c = 0.0, 0, 0
    for C, with_idx in ((1, True), (3, False), (3, True), (4, False)):
        uv = _uv_cases(R, 2000, g)
        P = uv.shape[0]
        ar = torch.arange(P)
        for L in _levels_for(R):
            rho = _rho_cases(P, R, L, g)
            for name, w0 in patterns(R, g).items():
                fg = torch.ones(P, dtype=torch.bool)
                face_idx = None
                if with_idx:
                    fg = torch.rand(P, generator=g) > 0.2
                    face_idx = torch.where(fg, torch.randint(0, 9, (P,), generator=g), torch.full((P,), -1)).int().to(dev)
                tex = torch.randn(C, R, R, generator=g)
                wl, w0_d, wpyr = _weights(dev, w0, R, L)
                tex_d, uv_d, rho_d = tex.to(dev), uv.to(dev), rho.to(dev)
                pyr = mipcov_pull(tex_d, w0_d, wpyr, L)
                got_d = mip_lookup(tex_d, pyr, uv_d, rho_d, face_idx, L, bias, w0_d, wpyr)
                got = got_d.cpu().double()
                levels = [tex] + (M.unpack(pyr.cpu(), R, L) if L else [])
                look = V.Lookup(levels, wl, uv)
                lam = M.lod(rho, R, L, bias)
                pts, pieces = V.lambda_pieces(lam, _dlam(lam), L)
                ev = {n: (look.at(l0, t), valid) for n, l0, t, valid in pts}
                ok = torch.zeros(P, C, dtype=torch.bool)
                for first, last in pieces:
                    a, valid = ev[first]
                    b, _ = ev[last]
                    ok |= valid[:, None] & _between(got, ((a["out"], a["bound"]), (b["out"], b["bound"])))
                assert bool(ok[fg].all()), (C, with_idx, L, name, int((~ok[fg]).sum()))
                assert bool((got[~fg] == 0).all())
                # the lookup at the float64 lambda itself: the cases, and the backward's reference
                cell = lam.floor().clamp(max=L).long()
                ref = look.at(cell, lam - cell)
                far = ev["a"][1]                         # no integer within dlam: the case is the float64 lambda's
                sure_b = ref["case_b"] & far & fg
                seen_b += int(sure_b.sum())
                seen_c += int((~ref["case_a"] & ~ref["case_b"] & fg).sum())
                want_plain = mip_lookup(tex_d, pyr, uv_d, rho_d, face_idx, L, bias)
                if name == "ones":                       # case (a) everywhere: the plain mode bit for bit
                    assert bool(ref["case_a"].all()) and torch.equal(got_d, want_plain)
                # case (b): every tap has weight 0 -- the plain mode's value there
                assert torch.equal(got_d.cpu()[sure_b], want_plain.cpu()[sure_b]), (C, L, name)
                # ---- backward: level 0 after the fold, per texel
                dout = torch.randn(P, C, generator=g)
                gotb = mip_lookup_backward(dout.to(dev), (C, R), uv_d, rho_d, face_idx, L, bias, w0_d, wpyr).cpu().double()
                gT = torch.where(fg[None], dout.double().T, torch.zeros(()).double())             # [C,P]
                d, s, n, slack = [], [], [], []
                reach_b = torch.zeros(R * R, dtype=torch.bool)      # level-0 texels a case (b) pixel may add to
                for l in range(L + 1):
                    idx, _ = look.taps[l]
                    side = R >> l
                    ix = idx[None].expand(C, -1, -1).reshape(C, -1)
                    coef = ref["coef"][l]
                    dev_c = torch.zeros_like(coef)
                    for alt, valid in ev.values():
                        dev_c = torch.maximum(dev_c, torch.where(valid[:, None], (alt["coef"][l] - coef).abs(),
                                                                 torch.zeros(()).double()))
                        if l == 0:
                            hit = (valid & fg & alt["case_b"])[:, None] & (alt["coef"][0] > 0)
                            reach_b[idx[hit]] = True
                    zero = torch.zeros(C, side * side, dtype=torch.float64)
                    gw = (coef[None] * gT[:, :, None]).reshape(C, -1)
                    cmax = coef.abs() + dev_c                  # no admissible coefficient is larger: the roundings' scale
                    live = ((cmax != 0) & fg[:, None])[None].expand(C, -1, -1).double().reshape(C, -1)
                    sl = (dev_c[None] * gT.abs()[:, :, None]).reshape(C, -1)
                    d.append(zero.scatter_add(1, ix, gw).reshape(C, side, side))
                    s.append(zero.scatter_add(1, ix, (cmax[None] * gT.abs()[:, :, None]).reshape(C, -1)).reshape(C, side, side))
                    n.append(zero.scatter_add(1, ix, live).reshape(C, side, side))
                    slack.append(zero.scatter_add(1, ix, sl).reshape(C, side, side))
                want = V.pull_transpose(d, wl)
                s0, slack0 = V.pull_transpose(s, wl), V.pull_transpose(slack, wl)
                n0 = n[-1]
                for l in range(L, 0, -1):                                 # counts fold with weight 1 where w > 0
                    n0 = n[l - 1] + V._up2(n0) * (wl[l - 1] > 0)
                berr = (gotb - want).abs()
                bbound = (n0 + 18 + 5 * L + 2) * ULP * s0 + slack0
                worst_b = max(worst_b, float((berr / bbound.clamp(min=1e-300)).max()))
                assert bool((berr <= bbound).all()), (C, with_idx, L, name, float(berr.max()), worst_b)
                # uncovered texels take no gradient, except the level-0 taps of case (b) pixels
                dead = (w0 == 0) & ~reach_b.reshape(R, R)
                assert bool((gotb[:, dead] == 0).all()), (C, L, name)
    assert seen_b > 0 and seen_c > 0                      # both non-trivial cases occurred
    print("lookup R=%d bias=%.2f: max backward err / bound = %.3g, %d case (b) and %d case (c) pixels" % (
        R, bias, worst_b, seen_b, seen_c))
