"""float64 references of the coverage-weighted pyramids (csrc/texmip.hip; the contracts are in include/lnerf_hip.h):
the weights, the pull and its transpose, the push, and the normalised trilinear lookup.  Taps, lambda, the packing and
the ULP come from tests/mip_reference.py.

Every reference takes the WEIGHTS as f32 tensors (level 0 and the levels a kernel or `weight_levels_f32` made of it) and
reads them exactly as the kernels do, so that the kernels' branch decisions -- s > 0, k == 1, k == 0, every W == 1,
D == 0 -- are taken from the very f32 values the kernels see: `_s32` adds four f32 children in the kernel's order, which
IEEE arithmetic makes the same bits on any machine.  Everything else is float64.

Each function that a bound hangs on also returns the MAGNITUDE the bound is relative to, propagated by the same rule as
the value with absolute values in place of the values (so |value| <= magnitude throughout)."""
import torch

from tests import mip_reference as M

ULP = M.ULP
TINY = 1e-12          # how near an integer lambda the open cells next to it are evaluated


def _kids(x):
    """[..., r, r] -> the four children of every coarse texel in the kernels' order 00, 01, 10, 11."""
    return x[..., 0::2, 0::2], x[..., 0::2, 1::2], x[..., 1::2, 0::2], x[..., 1::2, 1::2]


def _s32(w):
    """s = (wa + wb) + (wc + wd) in f32, the kernels' bits."""
    a, b, c, d = _kids(w.float())
    return (a + b) + (c + d)


def weight_levels(w0, L):
    """[w_0 .. w_L] in float64: w_l = the sum of the four children / 4."""
    out = [w0.double()]
    for _ in range(L):
        a, b, c, d = _kids(out[-1])
        out.append(((a + b) + (c + d)) * 0.25)
    return out


def weight_levels_f32(w0, L):
    """[w_0 .. w_L] with the kernel's f32 operations in the kernel's order: its bits for ANY input weights."""
    out = [w0.float()]
    for _ in range(L):
        out.append(_s32(out[-1]) * 0.25)
    return out


def pack_weights(levels):
    """[w_1 .. w_L] -> the packed [S] buffer."""
    return torch.cat([l.reshape(-1) for l in levels]) if levels else None


def unpack_weights(w0, wpyr, R, L):
    """w0 [R,R] and the packed [S] -> [w_0 .. w_L] (f32)."""
    offs, _ = M.level_offsets(R, L)
    return [w0.float()] + [wpyr[offs[l]:offs[l] + (R >> l) ** 2].reshape(R >> l, R >> l).float() for l in range(1, L + 1)]


def pull(tex, wl, L):
    """tex [C,R,R], wl = f32 [w_0 .. w_L] -> (values [v_0 = tex, v_1 .. v_L], magnitudes) in float64:
    v_l = sum w v / sum w over the four children where the f32 sum is > 0, else 0."""
    vals, mags = [tex.double()], [tex.double().abs()]
    for l in range(1, L + 1):
        live = _s32(wl[l - 1]) > 0
        a, b, c, d = (k.double() for k in _kids(wl[l - 1]))
        s = torch.where(live, (a + b) + (c + d), torch.ones(()).double())
        for src, dst in ((vals, vals), (mags, mags)):
            ta, tb, tc, td = _kids(src[l - 1])
            dst.append(torch.where(live, (a * ta + b * tb + c * tc + d * td) / s, torch.zeros(()).double()))
    return vals, mags


def _up2(x):
    return x.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def pull_transpose(dlevels, wl):
    """The transpose of `pull` in the values: gradients of [v_0 .. v_L] -> the gradient of v_0, from the coarsest level
    down d[l-1][child] += (w_child / s) d[l][parent], nothing where the f32 s is not > 0."""
    acc = dlevels[-1].double()
    for l in range(len(dlevels) - 1, 0, -1):
        w = wl[l - 1]
        s32 = _up2(_s32(w))
        a, b, c, d = (k.double() for k in _kids(w))
        s = _up2((a + b) + (c + d))
        q = torch.where(s32 > 0, w.double() / torch.where(s32 > 0, s, torch.ones(()).double()), torch.zeros(()).double())
        acc = dlevels[l - 1].double() + q * _up2(acc)
    return acc


def _neighbours(r):
    """For the r fine rows (or columns): the parent index and the other tap's index on the level of side r / 2."""
    i = torch.arange(r)
    p = i // 2
    n = torch.where(i % 2 == 1, (p + 1).clamp(max=r // 2 - 1), (p - 1).clamp(min=0))
    return p, n


def push(tex, wl, vals, mags, L):
    """The push over the pulled `vals` / `mags` (pull's) -> (F [F_0 .. F_L], magnitudes M [M_0 .. M_L], filled [R,R]
    bool, reached [R,R] bool).  k is taken from the f32 weights in the kernel's order; a texel is reached when its
    level-L ancestor has w_L > 0; up is the 2 x bilinear upsample over the reached taps, renormalised."""
    R = tex.shape[-1]
    top = wl[L] > 0
    F, Mg = [None] * (L + 1), [None] * (L + 1)
    F[L], Mg[L] = vals[L].clone(), mags[L].clone()
    reached0 = top if L == 0 else None
    for l in range(L - 1, -1, -1):
        r = R >> l
        k32 = wl[0].float() if l == 0 else torch.minimum(_s32(wl[l - 1]), torch.ones(()))
        k = k32.double()
        reach_c = top.repeat_interleave(1 << (L - l - 1), 0).repeat_interleave(1 << (L - l - 1), 1)   # level l + 1
        p, n = _neighbours(r)
        taps = ((p, p, 9 / 16), (p, n, 3 / 16), (n, p, 3 / 16), (n, n, 1 / 16))
        den = sum(torch.where(reach_c[I][:, J], b, 0.0) for I, J, b in taps).double()
        me = reach_c[p][:, p]
        safe = torch.where(me, den, torch.ones(()).double())
        out = []
        for src, own in ((F[l + 1], vals[l]), (Mg[l + 1], mags[l])):
            num = sum(torch.where(reach_c[I][:, J], b * src[:, I][:, :, J], torch.zeros(()).double()) for I, J, b in taps)
            up = num / safe
            new = torch.where(k32 == 1, own, torch.where(k32 == 0, up, k * own + (1 - k) * up))
            out.append(torch.where(me, new, own))
        F[l], Mg[l] = out
        if l == 0:
            reached0 = me
    filled = reached0 & (wl[0] != 1) if L > 0 else torch.zeros(R, R, dtype=torch.bool)
    return F, Mg, filled, reached0


# ------------------------------------------------------------------------------------------------------- lookup
class Lookup:
    """Everything of the normalised lookup that does not depend on lambda: per level the taps (index, float64 weight),
    the f32 decisions and the float64 sums.  levels = [V_0 .. V_L] ([C,r,r]), wl = f32 [w_0 .. w_L], uv [P,2]."""

    def __init__(self, levels, wl, uv):
        self.L = len(levels) - 1
        self.P, self.C = uv.shape[0], levels[0].shape[0]
        self.taps, self.bw, self.n, self.nabs, self.d, self.ones, self.dzero, self.plain, self.pabs = ([] for _ in range(9))
        for lev, w in zip(levels, wl):
            C, r = lev.shape[0], lev.shape[1]
            idx, b = M.bilinear_taps(uv, r)                       # [P,4], float64 weights of the f32 fractions
            W = w.reshape(-1)[idx]                                # [P,4] f32
            bw32 = b.float() * W                                  # the kernel's products decide D == 0
            d32 = ((bw32[:, 0] + bw32[:, 1]) + bw32[:, 2]) + bw32[:, 3]
            V = lev.double().reshape(C, r * r)[:, idx]            # [C,P,4]
            bw = b * W.double()
            self.taps.append((idx, b))
            self.bw.append(bw)
            self.n.append((bw[None] * V).sum(-1).T)               # [P,C]
            self.nabs.append((bw[None] * V.abs()).sum(-1).T)
            self.d.append(bw.sum(-1))                             # [P]
            self.ones.append((W == 1).all(-1))
            self.dzero.append(d32 == 0)
            self.plain.append((b[None] * V).sum(-1).T)
            self.pabs.append((b[None] * V.abs()).sum(-1).T)

    def _pick(self, per_level, l):
        return torch.stack(per_level)[l, torch.arange(self.P)]

    def at(self, l0, t):
        """The lookup at lambda = l0 + t per pixel (l0 [P] long, t [P] float64 in [0, 1); t == 0 reads one level).
        -> dict(out [P,C], bound [P,C], coef [L+1][P,4], case_a [P], case_b [P]): coef = d out / d V per tap of every
        level (the backward's addend per unit gradient), bound = the forward's rounding bound (derived in
        tests/test_gpu_mipcov.py), case_a / case_b = the header's cases (a) and (b); the rest is case (c)."""
        two = t > 0
        l1 = (l0 + 1).clamp(max=self.L)
        m0, m1 = torch.where(two, 1 - t, torch.ones_like(t)), torch.where(two, t, torch.zeros_like(t))
        pick = self._pick
        D = m0 * pick(self.d, l0) + m1 * pick(self.d, l1)
        ones = pick(self.ones, l0) & (pick(self.ones, l1) | ~two)
        dzero = pick(self.dzero, l0) & (pick(self.dzero, l1) | ~two)
        plain = ones | dzero
        N = m0[:, None] * pick(self.n, l0) + m1[:, None] * pick(self.n, l1)
        Nabs = m0[:, None] * pick(self.nabs, l0) + m1[:, None] * pick(self.nabs, l1)
        Pl = m0[:, None] * pick(self.plain, l0) + m1[:, None] * pick(self.plain, l1)
        Pabs = pick(self.pabs, l0) + torch.where(two[:, None], pick(self.pabs, l1), torch.zeros(()).double())
        Dsafe = torch.where(plain, torch.ones_like(D), D)
        out = torch.where(plain[:, None], Pl, N / Dsafe[:, None])
        bound = torch.where(plain[:, None], PLAIN_ULPS * ULP * Pabs, COV_ULPS * ULP * Nabs / Dsafe[:, None])
        coef = []
        for l in range(self.L + 1):
            mix = torch.where(l0 == l, m0, torch.zeros_like(t)) + torch.where((l1 == l) & two, m1, torch.zeros_like(t))
            c = torch.where(plain[:, None], self.taps[l][1], self.bw[l] / Dsafe[:, None])
            coef.append(mix[:, None] * c)
        return {"out": out, "bound": bound, "coef": coef, "case_a": ones, "case_b": dzero & ~ones}


# Rounding counts of the forward, derived in tests/test_gpu_mipcov.py
PLAIN_ULPS = 4 + 2        # the plain mode's tap bound (tests/test_gpu_mip.py TAP_ULPS) on the absolute sum of both levels
COV_ULPS = 22             # case (c): N and D are each within 10 ulp, the quotient adds one, one for second order


def lambda_pieces(lam, dl, L):
    """The lambdas a kernel whose f32 lambda is within dl of `lam` (float64, [P]) may have used, as evaluation points
    (l0, t, valid): for a pixel with no integer within dl the two ends of [lam - dl, lam + dl]; else the ends of the
    open piece below the integer m, m itself (t == 0: one level), and the ends of the open piece above it.  Within an
    open piece the lookup is (a + b t) / (c + e t) in t -- monotone -- so its values lie between the piece's ends.
    -> list of (name, l0, t, valid) and the list of pieces as (first, last) names; single points are (name, name)."""
    lo, hi = (lam - dl).clamp(0, L), (lam + dl).clamp(0, L)
    m = lam.round()
    near = (lam - m).abs() <= dl
    cell = lam.floor().clamp(max=L)
    zero = torch.zeros_like(lam)
    # far from an integer: one piece inside the cell of lam
    pts = [("a", cell.long(), torch.where(near, zero, lo - cell), ~near),
           ("b", cell.long(), torch.where(near, zero, hi - cell), ~near)]
    # near the integer m: below (cell m - 1), at, above (cell m)
    below = near & (m >= 1) & (lo < m)
    above = near & (m < L) & (hi > m)
    lm = (m - 1).clamp(min=0)
    pts += [("c", lm.long(), torch.where(below, (lo - lm).clamp(TINY, 1 - TINY), zero), below),
            ("d", lm.long(), torch.where(below, torch.full_like(lam, 1 - TINY), zero), below),
            ("m", m.long().clamp(0, L), zero, near),
            ("e", m.long().clamp(0, L), torch.where(above, torch.full_like(lam, TINY), zero), above),
            ("f", m.long().clamp(0, L), torch.where(above, (hi - m).clamp(TINY, 1 - TINY), zero), above)]
    return pts, (("a", "b"), ("c", "d"), ("m", "m"), ("e", "f"))
