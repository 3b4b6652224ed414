"""float64 references of the mip-mapped texture lookup (csrc/texmip.hip; the contracts are in include/lnerf_hip.h):
the pixel footprint with a running error bound, the box pyramid and its transpose, and the trilinear taps and weights.

The footprint's error bound is a running error analysis.  Every intermediate of the kernel is tracked as (v, m, k): its
float64 value, a count k of roundings and a magnitude m with the invariant |fl(v) - v| <= k * ULP * m (ULP = 2^-24, the
relative error of one f32 operation).  With da = k_a ULP m_a the error an operand brings along, each rule is the error
of one operation written out, its own rounding ULP |c| included, and divided by k:
    leaf (an f32 input)   no error                                                          k = 0
    c = a +- b            k m = k_a m_a + k_b m_b + |c|                                     k = max(k_a, k_b) + 1
    c = a * b             k m = k_a |b| m_a + k_b |a| m_b + k_a k_b ULP m_a m_b + |c|       k = k_a + k_b + 1
    c = a / b             k m = (k_a m_a / |b| + k_b |a| m_b / b^2) / (1 - eps_b) + |c|     k = k_a + k_b + 1
                          with eps_b = k_b ULP m_b / |b| < 1/2, the divisor's own relative error
    c = sqrt(a^2 + b^2)   k m = k_a m_a + k_b m_b + 3 |c|                                   k = max(k_a, k_b) + 3
                          (1-Lipschitz in (a, b); two squares, a sum and a root of positive terms: < 3 ULP)
    c = max(a, b)         k m = max(k_a m_a, k_b m_b)                                       k = max(k_a, k_b)
So m is a weighted sum of the absolute values of the terms that entered, not a multiple of |v|: where the quotient rule
cancels (a near-affine face) v goes to zero and m stays at the size of the terms, and a divisor's own cancellation
enters through m_b / |b|.  A difference of two inputs costs ULP times the difference, which is what keeps the bound
useful on triangles much smaller than a pixel.
k of the result is a property of the expression alone: FOOTPRINT_ROUNDINGS."""
import numpy as np
import torch

ULP = 2.0 ** -24

# k of rho for the kernel as written (k_uv_footprint): area, e_k 4 -> inv 5 -> w0, w1 10 -> w2 12 -> q2 13 -> qs 14
# -> z 15 -> bw2 29;  dw_k 7 -> dw2 8 -> a2 9 -> s 10;  bw2 * s 40 -> a2 - .. 41 -> (..) * z 57 -> u2 * .. 58 -> the sum
# of three 59 (the other two products are at 56) -> the root 62 -> * (2 / W) 64.  test_mip_cpu.py checks that the
# tracker arrives at the same number.
FOOTPRINT_ROUNDINGS = 64


class Tracked:
    __slots__ = ("v", "m", "k")

    def __init__(self, v, m=None, k=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.m = np.abs(self.v) if m is None else m
        self.k = k

    def _sum(a, b, v):
        k = max(a.k, b.k) + 1
        return Tracked(v, (a.k * a.m + b.k * b.m + np.abs(v)) / k, k)

    def __add__(a, b):
        return a._sum(b, a.v + b.v)

    def __sub__(a, b):
        return a._sum(b, a.v - b.v)

    def __neg__(a):
        return Tracked(-a.v, a.m, a.k)

    def __mul__(a, b):
        k, v = a.k + b.k + 1, a.v * b.v
        m = a.k * np.abs(b.v) * a.m + b.k * np.abs(a.v) * b.m + a.k * b.k * ULP * a.m * b.m + np.abs(v)
        return Tracked(v, m / k, k)

    def __truediv__(a, b):
        eps = b.k * ULP * b.m / np.abs(b.v)
        assert bool((eps < 0.5).all()), "a divisor lost all its digits: the bound does not exist"
        k, v = a.k + b.k + 1, a.v / b.v
        m = (a.k * a.m / np.abs(b.v) + b.k * np.abs(a.v) * b.m / (b.v * b.v)) / (1.0 - eps) + np.abs(v)
        return Tracked(v, m / k, k)


def _hypot(a, b):
    k, v = max(a.k, b.k) + 3, np.hypot(a.v, b.v)
    return Tracked(v, (a.k * a.m + b.k * b.m + 3 * v) / k, k)


def _max(a, b):
    k = max(a.k, b.k)
    return Tracked(np.maximum(a.v, b.v), np.maximum(a.k * a.m, b.k * b.m) / k, k)


def pixel_centres(H, W):
    """k_rasterize's pixel centres in NDC with its f32 arithmetic (the same bits), as float64."""
    j = torch.arange(W, dtype=torch.float32)
    i = torch.arange(H, dtype=torch.float32)
    return ((2 * j + 1) / W - 1).double().numpy(), (1 - (2 * i + 1) / H).double().numpy()


def uv_derivatives(xy, z, uv, px, py):
    """The analytic screen-space UV derivatives on one face per point: xy [N,3,2], z [N,3], uv [N,3,2], px, py [N]
    (arrays of f32-representable values) -> Tracked (du/dpx, dv/dpx, du/dpy, dv/dpy), the kernel's expression tree."""
    T = Tracked
    x = [T(xy[:, k, 0]) for k in range(3)]
    y = [T(xy[:, k, 1]) for k in range(3)]
    zz = [T(z[:, k]) for k in range(3)]
    px, py = T(px), T(py)
    one = T(np.ones_like(px.v))
    area = (x[1] - x[0]) * (y[2] - y[0]) - (x[2] - x[0]) * (y[1] - y[0])
    e0 = (x[1] - px) * (y[2] - py) - (x[2] - px) * (y[1] - py)
    e1 = (x[2] - px) * (y[0] - py) - (x[0] - px) * (y[2] - py)
    inv = one / area
    w0, w1 = e0 * inv, e1 * inv
    w = [w0, w1, one - w0 - w1]
    q = [w[k] / zz[k] for k in range(3)]
    qs = q[0] + q[1] + q[2]
    zc = one / qs
    bw = [q[k] * zc for k in range(3)]
    out = []
    for d0, d1 in (((y[1] - y[2]) * inv, (y[2] - y[0]) * inv), ((x[2] - x[1]) * inv, (x[0] - x[2]) * inv)):
        dw = [d0, d1, -d0 - d1]
        a = [dw[k] / zz[k] for k in range(3)]
        s = a[0] + a[1] + a[2]
        dbw = [(a[k] - bw[k] * s) * zc for k in range(3)]
        for c in range(2):
            t = [T(uv[:, k, c]) * dbw[k] for k in range(3)]
            out.append(t[0] + t[1] + t[2])
    return tuple(out)


def interp_uv(xy, z, uv, px, py):
    """The perspective-correct interpolant itself in float64: (u, v) [N] at (px, py) -- what uv_derivatives differentiates."""
    x, y = xy[..., 0], xy[..., 1]
    area = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (x[:, 2] - x[:, 0]) * (y[:, 1] - y[:, 0])
    e0 = (x[:, 1] - px) * (y[:, 2] - py) - (x[:, 2] - px) * (y[:, 1] - py)
    e1 = (x[:, 2] - px) * (y[:, 0] - py) - (x[:, 0] - px) * (y[:, 2] - py)
    w = np.stack([e0 / area, e1 / area, 1 - e0 / area - e1 / area], -1)
    q = w / z
    bw = q / q.sum(-1, keepdims=True)
    return (bw * uv[..., 0]).sum(-1), (bw * uv[..., 1]).sum(-1)


def footprint(face_idx, face_xy, face_z, face_uv, B, H, W):
    """lnerf_uv_footprint in float64 from the f32 arrays the rasteriser wrote: face_idx [B*H*W], face_xy [B,F,3,2],
    face_z [B,F,3], face_uv [F,3,2] (torch CPU tensors) -> (rho [P], scale [P], k): |rho_f32 - rho| <= k ULP scale."""
    idx = face_idx.long().numpy().reshape(B, H * W)
    fxy, fz, fuv = face_xy.double().numpy(), face_z.double().numpy(), face_uv.double().numpy()
    cx, cy = pixel_centres(H, W)
    rho = np.zeros((B, H * W))
    scale = np.zeros((B, H * W))
    k = 0
    for b in range(B):
        fg = np.nonzero(idx[b] >= 0)[0]
        if fg.size == 0:
            continue
        f = idx[b, fg]
        ux, vx, uy, vy = uv_derivatives(fxy[b, f], fz[b, f], fuv[f], cx[fg % W], cy[fg // W])
        two = Tracked(np.full(fg.size, 2.0))
        r = _max(_hypot(ux, vx) * (two / Tracked(np.full(fg.size, float(W)))),
                 _hypot(uy, vy) * (two / Tracked(np.full(fg.size, float(H)))))
        rho[b, fg], scale[b, fg], k = r.v, r.m, r.k
    return rho.reshape(-1), scale.reshape(-1), k


# ------------------------------------------------------------------------------------------------------- pyramid
def full_levels(R):
    """The trailing zero bits of R."""
    return (R & -R).bit_length() - 1


def level_offsets(R, L):
    """Start of level l = 1..L inside one channel of the packed buffer, and the channel's length S."""
    offs, at = {}, 0
    for l in range(1, L + 1):
        offs[l] = at
        at += (R >> l) ** 2
    return offs, at


def pyramid(tex, L):
    """tex [C,R,R] -> [level 0, ..., level L] in float64: level l = the 2 x 2 box average of level l - 1."""
    levels = [tex.double()]
    for _ in range(L):
        t = levels[-1]
        C, r = t.shape[0], t.shape[1]
        levels.append(t.reshape(C, r // 2, 2, r // 2, 2).mean(dim=(2, 4)))
    return levels


def pyramid_abs_step(level):
    """One box average of |level|: what the forward's 4 ULP per level are relative to."""
    C, r = level.shape[0], level.shape[1]
    return level.abs().reshape(C, r // 2, 2, r // 2, 2).mean(dim=(2, 4))


def pyramid_transpose(dlevels):
    """The transpose of `pyramid`: gradients of [level 0, ..., level L] -> the gradient of level 0, from the coarsest
    level down d[l-1][c,i,j] += 0.25 d[l][c,i/2,j/2]."""
    acc = dlevels[-1].double()
    for d in reversed(dlevels[:-1]):
        acc = d.double() + 0.25 * acc.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    return acc


def pack(levels):
    """[level 1, ..., level L] -> the packed [C,S] buffer."""
    return torch.cat([l.reshape(l.shape[0], -1) for l in levels], dim=1)


def unpack(packed, R, L):
    """The packed [C,S] buffer -> [level 1, ..., level L]."""
    offs, _ = level_offsets(R, L)
    return [packed[:, offs[l]:offs[l] + (R >> l) ** 2].reshape(-1, R >> l, R >> l) for l in range(1, L + 1)]


# ------------------------------------------------------------------------------------------------------- lookup
def tex_coords(uv, R):
    """csrc/tex_shared.h tex_coords (clip = true) in f32: the same operations in the same order."""
    u, v = uv[:, 0].clamp(0, 1), uv[:, 1].clamp(0, 1)
    gx, gy = u * 2.0 - 1.0, -(v * 2.0 - 1.0)
    x = (((gx + 1.0) * float(R) - 1.0) * 0.5).clamp(0, R - 1)
    y = (((gy + 1.0) * float(R) - 1.0) * 0.5).clamp(0, R - 1)
    return x, y


def bilinear_taps(uv, R):
    """(texel index [P,4] into R*R, float64 weight [P,4]) of the bilinear lookup on an R x R level."""
    x, y = tex_coords(uv.float(), R)
    xf, yf = torch.floor(x), torch.floor(y)
    ax, ay = (x - xf).double(), (y - yf).double()
    x0, y0 = xf.long(), yf.long()
    x1, y1 = (x0 + 1).clamp(max=R - 1), (y0 + 1).clamp(max=R - 1)
    idx = torch.stack([y0 * R + x0, y0 * R + x1, y1 * R + x0, y1 * R + x1], -1)
    w = torch.stack([(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay], -1)
    return idx, w


def lod(rho, R, L, bias):
    """lambda [P] in float64 from the f32 footprint: clamp(log2(rho R) + bias, 0, L), 0 where rho R <= 0."""
    s = rho.double() * R
    lam = (torch.log2(s.clamp(min=1e-300)) + float(bias)).clamp(0, L)
    return torch.where(s > 0, lam, torch.zeros_like(lam))


def level_weights(lam, L):
    """[L+1,P]: the weight of every level in the trilinear mix: 1 - t on l0 = min(floor(lambda), L), t on l0 + 1."""
    l0 = lam.floor().clamp(max=L).long()
    t = lam - l0
    w = torch.zeros(L + 1, lam.shape[0], dtype=torch.float64)
    w.scatter_(0, l0[None], (1 - t)[None])
    up = t > 0
    w[:, up] = w[:, up].scatter(0, (l0[up] + 1)[None], t[up][None])
    return w, l0, t


def bilinear_levels(levels, uv):
    """bil(l) [L+1,P,C] of every level and the bound's scale sum |w| |texel| [L+1,P,C]; levels = [C,r,r] tensors."""
    vals, scales, taps = [], [], []
    for lev in levels:
        C, r = lev.shape[0], lev.shape[1]
        idx, w = bilinear_taps(uv, r)
        flat = lev.double().reshape(C, r * r)
        vals.append((flat[:, idx] * w[None]).sum(-1).T)
        scales.append((flat[:, idx].abs() * w[None]).sum(-1).T)
        taps.append((idx, w))
    return torch.stack(vals), torch.stack(scales), taps
