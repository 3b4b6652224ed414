"""float64 reference of the background net (csrc/bg.hip: frequency encoding of degree 6, 39 -> 64 ReLU -> C), the
directions and the error scales shared by tests/test_bg_reference_cpu.py and tests/test_gpu_bg_net.py.

The reference is oracle.nerf_oracle.freq_encode / bg_mlp (dtype-generic) on the f32 directions and parameters cast to
float64; gradients are float64 autograd.  The parameters are init_bg_params(out_dim=C, seed=0); w1, b1 are drawn first and
do not depend on C.  The directions are at most 1024 distinct unit vectors (torch.Generator().manual_seed(0), normalised
randn, rows 0..5 overwritten with the six axis directions, the few rows that miss the ReLU condition below left out),
tiled to the wanted N.

ReLU condition.  With A = |b1_h| + sum_i |w1_hi enc_i| (the sum of the magnitudes of a pre-activation's 40 terms), every
float64 hidden pre-activation of every distinct direction has |pre| > 64 * 2^-24 * A: an f32 evaluation (39 fused
multiply-adds, sines and cosines of a few ulp) is within that of the float64 value, so it cannot take the other branch,
and the float64 derivative is the derivative of what the kernel computes."""
import torch

from oracle import nerf_oracle as O

ULP = 2.0 ** -24
N_DISTINCT = 1024
RELU_MARGIN = 64 * ULP


def bg_params(C):
    return O.init_bg_params(out_dim=C, seed=0)


_DISTINCT = []


def distinct_directions():
    """The distinct directions, [D,3] f32, D <= 1024: the six axes, then the drawn vectors whose 64 pre-activations all
    clear twice the ReLU margin (a choice made on the float64 reference alone; a handful of the 1024 are left out)."""
    if not _DISTINCT:
        g = torch.Generator().manual_seed(0)
        d = torch.nn.functional.normalize(torch.randn(N_DISTINCT, 3, generator=g), dim=-1)
        d[:6] = torch.tensor([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
        _, pre, A = bg_hidden(d, bg_params(1))
        ok = (pre.abs() / A).amin(1) > 2 * RELU_MARGIN
        assert bool(ok[:6].all())
        _DISTINCT.append(d[ok].contiguous())
    return _DISTINCT[0]


def bg_directions(N):
    """[N,3] f32 unit vectors: row n is distinct direction n % D."""
    d = distinct_directions()
    return d[torch.arange(N) % d.shape[0]].contiguous()


def bg_hidden(dirs, params):
    """float64: enc [n,39], pre [n,64], A [n,64] (the sum of the magnitudes of the 40 terms of pre)."""
    enc = O.freq_encode(dirs.double())
    w1, b1 = params["w1"].double(), params["b1"].double()
    pre = enc @ w1.T + b1
    A = enc.abs() @ w1.abs().T + b1.abs()
    return enc, pre, A


def relu_margin(params):
    """The smallest |pre| / A over the hidden units of the distinct directions (to be > RELU_MARGIN)."""
    _, pre, A = bg_hidden(distinct_directions(), params)
    return float((pre.abs() / A).min())


def bg_forward_ref(dirs, params):
    """-> out [n,C] float64 and the forward scale B [n,C] = sum_h |w2_ch| A_h + |b2_c|."""
    p = {k: v.double() for k, v in params.items()}
    out = O.bg_mlp(dirs.double(), p)
    _, _, A = bg_hidden(dirs, params)
    B = A @ p["w2"].abs().T + p["b2"].abs()
    return out, B


def bg_backward_ref(dirs, params, dout):
    """float64 autograd gradients of sum(out * dout) -> dict(w1, b1, w2, b2), and for every element the scale S: the sum
    over rays of the magnitudes of its per-ray terms, every term expanded down to the products the kernel forms
    (dh = sum_c w2_ch dout_c -> sum_c |w2_ch dout_c|; hid = relu(pre) -> A where the unit is active):
        db2_c = sum_n |dout_nc|                      dw2_ch = sum_n |dout_nc| A_nh [pre_nh > 0]
        db1_h = sum_n Dh_nh                          dw1_hi = sum_n Dh_nh |enc_ni|,   Dh_nh = [pre_nh > 0] sum_c |w2_ch dout_nc|."""
    p = {k: v.double().requires_grad_() for k, v in params.items()}
    out = O.bg_mlp(dirs.double(), p)
    grads = torch.autograd.grad(out, [p[k] for k in ("w1", "b1", "w2", "b2")], dout.double())
    enc, pre, A = bg_hidden(dirs, params)
    act = (pre > 0).double()
    da = dout.double().abs()
    Dh = (da @ params["w2"].double().abs()) * act
    S = {"b2": da.sum(0), "w2": da.T @ (A * act), "b1": Dh.sum(0), "w1": Dh.T @ enc.abs()}
    return dict(zip(("w1", "b1", "w2", "b2"), grads)), S
