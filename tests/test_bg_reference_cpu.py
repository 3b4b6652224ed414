"""tests/bg_reference.py without a GPU: the ReLU condition the GPU tests rely on, the direction set, and the reference
against the f32 oracle under the bounds tests/test_gpu_bg_net.py uses."""
import pytest
import torch

from oracle import nerf_oracle as O
from tests import bg_reference as R


def test_directions_are_distinct_unit_vectors_with_the_axes():
    d = R.distinct_directions()
    assert 1000 < d.shape[0] <= R.N_DISTINCT and torch.unique(d, dim=0).shape[0] == d.shape[0]
    assert float((d.double().norm(dim=-1) - 1).abs().max()) < 2e-7
    axes = torch.tensor([[1., 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
    assert torch.equal(d[:6], axes)
    tiled = R.bg_directions(2 * d.shape[0] + 5)
    assert torch.equal(tiled[d.shape[0]:2 * d.shape[0]], d) and torch.equal(tiled[-5:], d[:5])


@pytest.mark.parametrize("C", [1, 3, 4])
def test_relu_condition(C):
    """Every float64 hidden pre-activation of every distinct direction is further than 64 * 2^-24 * A from zero."""
    p = R.bg_params(C)
    assert p["w2"].shape == (C, 64) and torch.equal(p["w1"], R.bg_params(4)["w1"])
    margin = R.relu_margin(p)
    print("background net C=%d: smallest |pre| / A = %.3e (required %.3e)" % (C, margin, R.RELU_MARGIN))
    assert margin > R.RELU_MARGIN
    _, pre, _ = R.bg_hidden(R.distinct_directions(), p)
    act = (pre > 0).double().mean()
    assert 0.2 < float(act) < 0.8                                                  # both branches are taken


@pytest.mark.parametrize("C", [1, 3, 4])
def test_f32_oracle_is_within_the_bounds_of_the_gpu_tests(C):
    """An f32 CPU evaluation (another summation order than the kernel's) sits well inside the forward bound
    2^-24 (39 + 64 + 8) B and the backward bound 2^-24 (111 + 64 + tiles) S."""
    N = 1000
    d, p = R.bg_directions(N), R.bg_params(C)
    want, B = R.bg_forward_ref(d, p)
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    got = O.bg_mlp(d, pr)
    r = float(((got.detach().double() - want).abs() / (R.ULP * 111 * B)).max())
    assert r <= 1.0, r
    dout = torch.randn(N, C, generator=torch.Generator().manual_seed(C))
    got.backward(dout)
    grads, S = R.bg_backward_ref(d, p, dout)
    tiles = (N + 63) // 64
    for k in ("w1", "b1", "w2", "b2"):
        tol = R.ULP * (111 + 64 + tiles) * S[k].reshape(grads[k].shape)
        err = (pr[k].grad.double() - grads[k]).abs()
        assert bool((err <= tol).all()), (k, float((err / tol.clamp(min=1e-300)).max()))
        assert bool((grads[k].abs() <= S[k].reshape(grads[k].shape) * (1 + 1e-12)).all())   # S bounds the gradient itself
