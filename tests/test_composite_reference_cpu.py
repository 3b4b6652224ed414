"""tests/composite_reference.py against the oracle and against tests/latent_tune_reference.py::weights64, and the
conditions that tests/test_gpu_composite.py relies on, for every one of its input cases (no GPU)."""
import math

import pytest
import torch

from oracle import nerf_oracle as O
from tests import composite_reference as R
from tests.latent_tune_reference import weights64


def _parity_inputs(C):
    """The inputs of tests/test_gpu_parity.py::test_composite_forward_backward."""
    torch.manual_seed(C)
    cnts = torch.tensor([0, 5, 1, 64, 65, 3, 0, 300, 128, 2])
    N = len(cnts)
    offs = torch.cumsum(cnts, 0) - cnts
    M = int(cnts.sum())
    rays = torch.stack([torch.randperm(N), offs, cnts], -1).int()
    sig = torch.rand(M) * 20
    sig[offs[7]:offs[7] + 300] = torch.rand(300) * 400
    rgb = torch.randn(M, C)
    dl = torch.stack([torch.full((M,), 3.4e-3), torch.rand(M) + 0.3], -1)
    bg = torch.rand(N, C)
    return sig, rgb, dl, rays, bg


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("with_bg", [True, False])
def test_reference_matches_the_oracle(C, with_bg):
    """Cast to f32, within COMPOSITE_TOL(k) x the largest value of each output (as tests/test_gpu_latent_tune.py)."""
    sig, rgb, dl, rays, bg = _parity_inputs(C)
    ids = rays[:, 0].long()
    bg_by_id = torch.zeros_like(bg).index_copy(0, ids, bg) if with_bg else None      # the oracle's bg is by ray id
    ws, dp, img = O.composite_rays_train(sig, rgb, dl, rays, 1e-4, bg_by_id)
    ref = R.composite_reference(sig.double(), rgb.double(), dl.double(), rays, 1e-4,
                                None if bg_by_id is None else bg_by_id.double())
    assert ref["margin"] > 1e-3
    k = ref["count"].double()
    for name, got in (("weights_sum", ws), ("depth", dp), ("image", img)):
        want = ref[name].float()
        err = (got - want).abs().double()
        err = err.amax(-1) if err.dim() == 2 else err
        tol = R.COMPOSITE_TOL(k) * float(want.abs().max())
        assert bool((err <= tol).all()), (name, float((err / tol).max()))


@pytest.mark.parametrize("T_thresh", [1e-4, 1e-2])
def test_reference_matches_weights64(T_thresh):
    sig, rgb, dl, rays, _ = _parity_inputs(4)
    ref = R.composite_reference(sig.double(), rgb.double(), dl.double(), rays, T_thresh)
    w, idx, valid, keep, margin = weights64(sig.double(), dl.double(), rays, T_thresh)
    assert float((ref["w"][idx[valid]] - w[valid]).abs().max()) <= 1e-12
    assert torch.equal(ref["keep"][idx[valid]], keep[valid])
    assert abs(margin - ref["margin"]) <= 1e-9 * margin
    ids = rays[:, 0].long()
    assert float((ref["weights_sum"][ids] - w.sum(1)).abs().max()) <= 1e-12
    assert int(ref["in_span"].sum()) == int(rays[:, 2].sum()) and torch.equal(ref["count"][ids], rays[:, 2].long())


def test_shifted_prefix_is_exact_where_the_subtraction_is_not():
    """One ray: 20 thin samples, one surface sample, thin samples.  f32 `cumsum - tau` loses the prefix; the shifted
    cumsum does not, at any density, +inf included (the oracle is stated with the shifted form)."""
    for s in R.SAT_SIGMAS:
        sig = torch.full((33,), 0.1 / R.DT)
        sig[20] = s
        dl = torch.stack([torch.full((33,), R.DT), torch.linspace(0.3, 1.3, 33)], -1)
        rays = torch.tensor([[0, 0, 33]], dtype=torch.int32)
        rgb = torch.ones(33, 3)
        ref = R.composite_reference(sig.double(), rgb.double(), dl.double(), rays, 1e-4)
        assert abs(float(ref["w"][20]) - math.exp(-2.0)) < 1e-6
        assert bool(torch.isfinite(ref["weights_sum"]).all()) and float(ref["weights_sum"]) <= 1.0 + 1e-12
        ws, dp, img = O.composite_rays_train(sig, rgb, dl, rays, 1e-4)
        assert abs(float(ws) - float(ref["weights_sum"])) <= R.COMPOSITE_TOL(33), (s, float(ws))


@pytest.mark.parametrize("regime,C,with_bg,T_thresh", R.CASES)
def test_case_meets_what_the_gpu_tests_rely_on(regime, C, with_bg, T_thresh):
    case = R.composite_case(regime, C, with_bg, T_thresh)
    inp, ref = case["inp"], case["ref"]
    N, M = inp["N"], inp["M"]
    assert ref["margin"] > 1e-3, ref["margin"]
    # the table: ids a permutation, gaps between spans and behind the last one
    rays = inp["rays"].long()
    assert sorted(rays[:, 0].tolist()) == list(range(N))
    assert int(ref["in_span"].sum()) == int(rays[:, 2].sum()) < M - 4 and not bool(ref["in_span"][-5:].any())
    ends = (rays[:, 1] + rays[:, 2])[:-1]
    assert bool((rays[1:, 1] > ends).all())
    # everything finite, gradients included
    for key in ("weights_sum", "depth", "image", "w", "T"):
        assert bool(torch.isfinite(ref[key]).all()), key
    for sel, grads in case["ref_grads"].items():
        for key, g in grads.items():
            assert bool(torch.isfinite(g).all()), (sel, key)
    assert float(ref["weights_sum"].max()) <= 1.0 + 1e-12
    offs, cnts = rays[:, 1].tolist(), rays[:, 2].tolist()
    if regime in ("benign", "empty"):
        assert tuple(cnts) == R.SPANS and N % 4 != 0
    if regime == "one":
        assert N == 1
    if regime == "benign" and T_thresh > 0:
        assert int((ref["in_span"] & ~ref["keep"]).sum()) > 100            # the dense span did stop early
    if regime == "empty":
        assert int((inp["sigmas"][ref["in_span"]] == 0).sum()) > 50 and float(ref["weights_sum"].max()) < 2e-3
    if regime == "edge":
        assert len(cnts) == 14
        for r, first in enumerate(inp["meta"]["first_dropped"]):
            keep = ref["keep"][offs[r]:offs[r] + cnts[r]]
            assert bool(keep[:first].all()) and not bool(keep[first:].any()), (r, first)
    if regime == "saturated":
        assert len(cnts) == 20
        for r, s in enumerate(inp["meta"]["surface"]):
            end = offs[r] + cnts[r]
            assert bool(ref["keep"][s]) and abs(float(ref["w"][s]) - (math.exp(-2.0) if s > offs[r] else 1.0)) < 1e-4
            assert float(ref["w"][s + 1:end].abs().max()) == 0.0
            if T_thresh > 0:
                assert not bool(ref["keep"][s + 1:end].any())              # no kept sample behind the surface
    if regime == "bigbg":
        ws = ref["weights_sum"][rays[:, 0]]
        assert float(ws[:4].max()) < 3e-3 and float(ws[4:].min()) > 0.99 and float(inp["bg"].abs().max()) > 95
