"""The inputs of tests/test_gpu_span_weights.py (tests/span_reference.py, weights_case) do what that test says, checked
without a GPU on the float32 restatements of tests/distortion_reference.py and tests/normal_image_reference.py and on the
float64 weights: every normal is exactly (-1, 0, 0), the two restatements give the same weight for every sample bit for
bit, the normal image's y rows carry (-w, +w), and the regimes cut where they are meant to."""
import numpy as np
import pytest

from tests import distortion_reference as D
from tests import normal_image_reference as NI
from tests import span_reference as S


@pytest.mark.parametrize("regime", S.W_REGIMES)
@pytest.mark.parametrize("T_thresh", S.W_T_THRESHES)
def test_restatements_agree_on_the_case(regime, T_thresh):
    k = S.weights_case(regime)
    N, M, rays = k["N"], k["M"], k["rays"]
    rows, ids = S.span_rows(rays)
    assert M == 653 and np.array_equal(rows, np.arange(M)) and sorted(rays[:, 0].tolist()) == list(range(N))
    assert np.isfinite(k["sig"]).all() and (k["sig"] >= 0).all() and (k["deltas"][:, 0] > 0).all()
    for _, off, cnt in rays.tolist():
        assert (np.diff(k["deltas"][off:off + cnt, 1]) > 0).all()
    inv_2eps = 1.0 / (2.0 * S.W_EPS)
    n, s2, r = S.fd_normal(k["sig7"].reshape(-1, 7), inv_2eps, np.float32)
    assert inv_2eps == 1.0 and (n[:, 0] == -1).all() and not n[:, 1:].any() and (s2 == 1).all() and (r == 1).all()
    dN = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (N, 1))
    d32 = D.restate(k["sig"], k["deltas"], rays, N, T_thresh)
    n32 = NI.restate(k["sig7"], k["deltas"], rays, N, inv_2eps, 1.0, T_thresh, dN)
    w = d32["w"]
    assert not np.isnan(w).any() and np.array_equal(w, n32["w"]) and np.array_equal(d32["live"], n32["live"])
    assert np.array_equal(n32["grad"][:, 4], w) and np.array_equal(n32["grad"][:, 3], -w)
    assert not n32["image"][:, 1:].any()
    # per ray, the sums of the same weights (numpy adds them in another order than either kernel: a few ulp apart)
    per_ray = np.zeros(N)
    np.add.at(per_ray, ids, w.astype(np.float64))
    assert np.abs(-n32["image"][:, 0].astype(np.float64) - per_ray).max() <= 2.0 ** -24 * 201
    assert np.abs(d32["sums"][:, 0].astype(np.float64) - per_ray).max() <= 2.0 ** -24 * 201
    # what the regimes are for (float64 weights)
    w64, T64, tau64 = S.weights(k["sig"], k["deltas"], rays, T_thresh)
    at = np.concatenate([[0], np.cumsum(rays[:, 2])])
    if regime == "thin":
        assert 1e-3 * 0.999 <= tau64.min() and tau64.max() <= 1e-1 * 1.001 and (T64 >= 1e-4).all()
    if regime == "opaque":
        assert 1e3 <= k["sig"].max() <= 1e4
        first_dead = [int(np.argmax(T64[at[i]:at[i + 1]] < 1e-4)) if (T64[at[i]:at[i + 1]] < 1e-4).any() else None
                      for i in range(N)]
        assert first_dead == [None, None, None, 31, None, 64, 21, 101, 151], first_dead
        assert ((w64 == 0) == (T64 < T_thresh)).all() or T_thresh == 0.0
    if regime == "mixed":
        zero = k["sig"] == 0
        assert 0.2 < zero.mean() < 0.6 and (zero[1:] & zero[:-1]).sum() > 50 and (w64[zero] == 0).all()
    margin = np.abs(T64 - 1e-4) / 1e-4
    assert margin.min() >= 1e-3, margin.min()        # float32 and float64 agree on which samples are live
