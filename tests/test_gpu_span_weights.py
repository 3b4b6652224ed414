"""The four ray-span ops weight samples with ONE compositing weight (csrc/span_walk.h, span_weight), pinned at the op level on
the MI355X: on an input where every finite-difference normal is exactly (-1, 0, 0) and every view direction too
(tests/span_reference.py, weights_case: sigmas7 row 7 i = sigma_i, row 7 i + 1 = 1, the rest 0, eps = 0.5 so inv_2eps = 1,
density_scale = 1, rays_d = (-1, 0, 0)), the ops' outputs are plain sums of the weights and must agree EXACTLY -- no
tolerance.  "Equal" is value equality with no NaN present, i.e. bit equality up to the sign of zero.

Per ray:
  weights_sum of composite_rays_train (C = 3, no background)  ==  orient_ray of shade_fd(..., orient=...)  ==
  -normal_image[:, 0];  normal_image[:, 1:] == 0;
  rays of at most 64 samples:  ray_sums[:, 0] of lnerf_distortion_forward == weights_sum (longer rays chain their chunk sums
  in another order -- lane partials then one wave sum there, one wave sum per chunk here -- and are left out).
Per sample:
  rgbs.grad[:, 0] of image[:, 0].sum() through composite_rays_train (d_rgbs = di w with di = 1)  ==
  sigmas7.grad.view(-1, 7)[:, 4] of normal_image[:, 1].sum() (the y pair of the stencil is (-w, +w) for n = (-1, 0, 0),
  r = 1, inv_2eps = 1: row 3 is checked as its negative).  Both are w_i.

Rays of 0, 1, 2, 63, 64, 65, 128, 130 and 200 samples (ids permuted, the spans tile [0, 653)), three density regimes (thin;
opaque, where T_thresh = 1e-4 cuts inside the first chunk, on the chunk edge and inside the second and third chunk; mixed
with runs of sigma = 0), T_thresh 1e-4 and 0.  The raw entry points write into buffers pre-filled with NaN: an element an
op fails to write fails the comparison.  tests/test_span_weights_cpu.py checks the same identities on the float32
restatements of the references, without a GPU.  The test holds on the library before span_walk.h as well (five copies of
the same arithmetic): it pins what the header now states once."""
import numpy as np
import pytest
import torch

from tests import span_reference as S

pytestmark = pytest.mark.gpu

CASES = [(regime, T) for regime in S.W_REGIMES for T in S.W_T_THRESHES]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _equal(a, b):
    """value equality with no NaN present"""
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any()) and bool((a == b).all())


@pytest.mark.parametrize("regime,T_thresh", CASES)
def test_four_ops_one_weight(dev, regime, T_thresh):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching import raymarching as RM
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    k = S.weights_case(regime)
    N, M = k["N"], k["M"]
    rows, _ = S.span_rows(k["rays"])
    assert np.array_equal(rows, np.arange(M)) and sorted(k["rays"][:, 0].tolist()) == list(range(N))
    assert np.isfinite(k["sig"]).all() and (k["sig"] >= 0).all() and (k["deltas"][:, 0] > 0).all()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    sig, sig7, deltas, rays, rays_d, shade = (t(k[n]) for n in ("sig", "sig7", "deltas", "rays", "rays_d", "shade"))
    ids = rays[:, 0].long()
    inv_2eps = 1.0 / (2.0 * S.W_EPS)
    poison = lambda *shape: torch.full(shape, float("nan"), device=dev, dtype=torch.float32)

    # ---- the four forwards, through the entry points, into poisoned buffers
    rgbs = torch.zeros(M, 3, device=dev)
    ws, depth, image = poison(N), poison(N), poison(N, 3)
    B.call("lnerf_composite_rays_train_forward", _p(sig), _p(rgbs), _p(deltas), _p(rays), N, 3, float(T_thresh), None,
           _p(ws), _p(depth), _p(image), _stream())
    rgbs7 = torch.zeros(7 * M, 3, device=dev)
    sigma_c, colours, orient = poison(M), poison(M, 3), poison(N)
    B.call("lnerf_shade_fd_orient_forward", _p(sig7), _p(rgbs7), 3, _p(rays), N, N, _p(shade), 1, inv_2eps, _p(deltas),
           _p(rays_d), 1.0, float(T_thresh), _p(sigma_c), _p(colours), _p(orient), _stream())
    nimg = poison(N, 3)
    B.call("lnerf_normal_image_forward", _p(sig7), _p(deltas), _p(rays), N, inv_2eps, 1.0, float(T_thresh), _p(nimg),
           _stream())
    dloss, sums = poison(N), poison(N, 2)
    B.call("lnerf_distortion_forward", _p(sig), _p(deltas), _p(rays), N, float(T_thresh), _p(dloss), _p(sums), _stream())
    torch.cuda.synchronize()
    print("%s T_thresh=%g: weights_sum %s" % (regime, T_thresh, ws[ids].cpu().numpy()))
    assert _equal(ws, orient), (ws, orient)
    assert _equal(ws, -nimg[:, 0]), (ws, nimg[:, 0])
    assert _equal(nimg[:, 1:], torch.zeros(N, 2)), nimg
    short = ids[rays[:, 2] <= S.CHUNK]
    assert len(short) == 5
    assert _equal(sums[short, 0], ws[short]), (sums[short, 0], ws[short])
    assert _equal(sigma_c, sig)                      # (the shade forward wrote every row: the spans tile [0, M))

    # ---- the Python surface gives the same forwards, and the per-sample weights through the two backwards
    rgbs_g = torch.zeros(M, 3, device=dev, requires_grad=True)
    ws2, _, image2 = RM.composite_rays_train(sig, rgbs_g, deltas, rays, float(T_thresh), None)
    image2[:, 0].sum().backward()
    _, _, orient2 = RM.shade_fd(sig7, rgbs7, rays, shade, N, S.W_EPS, orient=(deltas, rays_d, 1.0, float(T_thresh), N))
    sig7_g = sig7.clone().requires_grad_()
    nimg2 = RM.normal_image(sig7_g, deltas, rays, N, S.W_EPS, 1.0, float(T_thresh))
    nimg2[:, 1].sum().backward()
    torch.cuda.synchronize()
    assert _equal(ws2, ws) and _equal(orient2, orient) and _equal(nimg2, nimg)
    w_comp = rgbs_g.grad[:, 0]
    stencil = sig7_g.grad.view(-1, 7)
    print("   per-sample weights: %d of %d non-zero, largest %.6g" % (int((w_comp != 0).sum()), M, float(w_comp.max())))
    assert _equal(w_comp, stencil[:, 4]), float((w_comp - stencil[:, 4]).abs().max())
    assert _equal(w_comp, -stencil[:, 3])
    assert _equal(rgbs_g.grad[:, 1:], torch.zeros(M, 2))
    # the weights are weights: in [0, 1], and per ray they sum to the forward's weights_sum up to the order of the sum
    assert float(w_comp.min()) >= 0.0 and float(w_comp.max()) <= 1.0
    per_ray = torch.zeros(N, device=dev, dtype=torch.float64).index_add(0, torch.from_numpy(S.span_rows(k["rays"])[1]).to(dev),
                                                                        w_comp.double())
    assert float((per_ray - ws.double()).abs().max()) <= 2.0 ** -24 * 201
