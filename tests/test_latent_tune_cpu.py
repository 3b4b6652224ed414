"""The RGB refinement stage (render.nerf_type = latent_tune) on the host: the model it builds, the latent -> tune
hand-over of a state dict, the algebra the fused kernels rest on (per-ray decode == per-sample decode) and the RGB form
of the diffusion guidance step, driven with stub modules."""
import types

import torch

from oracle import nerf_oracle as O
from src.latent_nerf.configs.render_config import RenderConfig
from src.latent_nerf.models.nerf_utils import NeRFType
from src.latent_nerf.training import guidance as G
from tests.test_guidance_cpu import _modules


def _net(nerf_type):
    from src.latent_nerf.models.network_grid import NeRFNetwork
    cfg = RenderConfig(grid_size=32, train_h=16, train_w=16, nerf_type=NeRFType(nerf_type))
    return NeRFNetwork(cfg, base_resolution=4, log2_hashmap_size=12)


def test_tuned_model_is_the_latent_field_with_a_decoder():
    net = _net("latent_tune")
    assert net.w3.shape == (5, 64) and net.b3.shape == (5,)
    assert net.img_dims == 3 and not net.latent_mode and net.tuned
    want = torch.tensor(G.LATENT_TO_RGB, dtype=torch.float32).T
    assert net.decoder.shape == (3, 4) and net.decoder.dtype == torch.float32 and torch.equal(net.decoder.detach(), want)
    assert "decoder" in net.state_dict()
    # per-point decode: (z D^T + 1) / 2, clamped
    z = torch.randn(7, 4, generator=torch.Generator().manual_seed(0)) * 6
    rgb = net.decode_points(z)
    assert rgb.shape == (7, 3) and float(rgb.min()) == 0.0 and float(rgb.max()) == 1.0
    assert float((rgb.double() - ((z.double() @ want.double().T + 1) / 2).clamp(0, 1)).abs().max()) <= 4 * 2.0 ** -24
    # the other two types are what they were
    lat, rgb = _net("latent"), _net("rgb")
    assert lat.w3.shape[0] == 5 and lat.img_dims == 4 and lat.latent_mode and not lat.tuned
    assert rgb.w3.shape[0] == 4 and rgb.img_dims == 3 and not rgb.latent_mode and not rgb.tuned
    assert not hasattr(lat, "decoder") and not hasattr(rgb, "decoder")


def test_latent_state_dict_loads_with_only_the_decoder_missing():
    lat, tune = _net("latent"), _net("latent_tune")
    missing, unexpected = tune.load_state_dict(lat.state_dict(), strict=False)
    assert list(missing) == ["decoder"] and list(unexpected) == []
    assert torch.equal(tune.w3.detach(), lat.w3.detach()) and torch.equal(tune.encoder.embeddings.detach(),
                                                                         lat.encoder.embeddings.detach())
    assert torch.equal(tune.decoder.detach(), torch.tensor(G.LATENT_TO_RGB).T)      # the initial decoder stays


def test_get_params_holds_the_decoder_once_at_the_small_learning_rate():
    net = _net("latent_tune")
    groups = net.get_params(1e-3)
    hits = [g for g in groups for p in g["params"] if p is net.decoder]
    assert len(hits) == 1 and hits[0]["lr"] == 1e-3
    flat = [p for g in groups for p in g["params"]]
    assert len(flat) == len({id(p) for p in flat}) == 8                          # table, six MLP tensors, decoder
    assert all(not any(p is getattr(n, "decoder", None) for g in n.get_params(1e-3) for p in g["params"])
               for n in (_net("latent"), _net("rgb")))


def _spans(seed):
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor([0, 1, 2, 17, 64, 65, 130, 300, 5, 33])
    offs = torch.cumsum(counts, 0) - counts
    M, N = int(counts.sum()), counts.numel()
    rays = torch.stack([torch.randperm(N, generator=g), offs, counts], -1).to(torch.int32)
    sigmas = torch.rand(M, generator=g) * 30
    deltas = torch.stack([torch.rand(M, generator=g) * 0.02 + 0.002, torch.rand(M, generator=g) + 0.5], -1)
    z = (torch.rand(M, 4, generator=g) * 2 - 1) * 4
    D = torch.rand(3, 4, generator=g) - 0.5
    bg = torch.rand(N, 3, generator=g)
    return rays, sigmas, deltas, z, D, bg


def test_per_ray_decode_equals_per_sample_decode_in_float64():
    """image = sum_k w_k (D z_k + 1) / 2 + (1 - ws) bg  ==  (D sum_k w_k z_k + ws) / 2 + (1 - ws) bg: compositing is
    linear in the colours.  The oracle's compositing accumulates in float32 whatever it is given, so the float64 weights
    are its formulas restated (tests/latent_tune_reference.py): first the restatement is held against the oracle itself on
    float32 inputs, then the two forms are compared in float64 over those weights, random spans, early stops included."""
    from tests.latent_tune_reference import composite_decode_ref
    for seed in (0, 1, 2, 4):      # (seed 3 puts one T within 4e-5 of the threshold: the margin check below refuses it)
        rays, sigmas, deltas, z, D, bg = _spans(seed)
        ws_o, dp_o, L_o = O.composite_rays_train(sigmas, z, deltas, rays, 1e-4, None)
        _, _, img_o = O.composite_rays_train(sigmas, (z @ D.T + 1) / 2, deltas, rays, 1e-4, bg)
        ref = composite_decode_ref(sigmas.double(), z.double(), deltas.double(), rays, D.double(), bg.double())
        assert ref["margin"] > 1e-3, ref["margin"]           # no kill decision hangs on float32 rounding
        assert float(ws_o.max()) > 0.999                     # the dense spans do stop early ...
        assert not bool(ref["keep_samples"].all()) and bool(ref["keep_samples"].any())
        for got, want in ((ws_o, ref["weights_sum"]), (dp_o, ref["depth"]), (L_o, ref["latent_image"]),
                          (img_o, ref["image"])):
            assert float((got.double() - want).abs().max()) <= 1e-5 * max(1.0, float(want.abs().max()))
        ws, L = ref["weights_sum"], ref["latent_image"]
        per_ray = (L @ D.double().T + ws[:, None]) / 2 + (1 - ws)[:, None] * bg.double()
        assert ref["image"].dtype == torch.float64
        assert float((per_ray - ref["image"]).abs().max()) <= 1e-12


class _AffineVAE(torch.nn.Module):
    """A differentiable stub encoder: 8x average pooling, then a fixed 3 -> 4 channel mix."""
    mix = torch.tensor([[0.5, -0.25, 0.125], [0.75, 0.5, -0.5], [-1.0, 0.25, 0.5], [0.125, 0.125, 0.25]])

    @classmethod
    def from_pretrained(cls, path, subfolder=None, local_files_only=False):
        assert local_files_only
        return cls()

    def encode(self, x):
        z = torch.einsum("oc,bchw->bohw", self.mix, torch.nn.functional.avg_pool2d(x, 8))
        return types.SimpleNamespace(latent_dist=types.SimpleNamespace(sample=lambda: z))


def test_train_step_rgb_pulls_the_sds_gradient_back_through_the_encoder():
    g = G.StableDiffusionGuidance(torch.device("cpu"), "/nonexistent", guidance_scale=7.5, modules=_modules(_AffineVAE))
    tz = g.get_text_embeds("a teddy bear")
    torch.manual_seed(1)
    pred = torch.rand(1, 3, 16, 16)
    torch.manual_seed(5)
    got = g.train_step_rgb(tz, pred)
    assert got.shape == pred.shape and not got.requires_grad and float(got.abs().max()) > 0
    # the same by hand: bilinear to 512 x 512, encode under autograd, SDS gradient on the latents (same random draws),
    # vector-Jacobian product back to the prediction
    x = pred.clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(x, (512, 512), mode="bilinear", align_corners=False)
    lat = g._encode(up)
    assert lat.shape == (1, 4, 64, 64) and lat.requires_grad
    torch.manual_seed(5)
    sds = g.train_step(tz, lat.detach())
    want, = torch.autograd.grad(lat, x, sds)
    assert torch.equal(got, want)
    assert not pred.requires_grad                      # the caller's tensor is left alone
    with torch.no_grad():                              # also callable from a no-grad region (the trainer's step)
        torch.manual_seed(5)
        assert torch.equal(g.train_step_rgb(tz, pred), want)
