"""The RGB refinement stage (render.nerf_type = latent_tune) on the GPU: the fused compositing + decode against the
float64 per-sample DEFINITION (tests/latent_tune_reference.py: c_k = (D z_k + 1) / 2, image = sum_k w_k c_k + (1 - ws) bg),
its backward against the chain that existed before it (torch per-sample decode in f32 -> composite_rays_train, C = 3),
the per-pixel epilogue of the inference loop, and the trainer: eager == captured, the latent -> tune hand-over,
checkpoints and mesh export.

Tolerances.  COMPOSITE_TOL(k) = 32 * 2^-24 (k + 1) is the compositing bound of tests/test_gpu_inference.py (sigma dt <= 1.5
here too).  image of a ray with k samples: COMPOSITE_TOL(k) (1 + max_k |c_k|_inf); latent_image / weights_sum / depth:
COMPOSITE_TOL(k) x the largest reference value, as there.  Kill decisions are compared exactly, so the inputs are checked
to keep every reference T 1e-3 (relative) away from T_thresh.  Every test prints the figures it asserts on (run with -s)."""
import math

import pytest
import torch

from oracle import nerf_oracle as O
from tests.latent_tune_reference import composite_decode_ref

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
T_THRESH = 1e-4
SPANS = (0, 1, 2, 63, 64, 65, 130, 300)
SMALL = dict(num_levels=16, base_resolution=4, desired_resolution=128, log2_hashmap_size=12)   # tests/test_gpu_normals.py


def COMPOSITE_TOL(k):
    return 32 * ULP * (k + 1)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


def _inputs(name):
    """Hand-built ray tables (ids permuted).  '1': one ray of 65 samples; '5': five rays (not a multiple of the four
    rays of a block), the dense 300-sample span among them; 'spans': every span length of SPANS; '4099': 4099 rays of
    0..8 samples (the decoder-gradient sum runs over all of them).  sigma dt <= 1.5; the 300-sample span is dense
    enough (sigma up to 400 at dt = 3.4e-3) that T < T_thresh stops it after a few dozen samples."""
    g = torch.Generator().manual_seed({"1": 11, "5": 12, "spans": 13, "4099": 14}[name])
    if name == "1":
        cnts = torch.tensor([65])
    elif name == "5":
        cnts = torch.tensor([0, 1, 64, 130, 300])
    elif name == "spans":
        cnts = torch.tensor(SPANS)
    else:
        cnts = torch.randint(0, 9, (4099,), generator=g)
    N = cnts.numel()
    offs = torch.cumsum(cnts, 0) - cnts
    M = int(cnts.sum())
    rays = torch.stack([torch.randperm(N, generator=g), offs, cnts], -1).to(torch.int32)
    sigmas = torch.rand(M, generator=g) * 20
    for r in (cnts == 300).nonzero().flatten().tolist():
        sigmas[offs[r]:offs[r] + 300] = torch.rand(300, generator=g) * 400
    deltas = torch.stack([torch.full((M,), 3.4e-3), torch.rand(M, generator=g) + 0.3], -1)
    z = (torch.rand(M, 4, generator=g) * 2 - 1) * 4                      # |z| <= 4
    D = torch.rand(3, 4, generator=g) - 0.5                              # decoder entries in [-0.5, 0.5]
    bg = torch.rand(N, 3, generator=g)
    grads = {"image": torch.randn(N, 3, generator=g), "weights_sum": torch.randn(N, generator=g),
             "depth": torch.randn(N, generator=g)}
    return {"rays": rays, "sigmas": sigmas, "deltas": deltas, "z": z, "D": D, "bg": bg, "grads": grads, "N": N, "M": M}


_CACHE = {}


def _case(name, with_bg):
    """Inputs and the float64 reference (forward values and, for the four gradient selections, autograd gradients) of
    one case: computed once, shared by the tests, never modified."""
    key = (name, with_bg)
    if key in _CACHE:
        return _CACHE[key]
    inp = _inputs(name)
    leaves = {k: inp[k].double().requires_grad_() for k in ("sigmas", "z", "D")}
    leaves["bg"] = inp["bg"].double().requires_grad_() if with_bg else None
    ref = composite_decode_ref(leaves["sigmas"], leaves["z"], inp["deltas"].double(), inp["rays"], leaves["D"],
                               leaves["bg"], T_THRESH)
    assert ref["margin"] > 1e-3, (name, ref["margin"])
    ref_grads = {}
    for sel in GRAD_SELECTIONS:
        outs = [ref[k] for k in sel]
        gs = [inp["grads"][k].double() for k in sel]
        wanted = [leaves[k] for k in ("sigmas", "z", "D", "bg") if leaves[k] is not None]
        got = torch.autograd.grad(outs, wanted, gs, retain_graph=True, allow_unused=True)
        got = [torch.zeros_like(w) if g is None else g for g, w in zip(got, wanted)]
        ref_grads[sel] = dict(zip([k for k in ("sigmas", "z", "D", "bg") if leaves[k] is not None], got))
    out = {"inp": inp, "ref": {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ref.items()}, "ref_grads": ref_grads}
    _CACHE[key] = out
    return out


# which outputs receive a gradient: all three, and each one left out (it then arrives as None)
GRAD_SELECTIONS = (("image", "weights_sum", "depth"), ("image", "depth"), ("image", "weights_sum"),
                   ("weights_sum", "depth"))
CASES = [(n, b) for n in ("1", "5", "spans", "4099") for b in (True, False)]


def _run_new(dev, inp, with_bg, sel=None):
    """The fused op on the GPU -> (outputs dict, gradients dict or None)."""
    from src.latent_nerf.raymarching import raymarching as rm
    need = sel is not None
    sg = inp["sigmas"].to(dev).requires_grad_(need)
    z = inp["z"].to(dev).requires_grad_(need)
    D = inp["D"].to(dev).requires_grad_(need)
    bg = inp["bg"].to(dev).requires_grad_(need) if with_bg else None
    ws, depth, image, latent_image = rm.composite_rays_train_decode(sg, z, inp["deltas"].to(dev), inp["rays"].to(dev), D,
                                                                    T_THRESH, bg)
    out = {"weights_sum": ws, "depth": depth, "image": image, "latent_image": latent_image}
    if not need:
        return out, None
    torch.autograd.backward([out[k] for k in sel], [inp["grads"][k].to(dev) for k in sel])
    grads = {"sigmas": sg.grad, "z": z.grad, "D": D.grad}
    if with_bg:
        grads["bg"] = bg.grad
    return out, grads


def _run_chain(dev, inp, with_bg, sel):
    """The chain that existed before the fused op: per-sample decode in torch (f32), composite_rays_train with C = 3."""
    from src.latent_nerf.raymarching import raymarching as rm
    sg = inp["sigmas"].to(dev).requires_grad_()
    z = inp["z"].to(dev).requires_grad_()
    D = inp["D"].to(dev).requires_grad_()
    bg = inp["bg"].to(dev).requires_grad_() if with_bg else None
    c = (z @ D.T + 1.0) / 2.0
    ws, depth, image = rm.composite_rays_train(sg, c, inp["deltas"].to(dev), inp["rays"].to(dev), T_THRESH, bg)
    out = {"weights_sum": ws, "depth": depth, "image": image}
    torch.autograd.backward([out[k] for k in sel], [inp["grads"][k].to(dev) for k in sel])
    grads = {"sigmas": sg.grad, "z": z.grad, "D": D.grad}
    if with_bg:
        grads["bg"] = bg.grad
    return grads


@pytest.mark.parametrize("name,with_bg", CASES)
def test_fused_forward_matches_the_per_sample_definition(dev, name, with_bg):
    """image per ray within COMPOSITE_TOL(k) (1 + max_k |c_k|), latent_image / weights_sum / depth within
    COMPOSITE_TOL(k) x the largest reference value; prints the worst error / tolerance ratio of each."""
    case = _case(name, with_bg)
    inp, ref = case["inp"], case["ref"]
    out, _ = _run_new(dev, inp, with_bg)
    k = ref["count"].double()
    err = (out["image"].cpu().double() - ref["image"]).abs().amax(-1)
    tol = COMPOSITE_TOL(k) * (1.0 + ref["cmax"])
    worst = {"image": float((err / tol).max())}
    assert bool((err <= tol).all()), ("image", float((err - tol).max()))
    for key in ("latent_image", "weights_sum", "depth"):
        e = (out[key].cpu().double() - ref[key]).abs()
        e = e.amax(-1) if e.dim() == 2 else e
        scale = float(ref[key].abs().max())
        t = COMPOSITE_TOL(k) * scale
        worst[key] = float((e / t).max()) if scale > 0 else 0.0
        assert bool((e <= t).all()), (key, float((e - t).max()))
    print("fused forward %s bg=%s: error / tolerance %s" % (name, with_bg, {a: "%.3f" % b for a, b in worst.items()}))
    # an empty span is exactly the background (or exactly (0 + 0) / 2 = 0 without one)
    empty = ref["count"] == 0
    if bool(empty.any()):
        want = inp["bg"][empty] if with_bg else torch.zeros(int(empty.sum()), 3)
        assert torch.equal(out["image"].cpu()[empty], want)
        assert bool((out["latent_image"].cpu()[empty] == 0).all()) and bool((out["weights_sum"].cpu()[empty] == 0).all())


@pytest.mark.parametrize("name,with_bg", CASES)
def test_fused_backward_is_as_close_to_float64_as_the_unfused_chain(dev, name, with_bg):
    """Both the fused op and the chain that existed before it (torch decode per sample, f32 -> composite_rays_train,
    C = 3) against the float64 autograd of the definition: the fused op's max-abs error may be at most twice the chain's
    plus 1e-7 max|ref| (both are f32 sums of the same terms in another order).  Samples behind an early stop get exact
    zeros; the decoder gradient is the same bits on every call.  Prints both errors for every gradient."""
    case = _case(name, with_bg)
    inp, ref = case["inp"], case["ref"]
    dead = ~ref["keep_samples"]
    if name in ("5", "spans"):
        assert int(dead.sum()) > 200            # the dense span did stop early
    for sel in GRAD_SELECTIONS:
        want = case["ref_grads"][sel]
        _, new = _run_new(dev, inp, with_bg, sel)
        old = _run_chain(dev, inp, with_bg, sel)
        for key in want:
            scale = float(want[key].abs().max())
            e_new = float((new[key].cpu().double() - want[key]).abs().max())
            e_old = float((old[key].cpu().double() - want[key]).abs().max())
            print("fused backward %s bg=%s grads of %s: d%s error new %.3e chain %.3e (max|ref| %.3e)"
                  % (name, with_bg, "+".join(sel), key, e_new, e_old, scale))
            assert e_new <= 2 * e_old + 1e-7 * scale, (sel, key, e_new, e_old, scale)
        assert bool((new["sigmas"].cpu()[dead] == 0).all()) and bool((new["z"].cpu()[dead] == 0).all())
        _, again = _run_new(dev, inp, with_bg, sel)
        assert torch.equal(again["D"], new["D"])
        assert torch.equal(again["sigmas"], new["sigmas"]) and torch.equal(again["z"], new["z"])


@pytest.mark.parametrize("N", [1, 4099])
@pytest.mark.parametrize("with_bg", [True, False])
def test_decode_image_matches_the_float64_formula(dev, N, with_bg):
    from src.latent_nerf.raymarching import raymarching as rm
    g = torch.Generator().manual_seed(N)
    L = (torch.rand(N, 4, generator=g) * 2 - 1) * 4
    ws = torch.rand(N, generator=g)
    D = torch.rand(3, 4, generator=g) - 0.5
    bg = torch.rand(N, 3, generator=g) if with_bg else None
    got = rm.decode_image(L.to(dev), ws.to(dev), D.to(dev), None if bg is None else bg.to(dev)).cpu().double()
    want = (L.double() @ D.double().T + ws.double()[:, None]) / 2
    if with_bg:
        want = want + (1 - ws.double())[:, None] * bg.double()
    assert got.shape == (N, 3)
    err, tol = (got - want).abs(), 8 * ULP * (1 + want.abs())
    print("decode_image N=%d bg=%s: worst error / tolerance %.3f" % (N, with_bg, float((err / tol).max())))
    assert bool((err <= tol).all()), float((err - tol).max())


# ------------------------------------------------------------------------------ the model
def _sphere_pair(dev):
    """A latent model and a tuned model over the SMALL encoder that share table, MLP and the sphere occupancy grid."""
    from src.latent_nerf.configs.render_config import RenderConfig
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.models.nerf_utils import NeRFType
    from src.latent_nerf.models.network_grid import NeRFNetwork
    G, HW = 32, 16
    torch.manual_seed(6)
    nets = []
    for kind in ("latent", "latent_tune"):
        cfg = RenderConfig(grid_size=G, train_h=HW, train_w=HW, mlp_precision="f32", table_dtype="f32",
                           nerf_type=NeRFType(kind))
        net = NeRFNetwork(cfg, base_resolution=4, log2_hashmap_size=12)
        net.encoder = E.GridEncoder(table_dtype=torch.float32, scatter_variant=2, **SMALL)
        nets.append(net)
    lat, tune = nets
    lat.encoder.embeddings.data.normal_(0, 0.1)
    missing, unexpected = tune.load_state_dict(lat.state_dict(), strict=False)
    assert list(missing) == ["decoder"] and not unexpected
    grid = O.density_grid_from_function(lambda p: (p.norm(dim=-1) < 0.5).float() * 10.0, G, 1, 1.0)
    bits = O.packbits(grid.reshape(-1), 0.01)
    for net in nets:
        net.to(dev).eval()
        net.density_grid.copy_(grid.to(dev))
        net.density_bitfield.copy_(bits.to(dev))
    f = HW / (2 * math.tan(math.radians(55) / 2))
    ro, rd = O.get_rays(O.pose_from_angles(math.radians(60), 0.3, 1.25), f, f, HW / 2, HW / 2, HW, HW)
    return lat, tune, ro.to(dev), rd.to(dev)


def _handover_check(lat, tune, ro, rd, max_steps=128, scene=True):
    """The tuned model's evaluation image with bg_color = 0 against (D L + ws) / 2, L and ws from the latent model
    that shares its table and MLP.  Both run the same march, field and compositing kernels on the same inputs, so L and
    ws carry the same rounding on both sides and what is left is the decode's own: the bound used is the decode
    tolerance 8 * 2^-24 (1 + |image|) alone (the compositing term COMPOSITE_TOL(k) the bound could also carry is not
    needed, and not granted)."""
    with torch.no_grad():
        a = lat.render(ro, rd, bg_color=0.0, max_steps=max_steps)
        b = tune.render(ro, rd, bg_color=0.0, max_steps=max_steps)
    N = ro.shape[1]
    assert a["image"].shape == (1, N, 4) and b["image"].shape == (1, N, 3)
    assert torch.equal(a["weights_sum"], b["weights_sum"]) and torch.equal(a["depth"], b["depth"])
    L, ws = a["image"][0].cpu().double(), a["weights_sum"][0].cpu().double()
    assert float(ws.max()) > (0.5 if scene else 0.0)
    assert not scene or float(ws.min()) == 0.0                       # the sphere: rays that hit and rays that miss
    D = tune.decoder.detach().cpu().double()
    want = (L @ D.T + ws[:, None]) / 2
    err, tol = (b["image"][0].cpu().double() - want).abs(), 8 * ULP * (1 + want.abs())
    assert bool((err <= tol).all()), float((err - tol).max())
    return float((err / tol).max())


def test_tuned_evaluation_render_is_the_decoded_latent_render(dev):
    lat, tune, ro, rd = _sphere_pair(dev)
    worst = _handover_check(lat, tune, ro, rd)
    print("evaluation hand-over: worst error / tolerance %.3f" % worst)
    # the default background is RGB white: a ray that misses everything is (1, 1, 1)
    with torch.no_grad():
        out = tune.render(ro, rd, max_steps=128)
    miss = out["weights_sum"][0] == 0
    assert int(miss.sum()) > 0 and bool((out["image"][0][miss] == 1.0).all())
    # the uniform sampler (cuda_ray = False) goes through the fused op as well
    tune.cuda_ray = lat.cuda_ray = False
    with torch.no_grad():
        a = lat.render(ro, rd, bg_color=0.0, num_steps=32)
        b = tune.render(ro, rd, bg_color=0.0, num_steps=32)
    L, ws = a["image"][0].double(), a["weights_sum"][0].double()
    want = (L @ tune.decoder.detach().double().T + ws[:, None]) / 2
    assert b["image"].shape == (1, ro.shape[1], 3)
    assert float((b["image"][0].double() - want).abs().max()) <= 8 * ULP * (1 + float(want.abs().max()))
    # normal shading is untouched: 3 channels, no background, the same picture from both models
    tune.cuda_ray = lat.cuda_ray = True
    with torch.no_grad():
        na = lat.render(ro, rd, shading="normal", max_steps=128)
        nb = tune.render(ro, rd, shading="normal", max_steps=128)
    assert torch.equal(na["image"], nb["image"])


# ------------------------------------------------------------------------------ the trainer
def _cfg(tmp_path, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": "t", "log.exp_root": str(tmp_path), "render.train_h": 16, "render.train_w": 16,
            "render.eval_h": 16, "render.eval_w": 16, "render.grid_size": 32, "optim.iters": 12, "optim.lr": 5e-3,
            "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1, "optim.fp16": True,
            "guide.text": "a lego man", "render.nerf_type": "latent_tune", "log.quiet": True}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


def _decoder_state(tr):
    (m, v), = [(e[1], e[2]) for e in tr.optimizer.small if e[0] is tr.nerf.decoder]
    return m, v


@pytest.mark.parametrize("fp16", [True, False])
def test_captured_tuned_steps_match_eager_steps_bit_for_bit(dev, tmp_path, fp16):
    from src.latent_nerf.training.guidance import LATENT_TO_RGB
    from src.latent_nerf.training.trainer import Trainer
    states = []
    for graph in (True, False):
        cfg = _cfg(tmp_path, **{"optim.graph_step": graph, "optim.fp16": fp16, "log.exp_name": "g%d%d" % (graph, fp16)})
        torch.manual_seed(7)
        torch.cuda.manual_seed(7)
        tr = Trainer(cfg, device=dev)
        assert tr.nerf.tuned and tr.nerf.img_dims == 3 and tr.diffusion.targets.shape[1] == 3
        assert sum(e[0] is tr.nerf.decoder for e in tr.optimizer.small) == 1
        table0 = tr.nerf.encoder.embeddings.detach().clone()
        tr.train()
        assert tr.train_step == 12 and tr.optimizer.step_no == 12
        if graph:
            assert tr.graph_stats["captures"] >= 1 and tr.graph_stats["replayed_steps"] >= 8 and tr._whole, tr.graph_stats
        else:
            assert tr.graph_stats["replayed_steps"] == 0 and tr.graph_stats["eager_steps"] == 12
        m, v = _decoder_state(tr)
        states.append({"table": tr.nerf.encoder.embeddings.detach().clone(), "decoder": tr.nerf.decoder.detach().clone(),
                       "decoder_m": m.clone(), "decoder_v": v.clone(),
                       **{k: getattr(tr.nerf, k).detach().clone() for k in ("w1", "b1", "w2", "b2", "w3", "b3")}})
        # the decoder and the table both move
        assert float((states[-1]["table"] - table0).abs().max()) > 0
        init = torch.tensor(LATENT_TO_RGB, device=dev).T
        assert float((states[-1]["decoder"] - init).abs().min()) > 0 and bool(torch.isfinite(states[-1]["decoder"]).all())
    for k in states[0]:
        assert torch.equal(states[0][k], states[1][k]), (k, float((states[0][k] - states[1][k]).abs().max()))


def test_tuned_training_converges_checkpoints_and_exports(dev, tmp_path):
    """Twelve eager steps on ONE fixed view (render.train_pose: the first four and the last four steps then look at the
    same target): mean |image - target| falls.  Then the checkpoint round trip and the mesh export of that model."""
    from src.latent_nerf.training.trainer import Trainer
    cfg = _cfg(tmp_path, **{"optim.graph_step": False, "log.exp_name": "conv"})
    cfg.render.train_pose = (60.0, 20.0, 1.25, 55.0)
    tr = Trainer(cfg, device=dev)
    errs = []
    inner = tr.diffusion.train_step_image

    def recording(image, dirs_dev, H, W, *a, **k):
        out = inner(image, dirs_dev, H, W, *a, **k)
        rows = tr.diffusion._targets_rows[(int(H), int(W))]
        errs.append(float((image.detach() - rows[dirs_dev.long()]).abs().mean()))
        return out

    tr.diffusion.train_step_image = recording
    tr.train()
    tr.diffusion.train_step_image = inner
    assert len(errs) == 12
    first, last = sum(errs[:4]) / 4, sum(errs[-4:]) / 4
    print("tuned training: mean |image - target| first four steps %.4f, last four %.4f" % (first, last))
    assert last < first, (first, last)
    # save_checkpoint(full=True) -> load_checkpoint restores the decoder and its moments exactly
    path = tr.save_checkpoint(full=True)
    tr2 = Trainer(_cfg(tmp_path, **{"optim.graph_step": False, "log.exp_name": "conv2"}), device=dev)
    assert not torch.equal(tr2.nerf.decoder.detach(), tr.nerf.decoder.detach())
    tr2.load_checkpoint(path, model_only=False)
    assert torch.equal(tr2.nerf.decoder.detach(), tr.nerf.decoder.detach())
    for a, b in zip(_decoder_state(tr2), _decoder_state(tr)):
        assert torch.equal(a, b) and float(b.abs().max()) > 0
    assert tr2.optimizer.step_no == tr.optimizer.step_no == 12
    # a latent run's optimiser state has one tensor fewer: refused, as before
    lat = Trainer(_cfg(tmp_path, **{"optim.graph_step": False, "log.exp_name": "lat0", "render.nerf_type": "latent"}),
                  device=dev)
    with pytest.raises(ValueError, match="optimizer state has 8 tensors, expected 7"):
        lat.optimizer.load_state_dict(tr.optimizer.state_dict())
    # export_mesh: vertex colours are the decoder's, at the field's latents
    tr.nerf.eval()
    mesh = tr.nerf.export_mesh(tmp_path / "mesh", resolution=32)
    V = mesh["verts"].shape[0]
    assert V > 0 and mesh["colors"].shape == (V, 3)
    with torch.no_grad():
        _, feats = tr.nerf.field(mesh["verts"].contiguous(), V)
    assert feats.shape == (V, 4)
    assert torch.equal(mesh["colors"], tr.nerf.decode_points(feats))
    assert float(mesh["colors"].min()) >= 0 and float(mesh["colors"].max()) <= 1 and float(mesh["colors"].std()) > 0
    lines = [l.split() for l in open(mesh["path"]) if l.startswith("v ")]
    assert len(lines) == V and len(lines[0]) == 7                       # v x y z r g b
    # the preview of a decoded prediction is taken as [0, 1], one negative value or not
    pred = torch.full((1, 3, 4, 4), 0.5)
    pred[0, 0, 0, 0] = -0.01
    rgb = tr.preview_rgb(pred)
    assert rgb.dtype.name == "uint8" and int(rgb[1, 1, 0]) == 127 and int(rgb[0, 0, 0]) == 0


def test_latent_checkpoint_continues_as_a_tuned_run(dev, tmp_path):
    """A checkpoint written by a 4-step latent run loads into a tuned trainer (optim.ckpt) with `decoder` the only
    missing key; the tuned model then renders the decoded picture of the latent model."""
    from src.latent_nerf.training.guidance import LATENT_TO_RGB
    from src.latent_nerf.training.trainer import Trainer
    lat = Trainer(_cfg(tmp_path, **{"optim.iters": 4, "log.exp_name": "lat", "render.nerf_type": "latent"}), device=dev)
    lat.train()
    path = lat.save_checkpoint(full=True)
    tune = Trainer(_cfg(tmp_path, **{"log.exp_name": "tune", "optim.ckpt": str(path)}), device=dev)
    log = open(tune.exp_path / "log.txt").read()
    assert "checkpoint: missing ['decoder'] unexpected []" in log
    assert torch.equal(tune.nerf.decoder.detach(), torch.tensor(LATENT_TO_RGB, device=dev).T)
    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        assert torch.equal(getattr(tune.nerf, k).detach(), getattr(lat.nerf, k).detach())
    assert torch.equal(tune.nerf.encoder.embeddings.detach(), lat.nerf.encoder.embeddings.detach())
    assert torch.equal(tune.nerf.density_bitfield, lat.nerf.density_bitfield)
    assert tune.train_step == 0                                        # model only: the tuned run starts its own count
    data = tune.dataloaders["val"].collate(0)
    lat.nerf.eval()
    tune.nerf.eval()
    worst = _handover_check(lat.nerf, tune.nerf, data["rays_o"], data["rays_d"], max_steps=1024, scene=False)
    print("trainer hand-over: worst error / tolerance %.3f" % worst)
    # resuming a tuned run from the latent run's optimiser state is refused
    with pytest.raises(ValueError, match="optimizer state has 7 tensors, expected 8"):
        tune.optimizer.load_state_dict(lat.optimizer.state_dict())
    # and the tuned run trains from there (captured steps)
    tune.train(iters=6)
    assert tune.train_step == 6 and bool(torch.isfinite(tune.nerf.decoder).all())
    assert not torch.equal(tune.nerf.decoder.detach(), torch.tensor(LATENT_TO_RGB, device=dev).T)
