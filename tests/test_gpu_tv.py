"""The hash table's total-variation regulariser on the MI355X (csrc/grid_tv.hip: lnerf_grid_tv_lines / lnerf_grid_tv_grad,
GridEncoder.grad_total_variation, optim.lambda_tv).  Reference: tests/tv_reference.py (float64, exact integers).

1. Exact inputs (table of integers in [-8, 8], weights powers of two, dtable multiples of 1 / 8: every f32 sum is exact in
   any order): the kernel EQUALS the reference on the five-level table for the three layouts -- explicit lines with the
   lattice borders, a duplicated line on a hashed level, a pre-filled dtable, a zero weight on one level; rows of
   unsampled vertices keep their bits.
2. lines = NULL equals lnerf_grid_tv_lines + explicit lines bit for bit; the drawn lines are the integer restatement; the
   same counter gives the same lines, a ticked step_dev different ones.
3. N(0, 1) table, arbitrary weights: per element |got - ref| <= 16 2^-24 A(row) on dense levels, (16 + k) 2^-24 A(row) on
   a hashed row with k contributions (derived: <= 8 roundings per contribution -- 1 for the differences, 5 adds, the
   weight, the accumulation -- each relative to at most A, doubled; one more per atomic that lands on the row).
4. GridEncoder.grad_total_variation adds into .grad and leaves table and shadow alone.
5. Trainer, one step with a zero guidance: changed rows are a subset of the step-1 lines' rows, and the change is the first
   Adam step of the reference gradient; the same with views_per_step = 2 (the grad_scale slip).
   The feature's specification states the expected change as -lr sign(g_ref) within 2^-20 lr, from "a first Adam step is
   -lr g / (|g| + 1e-15)".
   The two differ by lr eps / |g|, which is above 2^-20 lr for every |g| < 1e-9 -- about a third of the fine levels' rows at
   the default initialisation, whatever the kernel computes.  The test therefore compares with the first Adam step itself,
   -lr g_ref / (|g_ref| + 1e-15), at the stated 2^-20 lr plus that expression's own sensitivity to the bound of g_ref,
   lr eps bound / (|g_ref| + eps)^2: for |g_ref| >> 1e-9 this is the stated check, below it is the stricter one.
6. Captured against eager (six steps, zero guidance): dense rows bit-identical, steps are replayed, the set of changed rows
   grows with every step, hashed rows finite.
7. Default guidance: six steps through the one-graph path, the table differs from the lambda_tv = 0 run, whose optimiser
   still has the fused table update.
8. LNERF_FORCE_DIST with lambda_tv > 0 raises at construction.
Every test prints the figures it asserts on (run with -s)."""
import numpy as np
import pytest
import torch

from tests import tv_reference as TV

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
SMALL = (5, 2, 4, 96, 12)          # num_levels, level_dim, base, desired, log2_T: tv_reference.levels()


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()  # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _levels(layout):
    from src.latent_nerf.models import encoding as E
    lv, ref = E.GridLevels(*SMALL, gridtype=layout), TV.levels(layout)
    assert lv.offsets == ref.offsets and lv.resolutions == ref.resolutions
    return lv, ref


def _is_dense(ref):
    """bool [rows]: the row belongs to a dense level."""
    out = torch.zeros(ref.n_rows, dtype=torch.bool)
    for l, r in enumerate(ref.resolutions):
        if (r + 1) ** 3 <= ref.offsets[l + 1] - ref.offsets[l]:
            out[ref.offsets[l]:ref.offsets[l + 1]] = True
    return out


def _explicit_lines(res, counts, dup_level, seed):
    """Distinct lines per level -- the four corners of the (y, z) plane first, all of them where the count is the whole
    plane -- and on `dup_level` the last line repeats the first."""
    rng = np.random.default_rng(seed)
    out = []
    for l, (r, n) in enumerate(zip(res, counts)):
        s = r + 1
        if n == s * s:
            idx = np.arange(n)
        else:
            corners = np.array([0, r, r * s, r * s + r])
            rest = np.setdiff1d(np.arange(s * s), corners)
            idx = np.concatenate([corners, rng.choice(rest, n - 4, replace=False)])
            if l == dup_level:
                idx[-1] = idx[0]
        out.append(np.stack([idx % s, idx // s], axis=-1))
    return np.concatenate(out).astype(np.int64)


def _exact_case(ref, seed):
    g = torch.Generator().manual_seed(seed)
    table = torch.randint(-8, 9, (ref.n_rows, 2), generator=g).float()
    init = torch.randint(-64, 65, (ref.n_rows, 2), generator=g).float() / 8
    init[::7, 0] = -0.0
    return table, init


@pytest.mark.parametrize("layout", TV.LAYOUTS)
def test_exact_inputs_equal_the_reference_bit_for_bit(dev, layout):
    from src.latent_nerf.models import encoding as E
    lv, ref = _levels(layout)
    counts = [25, 40, 24, 12, 8]                        # level 0 whole; 97-vertex lines on level 4 cross a wave
    offs = [0] + list(np.cumsum(counts))
    lines = _explicit_lines(ref.resolutions, counts, dup_level=4, seed=1)
    for l, r in enumerate(ref.resolutions[1:], 1):
        yz = lines[offs[l]:offs[l + 1]]
        assert {(0, 0), (0, r), (r, 0), (r, r)} <= {tuple(v) for v in yz.tolist()}
    assert np.array_equal(lines[offs[5] - 1], lines[offs[4]])
    weights = [0.5, 0.25, 2.0, 0.0, 0.125]
    table, init = _exact_case(ref, 3)
    want, A, k = TV.tv_grad(table, ref, offs, lines, weights, init)
    assert torch.equal(want.float().double(), want)     # representable: the comparison is exact
    dtable = init.to(dev)
    E.grid_tv_grad(table.to(dev), lv, [int(o) for o in offs], weights, dtable, torch.from_numpy(lines).int().to(dev))
    torch.cuda.synchronize()
    got = dtable.cpu()
    bad = int((got != want.float()).any(-1).sum())
    print("%s: %d rows sampled, %d more than once (max %d), %d rows differ from the reference"
          % (layout, int((k > 0).sum()), int((k > 1).sum()), int(k.max()), bad))
    assert torch.equal(got, want.float())
    untouched = k == 0
    assert torch.equal(_bits(got)[untouched], _bits(init)[untouched])
    assert int(untouched[ref.offsets[3]:ref.offsets[4]].sum()) == ref.offsets[4] - ref.offsets[3]    # the zero weight
    assert int((k > 1).sum()) > 50 and int(untouched.sum()) > 1000
    assert int((got != init).any(-1).sum()) > 1000


@pytest.mark.parametrize("layout", TV.LAYOUTS)
def test_null_lines_equal_drawn_lines(dev, layout):
    from src.latent_nerf.models import encoding as E
    lv, ref = _levels(layout)
    offs = TV.plan(ref.resolutions, 500)
    assert E.grid_tv_plan(lv, 500) == offs and [offs[l + 1] - offs[l] for l in range(5)] == [25, 50, 23, 11, 5]
    seed, weights = 12345, [0.5, 0.25, 2.0, 1.0, 0.125]
    table, init = _exact_case(ref, 4)
    table_d = table.to(dev)
    step_dev = torch.tensor([3, 0], device=dev, dtype=torch.int32)

    def null_path(**kw):
        d = init.to(dev)
        E.grid_tv_grad(table_d, lv, offs, weights, d, None, seed, **kw)
        return d

    def explicit(lines):
        d = init.to(dev)
        E.grid_tv_grad(table_d, lv, offs, weights, d, lines, 999, 999)      # (seed and step are not read)
        return d

    lines3 = E.grid_tv_lines(lv, offs, seed, 777, step_dev, device=dev)     # (the counter wins over `step`)
    assert np.array_equal(lines3.cpu().numpy(), TV.draw_lines(ref.resolutions, offs, seed, 3))
    assert torch.equal(E.grid_tv_lines(lv, offs, seed, 3, None, device=dev), lines3)
    a, b, c = null_path(step=777, step_dev=step_dev), explicit(lines3), null_path(step=3)
    want, _, k = TV.tv_grad(table, ref, offs, lines3.cpu().numpy(), weights, init)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    assert torch.equal(a.cpu(), want.float())
    assert torch.equal(_bits(null_path(step=0, step_dev=step_dev)), _bits(a))      # the same counter: the same lines
    step_dev[0:1] += 1
    lines4 = E.grid_tv_lines(lv, offs, seed, 0, step_dev, device=dev)
    assert np.array_equal(lines4.cpu().numpy(), TV.draw_lines(ref.resolutions, offs, seed, 4))
    assert torch.equal(lines4[:offs[1]], lines3[:offs[1]])                  # level 0 is swept whole
    for l in range(1, 5):
        assert not torch.equal(lines4[offs[l]:offs[l + 1]], lines3[offs[l]:offs[l + 1]]), l
    d = null_path(step=0, step_dev=step_dev)
    assert torch.equal(_bits(d), _bits(explicit(lines4))) and not torch.equal(d, a)
    print("%s: %d rows sampled at step 3 (%d more than once); step 4 changes %d rows' values"
          % (layout, int((k > 0).sum()), int((k > 1).sum()), int((d != a).any(-1).sum())))


@pytest.mark.parametrize("layout", TV.LAYOUTS)
def test_random_table_within_the_derived_bound(dev, layout):
    from src.latent_nerf.models import encoding as E
    lv, ref = _levels(layout)
    offs = TV.plan(ref.resolutions, 2000)
    g = torch.Generator().manual_seed(9)
    table = torch.randn(ref.n_rows, 2, generator=g)
    init = torch.randn(ref.n_rows, 2, generator=g)
    weights = [float(np.float32(w)) for w in (0.3, -1.7, 0.011, 2.3, 0.77)]
    seed, step = 77, 5
    lines = TV.draw_lines(ref.resolutions, offs, seed, step)
    want, A, k = TV.tv_grad(table, ref, offs, lines, weights, init)
    dtable = init.to(dev)
    E.grid_tv_grad(table.to(dev), lv, offs, weights, dtable, None, seed, step)
    torch.cuda.synchronize()
    got = dtable.cpu()
    dense = _is_dense(ref)
    tol = torch.where(dense, torch.full_like(k, 16), 16 + k).double()[:, None] * ULP * A
    err = (got.double() - want).abs()
    ratio = torch.where(tol > 0, err / tol.clamp_min(1e-300), torch.zeros_like(err))
    worst = int(ratio.max(-1).values.argmax())
    print("%s: worst row %d (k = %d, %s): error %.3e at a tolerance of %.3e (ratio %.3f); rows sampled %d, more than once %d"
          % (layout, worst, int(k[worst]), "dense" if dense[worst] else "hashed", float(err[worst].max()),
             float(tol[worst].max()), float(ratio.max()), int((k > 0).sum()), int((k > 1).sum())))
    assert bool((err <= tol).all())
    assert torch.equal(_bits(got)[k == 0], _bits(init)[k == 0])
    assert int((k > 1).sum()) > 100 and float((want - init.double()).abs().max()) > 1e-2
    # dense levels: bitwise reproducible
    again = init.to(dev)
    E.grid_tv_grad(table.to(dev), lv, offs, weights, again, None, seed, step)
    assert torch.equal(_bits(again)[dense], _bits(got)[dense])


def test_encoder_method_adds_into_grad_and_leaves_table_and_shadow_alone(dev):
    from src.latent_nerf.models import encoding as E
    enc = E.GridEncoder(*SMALL, table_dtype=torch.bfloat16, gridtype="blocked").to(dev)
    ref = TV.levels("blocked")
    enc.embeddings.data.normal_(0, 0.1)
    shadow = enc.shadow()
    table0, shadow0, version = enc.embeddings.detach().clone(), shadow.clone(), enc.embeddings._version
    with pytest.raises(RuntimeError, match="embeddings.grad"):
        enc.grad_total_variation(1.0, tv_vertices=500)
    g = torch.Generator().manual_seed(2)
    init = torch.randn(ref.n_rows, 2, generator=g)
    enc.embeddings.grad = init.to(dev)
    out = enc.grad_total_variation(0.75, tv_vertices=500, seed=2, step=4)
    assert out is enc.embeddings.grad
    offs = TV.plan(ref.resolutions, 500)
    weights = [float(np.float32(0.75 / ((offs[l + 1] - offs[l]) * (r + 1)))) for l, r in enumerate(ref.resolutions)]
    want, A, k = TV.tv_grad(table0.cpu(), ref, offs, TV.draw_lines(ref.resolutions, offs, 2, 4), weights, init)
    err = (enc.embeddings.grad.cpu().double() - want).abs()
    tol = (16 + k).double()[:, None] * ULP * A
    print("encoder: worst error / tolerance %.3f over %d sampled rows" % (float((err / tol).max()), int((k > 0).sum())))
    assert bool((err <= tol).all()) and int((k > 0).sum()) > 1000
    assert float((want - init.double()).abs().max()) > 1e-6
    # the device counter and an explicit target
    other = torch.zeros(ref.n_rows, 2, device=dev)
    step_dev = torch.tensor([4, 0], device=dev, dtype=torch.int32)
    enc.grad_total_variation(0.75, tv_vertices=500, seed=2, step_dev=step_dev, grad=other)
    want0, A0, _ = TV.tv_grad(table0.cpu(), ref, offs, TV.draw_lines(ref.resolutions, offs, 2, 4), weights)
    assert bool(((other.cpu().double() - want0).abs() <= (16 + k).double()[:, None] * ULP * A0).all())
    torch.cuda.synchronize()
    assert torch.equal(_bits(enc.embeddings), _bits(table0)) and enc.embeddings._version == version
    assert enc.shadow() is shadow and torch.equal(_bits(shadow.view(torch.int16).int()), _bits(shadow0.view(torch.int16).int()))


# ------------------------------------------------------------------------------ the trainer
class _ZeroGuidance:
    """Stands where the diffusion model stands and returns a zero gradient: the table's gradient is the TV term alone."""

    def get_text_embeds(self, prompt):
        return torch.zeros(1)

    def train_step(self, text_z, latents, dirs=None):
        return torch.zeros_like(latents)


def _cfg(root, name, **over):
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    flat = {"log.exp_name": name, "log.exp_root": str(root), "render.train_h": 32, "render.train_w": 32,
            "render.eval_h": 32, "render.eval_w": 32, "render.grid_size": 64, "optim.iters": 6, "optim.lr": 5e-3,
            "log.save_interval": 1000, "log.eval_size": 1, "log.full_eval_size": 1, "optim.seed": 3,
            "guide.text": "a lego man", "log.quiet": True}
    flat.update(over)
    return apply_overrides(TrainConfig(), flat)


def _table(tr):
    torch.cuda.synchronize()
    return tr.nerf.encoder.embeddings.detach().cpu().clone()


@pytest.fixture(scope="module")
def step_one_reference(dev):
    """The reference gradient of step 1 on the default table, computed for whatever initial table a run hands in; the
    plan, lines and oracle levels are shared."""
    from oracle import nerf_oracle as O
    cache = {}

    def ref_for(tr):
        enc = tr.nerf.encoder
        lv = enc.levels
        if "lv" not in cache:
            cache["lv"] = O.make_grid_levels(lv.num_levels, 2, lv.base_resolution, lv.desired_resolution,
                                             lv.log2_hashmap_size, blocked=lv.gridtype == "blocked",
                                             tiled=lv.gridtype == "tiled")
            cache["offs"] = TV.plan(lv.resolutions, tr.cfg.optim.tv_vertices)
            cache["lines"] = TV.draw_lines(lv.resolutions, cache["offs"], tr.cfg.optim.seed, 1)
            cache["rows"] = TV.sampled_rows(cache["lv"], cache["offs"], cache["lines"])
        assert cache["lv"].offsets == lv.offsets and cache["lv"].resolutions == lv.resolutions
        return cache

    return ref_for


@pytest.fixture(scope="module")
def first_steps(dev, tmp_path_factory):
    """views_per_step -> (trainer, table before, table after, the other parameters before) of ONE step with a zero guidance,
    lambda_sparsity = 0 and lambda_tv = 1; each configuration trained once."""
    from src.latent_nerf.training.trainer import Trainer
    root, runs = tmp_path_factory.mktemp("tv"), {}

    def run(views):
        if views not in runs:
            tr = Trainer(_cfg(root, "v%d" % views, **{"optim.lambda_tv": 1.0, "optim.lambda_sparsity": 0.0,
                                                      "optim.views_per_step": views}), device=dev, guidance=_ZeroGuidance())
            before = _table(tr)
            small0 = [p.detach().clone() for p in tr.nerf.parameters() if p is not tr.nerf.encoder.embeddings]
            tr.train(iters=1)
            runs[views] = (tr, before, _table(tr), small0)
        return runs[views]

    return run


@pytest.mark.parametrize("views", [1, 2])
def test_trainer_first_step_is_the_adam_step_of_the_reference_gradient(dev, first_steps, step_one_reference, views):
    lam, eps = 1.0, 1e-15
    tr, before, after, small0 = first_steps(views)
    lr = float(np.float32(10 * tr.cfg.optim.lr))        # the table's learning rate (NeRFNetwork.get_params)
    assert tr.optimizer.big[0][3] == 10 * tr.cfg.optim.lr and tr.optimizer.big[0][0] is tr.nerf.encoder.embeddings
    assert tr.optimizer.fused is None and tr.nerf.encoder.fused_update is None
    assert tr.train_step == 1 and tr.optimizer.step_no == 1 and len(tr.views) == views
    c = step_one_reference(tr)
    delta = after.double() - before.double()
    changed = torch.nonzero((after != before).any(-1)).squeeze(-1)
    is_sampled = torch.zeros(before.shape[0], dtype=torch.bool)
    is_sampled[c["rows"]] = True
    assert bool(is_sampled[changed].all()) and len(changed) > 0.5 * len(c["rows"])
    lv, offs = c["lv"], c["offs"]
    # the gradient Adam sees: grad_scale * ((lambda / grad_scale) / n_l) = lambda / n_l whatever the number of views
    scale = 1.0 / views
    weights = [float(np.float32((lam / scale) / ((offs[l + 1] - offs[l]) * (r + 1)))) * scale
               for l, r in enumerate(lv.resolutions)]
    g, A, k = TV.tv_grad(before, lv, offs, c["lines"], weights)
    dense = torch.zeros(before.shape[0], dtype=torch.bool)
    dense[:lv.offsets[5]] = True
    assert all((r + 1) ** 3 <= lv.offsets[l + 1] - lv.offsets[l] for l, r in enumerate(lv.resolutions[:5]))
    assert (lv.resolutions[5] + 1) ** 3 > lv.offsets[6] - lv.offsets[5]
    bound = torch.where(dense, torch.full_like(k, 16), 16 + k).double()[:, None] * ULP * A
    sure = g.abs() > bound
    want = -lr * g / (g.abs() + eps)                    # the first Adam step (see the module docstring, 5.)
    tol = 2.0 ** -20 * lr + lr * eps * bound / (g.abs() + eps) ** 2
    err = (delta - want).abs()
    ratio = (err / tol)[sure]
    far = sure & (g.abs() > 1e-8)                       # eps / |g| <= 1e-7: -lr sign(g_ref) at the stated 2^-20 lr
    err_far = (delta + lr * torch.sign(g)).abs()[far]
    print("views %d: %d rows changed of %d sampled; %d elements with |g_ref| above its bound, worst error / tolerance %.3f; "
          "|g_ref| median %.3e, share below 1e-9: %.3f; %d elements with |g_ref| > 1e-8, worst |change + lr sign| %.3e lr"
          % (views, len(changed), len(c["rows"]), int(sure.sum()), float(ratio.max()), float(g.abs()[sure].median()),
             float((g.abs()[sure] < 1e-9).double().mean()), int(far.sum()), float(err_far.max()) / lr))
    assert int(sure.sum()) > 0.9 * 2 * len(c["rows"])
    assert bool((err[sure] <= tol[sure]).all())
    assert int(far.sum()) > 1000 and bool((err_far <= 2.0 ** -20 * lr).all())
    # nothing else moved: the guidance is zero
    for p, q in zip([p for p in tr.nerf.parameters() if p is not tr.nerf.encoder.embeddings], small0):
        assert torch.equal(p.detach(), q)
    if views == 2:      # the same result as with one view
        _, b1, a1, _ = first_steps(1)
        assert torch.equal(_bits(b1), _bits(before))
        single = dense | (k <= 1)                      # one writer per row: no arrival order to depend on
        assert torch.equal(_bits(a1)[single], _bits(after)[single])
        assert bool(((a1.double() - after.double()).abs()[sure] <= 2 * tol[sure]).all())
        assert torch.equal((a1 != b1).any(-1), (after != before).any(-1))


STEPS = (3, 4, 5, 6)       # the table is read back after these steps: the first capture's step and every replay after it


def test_trainer_captured_equals_eager_on_dense_levels_and_draws_fresh_lines(dev, tmp_path):
    from src.latent_nerf.training.trainer import Trainer
    runs = {}
    for graph in (True, False):
        tr = Trainer(_cfg(tmp_path, "g%d" % graph, **{"optim.lambda_tv": 1.0, "optim.lambda_sparsity": 0.0,
                                                      "optim.graph_step": graph}), device=dev, guidance=_ZeroGuidance())
        start = _table(tr)
        n_changed, tabs = [], []
        for it in STEPS:
            tr.train(iters=it)
            tabs.append(_table(tr))
            n_changed.append(int((tabs[-1] != start).any(-1).sum()))
        runs[graph] = (tr, start, tabs, n_changed)
        print("graph_step %s: rows changed after steps %s: %s; %s" % (graph, STEPS, n_changed, tr.graph_stats))
        assert tr.train_step == 6 and all(b > a for a, b in zip(n_changed, n_changed[1:])), n_changed
        assert bool(torch.isfinite(tabs[-1]).all())
    g, e = runs[True], runs[False]
    # (every train() call starts with two eager steps until a captured step exists: steps 1-2 eager, 3-6 replayed)
    assert g[0].graph_stats["replayed_steps"] == 4 and g[0].graph_stats["captures"] == 1
    assert e[0].graph_stats["replayed_steps"] == 0 and e[0].graph_stats["captures"] == 0
    n_dense = g[0].nerf.encoder.levels.offsets[5]
    assert torch.equal(_bits(g[1]), _bits(e[1]))
    for i, it in enumerate(STEPS):
        assert torch.equal(_bits(g[2][i][:n_dense]), _bits(e[2][i][:n_dense])), it
    assert g[3] == e[3]           # the same lines in both forms: the same rows move


def test_trainer_default_guidance_runs_in_one_graph_and_zero_is_the_default_path(dev, tmp_path):
    from src.latent_nerf.training.trainer import Trainer
    tabs = {}
    for lam in (1e-2, 0.0):
        tr = Trainer(_cfg(tmp_path, "d%g" % lam, **{"optim.lambda_tv": lam}), device=dev)
        tr.train()
        tabs[lam] = _table(tr)
        print("lambda_tv %g: %s, whole-step graph %s, fused table update %s"
              % (lam, tr.graph_stats, tr._whole, tr.optimizer.fused is not None))
        assert tr.train_step == 6 and tr._whole and tr.graph_stats["replayed_steps"] > 0
        assert (tr.optimizer.fused is not None) == (lam == 0.0)
        assert bool(torch.isfinite(tabs[lam]).all())
    assert not torch.equal(tabs[1e-2], tabs[0.0])
    assert int((tabs[1e-2] != tabs[0.0]).any(-1).sum()) > 100000


def test_exchange_with_lambda_tv_raises_at_construction(tmp_path, monkeypatch):
    import torch.distributed as dist
    from src.latent_nerf.training import distributed as D
    from src.latent_nerf.training.launch import free_port
    from src.latent_nerf.training.trainer import Trainer
    monkeypatch.setenv("LNERF_FORCE_DIST", "1")
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(free_port()))
    assert not dist.is_initialized()
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        assert D.exchange_active()
        with pytest.raises(ValueError, match="lambda_tv"):
            Trainer(_cfg(tmp_path, "x", **{"optim.lambda_tv": 1e-3}), device=torch.device("cuda:0"), guidance=_ZeroGuidance())
    finally:
        dist.destroy_process_group()
    assert not D.exchange_active()
