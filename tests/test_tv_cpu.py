"""The hash table's total-variation regulariser (optim.lambda_tv, GridEncoder.grad_total_variation, lnerf_grid_tv_*) without a
GPU.

1. tests/tv_reference.py: its full-sweep vertex gradient equals float64 autograd of R = sum_l 1 / (2 N_l) sum_edges
   |e(p) - e(q)|^2 on the five-level table (two dense, three hashed levels, hash collisions included) for the three
   layouts, to 1e-15 absolute on a table of N(0, 1) entries.
2. lnerf_grid_tv_plan (host only) equals the Python plan on that table and on the default 16-level table; the default
   budget sweeps levels 0-2 whole, takes 1 489 down to 31 lines on levels 3-15 and ~0.90 M vertices in all.
3. The stratified draw: no stratum is empty, the lines of a level are distinct, inside the lattice, and change with the step.
4. The three entry points refuse bad arguments before any device work; the host wrappers refuse CPU tensors.
5. Config validation; the route of a backward under an optimiser built the way the trainer builds it at lambda_tv > 0."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tv_reference as TV


@pytest.mark.parametrize("layout", TV.LAYOUTS)
def test_full_sweep_gradient_equals_autograd_of_the_energy(layout):
    lv = TV.levels(layout)
    assert lv.resolutions == [4, 9, 20, 44, 96]
    assert [lv.offsets[l + 1] - lv.offsets[l] for l in range(5)] == [128, 1000, 4096, 4096, 4096]
    dense = [(r + 1) ** 3 <= lv.offsets[l + 1] - lv.offsets[l] for l, r in enumerate(lv.resolutions)]
    assert dense == [True, True, False, False, False]
    g = torch.Generator().manual_seed(5)
    table = torch.randn(lv.n_rows, 2, generator=g, dtype=torch.float64)
    lam = 0.75
    leaf = table.clone().requires_grad_()
    TV.energy(leaf, lv, lam).backward()
    offs = TV.full_plan(lv.resolutions)
    weights = [lam / (r + 1) ** 3 for r in lv.resolutions]
    got, A, k = TV.tv_grad(table, lv, offs, TV.all_lines(lv.resolutions), weights)
    err = float((got - leaf.grad).abs().max())
    print("%s: max |vertex gradient - autograd| = %.3e (largest entry %.3e); rows with more than one contribution: %d"
          % (layout, err, float(leaf.grad.abs().max()), int((k > 1).sum())))
    assert err <= 1e-15 and float(leaf.grad.abs().max()) > 1e-3
    assert int((k > 1).sum()) > 1000                                 # collisions are in the comparison
    assert int(k.sum()) == sum((r + 1) ** 3 for r in lv.resolutions)
    assert bool((A >= got.abs() * (1 - 1e-12)).all())


def _c_plan(res, budget):
    from src.latent_nerf.raymarching import backend as B
    out = (ctypes.c_int32 * (len(res) + 1))()
    B.call("lnerf_grid_tv_plan", len(res), (ctypes.c_int32 * len(res))(*res), int(budget), out)
    return list(out)


def test_plan_equals_the_python_plan(built_lib):
    from src.latent_nerf.models import encoding as E
    small = TV.levels("hash").resolutions
    default = E.GridLevels()
    assert default.resolutions == __import__("oracle.nerf_oracle", fromlist=["x"]).make_grid_levels().resolutions
    for res in (small, default.resolutions):
        for budget in (1, 7, 97, 500, 4096, 65536, 1 << 20, 1 << 30):
            assert _c_plan(res, budget) == TV.plan(res, budget), (res, budget)
    assert E.grid_tv_plan(default, 65536) == TV.plan(default.resolutions, 65536)
    assert E.grid_tv_plan(E.GridLevels(5, 2, 4, 96, 12), 500) == TV.plan(small, 500)
    # the default budget on the default table
    offs = TV.plan(default.resolutions, 65536)
    n = [offs[l + 1] - offs[l] for l in range(16)]
    whole = [n[l] == (r + 1) ** 2 for l, r in enumerate(default.resolutions)]
    assert whole == [True] * 3 + [False] * 13
    assert n[3] == 1489 and n[15] == 31
    total = sum(k * (r + 1) for k, r in zip(n, default.resolutions))
    print("default plan: lines %s, %d vertices per step" % (n, total))
    assert 0.88e6 < total < 0.92e6
    # a budget below one line still takes one line; a huge one sweeps everything
    assert TV.plan(small, 1) == [0, 1, 2, 3, 4, 5]
    assert TV.plan(small, 1 << 30) == TV.full_plan(small)


@pytest.mark.parametrize("budget", [97, 500, 65536])
def test_strata_are_non_empty_and_lines_are_distinct(budget):
    for res in (TV.levels("hash").resolutions, [16, 43, 2048]):
        offs = TV.plan(res, budget)
        a = TV.draw_lines(res, offs, 3, 1)          # (asserts hi > lo for every stratum)
        b = TV.draw_lines(res, offs, 3, 2)
        for l, r in enumerate(res):
            yz = a[offs[l]:offs[l + 1]]
            assert yz.min() >= 0 and yz.max() <= r
            idx = yz[:, 0] + yz[:, 1] * (r + 1)
            assert len(np.unique(idx)) == len(idx) and bool((np.diff(idx) > 0).all())
            n, S = len(idx), (r + 1) ** 2
            j = np.arange(n)
            assert bool((idx >= j * S // n).all()) and bool((idx < (j + 1) * S // n).all())
            if n == S:
                assert np.array_equal(idx, j) and np.array_equal(b[offs[l]:offs[l + 1]], yz)
            elif n >= 8:
                assert not np.array_equal(b[offs[l]:offs[l + 1]], yz)


def test_entry_points_refuse_bad_arguments(built_lib):
    """Argument validation needs no device: every refusal comes back before any launch."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    assert len(B._SIGNATURES["lnerf_grid_tv_plan"]) == 4 and len(B._SIGNATURES["lnerf_grid_tv_lines"]) == 8
    assert len(B._SIGNATURES["lnerf_grid_tv_grad"]) == 14
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7
    assert {"lnerf_grid_tv_plan", "lnerf_grid_tv_lines", "lnerf_grid_tv_grad"} <= set(B.header_symbols())
    L = 5
    lv = E.GridLevels(L, 2, 4, 96, 12)
    res, offsets = lv.c_res, lv.c_offsets
    I32 = lambda *v: (ctypes.c_int32 * len(v))(*v)
    F32 = lambda *v: (ctypes.c_float * len(v))(*v)
    plan = I32(*TV.plan(lv.resolutions, 500))
    out = I32(*([0] * (L + 1)))
    w = F32(*([1.0] * L))
    fake = ctypes.c_void_p(256)            # a non-null "device pointer": never dereferenced, every call below is refused

    def refused(name, match, *args):
        with pytest.raises(B.LnerfError, match=match):
            B.call(name, *args)

    # plan
    refused("lnerf_grid_tv_plan", "null", L, None, 500, out)
    refused("lnerf_grid_tv_plan", "null", L, res, 500, None)
    refused("lnerf_grid_tv_plan", "budget", L, res, 0, out)
    refused("lnerf_grid_tv_plan", "budget", L, res, -5, out)
    refused("lnerf_grid_tv_plan", "budget", L, res, (1 << 30) + 1, out)
    refused("lnerf_grid_tv_plan", "num_levels", 0, res, 500, out)
    refused("lnerf_grid_tv_plan", "num_levels", 33, res, 500, out)
    refused("lnerf_grid_tv_plan", "resolution", L, I32(4, 9, 0, 44, 96), 500, out)
    # lines
    refused("lnerf_grid_tv_lines", "null", L, res, plan, 0, 0, None, None, None)
    refused("lnerf_grid_tv_lines", "null", L, None, plan, 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", "null", L, res, None, 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", "increase", L, res, I32(0, 5, 5, 8, 9, 10), 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", "increase", L, res, I32(0, 5, 4, 8, 9, 10), 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", "lattice only", L, res, I32(0, 26, 27, 28, 29, 30), 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", r"line_offsets_host\[0\]", L, res, I32(1, 2, 3, 4, 5, 6), 0, 0, None, fake, None)
    refused("lnerf_grid_tv_lines", "num_levels", 0, res, plan, 0, 0, None, fake, None)
    # grad
    G = lambda **kw: [kw.get(k, d) for k, d in (("table", fake), ("L", L), ("dim", 2), ("offsets", offsets), ("res", res),
                                                ("flags", 0), ("plan", plan), ("lines", None), ("seed", 0), ("step", 0),
                                                ("step_dev", None), ("w", w), ("dtable", fake), ("stream", None))]
    refused("lnerf_grid_tv_grad", "null", *G(table=None))
    refused("lnerf_grid_tv_grad", "null", *G(dtable=None))
    refused("lnerf_grid_tv_grad", "null", *G(offsets=None))
    refused("lnerf_grid_tv_grad", "null", *G(res=None))
    refused("lnerf_grid_tv_grad", "null", *G(plan=None))
    refused("lnerf_grid_tv_grad", "null", *G(w=None))
    refused("lnerf_grid_tv_grad", "exclude each other", *G(flags=B.GRID_BLOCKED | B.GRID_TILED))
    refused("lnerf_grid_tv_grad", "unknown layout flag", *G(flags=1))
    refused("lnerf_grid_tv_grad", "level_dim", *G(dim=4))
    refused("lnerf_grid_tv_grad", "num_levels", *G(L=0))
    refused("lnerf_grid_tv_grad", "increase", *G(offsets=I32(0, 128, 128, 5224, 9320, 13416)))
    refused("lnerf_grid_tv_grad", "increase", *G(offsets=I32(0, 128, 1128, 1000, 9320, 13416)))
    refused("lnerf_grid_tv_grad", "increase", *G(plan=I32(0, 5, 5, 8, 9, 10)))
    refused("lnerf_grid_tv_grad", "not finite", *G(w=F32(1.0, float("nan"), 1.0, 1.0, 1.0)))
    refused("lnerf_grid_tv_grad", "not finite", *G(w=F32(1.0, 1.0, float("inf"), 1.0, 1.0)))
    refused("lnerf_grid_tv_grad", ">= 16 rows", *G(flags=B.GRID_BLOCKED, offsets=I32(0, 8, 1008, 5104, 9200, 13296)))
    # the Python side: a budget < 1, CPU tensors
    with pytest.raises(B.LnerfError, match="budget"):
        E.grid_tv_plan(lv, 0)
    enc = E.GridEncoder(L, 2, 4, 96, 12)
    with pytest.raises(RuntimeError, match="embeddings.grad"):
        enc.grad_total_variation(1.0)
    with pytest.raises(ValueError, match="GPU"):
        enc.grad_total_variation(1.0, grad=torch.zeros(lv.n_rows, 2))
    enc.embeddings.grad = torch.zeros(lv.n_rows, 2)
    with pytest.raises(ValueError, match="GPU"):
        enc.grad_total_variation(1.0, tv_vertices=500)
    with pytest.raises(ValueError, match="GPU"):
        E.grid_tv_lines(lv, TV.plan(lv.resolutions, 500), device="cpu")
    assert float(enc.embeddings.grad.abs().sum()) == 0


def test_config_fields_and_validation():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    assert TrainConfig().optim.lambda_tv == 0.0 and TrainConfig().optim.tv_vertices == 65536
    cfg = apply_overrides(TrainConfig(), {"optim.lambda_tv": 1e-3, "optim.tv_vertices": 4096})
    assert cfg.optim.lambda_tv == 1e-3 and cfg.optim.tv_vertices == 4096
    for bad in (-1e-3, float("nan")):
        with pytest.raises(ValueError, match="lambda_tv"):
            apply_overrides(TrainConfig(), {"optim.lambda_tv": bad})
    for bad in (0, -4):
        with pytest.raises(ValueError, match="tv_vertices"):
            apply_overrides(TrainConfig(), {"optim.tv_vertices": bad})


def test_the_trainers_optimiser_at_lambda_tv_takes_the_plain_route():
    """Trainer.__init__ builds FusedAdam(fuse_table_update=False) when lambda_tv > 0: an armed step's backward then takes
    the `plain` route -- the dense f32 gradient the term is added to -- where the default build takes a fused one."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.training.optimizer import FusedAdam
    mlp = [torch.zeros(64, 32), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(5, 64), torch.zeros(5)]
    names = {}
    for fuse in (False, True):
        enc = E.GridEncoder(5, 2, 4, 96, 12)
        opt = FusedAdam([{"params": [enc.embeddings], "lr": 1e-3}], betas=(0.9, 0.99), eps=1e-15, encoder=enc,
                        fuse_table_update=fuse, capturable=True)
        opt.arm()
        names[fuse] = E.backward_route(enc.fused_update, enc.grad_sink, enc.scatter_variant, 1000, mlp, True, True).name
        assert (opt.fused is None) == (not fuse)
    assert names == {False: "plain", True: "adam"}
