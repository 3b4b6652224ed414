"""Every tuning and load path of the gather, the scatter and the bf16 / f32 MLP work splits (lnerf_set_tuning).

Three kinds of check, all on small shapes:
  1. EXACT inputs (tests/exact_grid.py): a hand-set level table, lattice positions and small-integer values on which every
     product and sum is exact in f32.  The kernels must equal the float64 oracle BIT FOR BIT under every setting -- one
     wrongly masked lane of a run sum, one swapped pair, one lost record is a nonzero integer, with no tolerance to hide
     in.  The table has a dense level, a power-of-two hashed one, a one-bucket level that is sliced at the capacity used
     here, and a hashed level whose size (and blocked block count) is NOT a power of two: the `% hsize` / `% nblk` arms.
  2. ORDINARY inputs (random table, samples along rays): every setting against the default run, bit for bit where the
     setting only changes where a value comes from or who adds it, and the default run against the oracle at the
     tolerances tests/test_gpu_parity.py already uses.
  3. The MLP's work splits: per-sample results do not depend on the number of workgroups.

Tuning is process-global and has no getter: every override goes through `tuning(...)`, which restores the WHOLE default
table on exit, and the module's last test re-runs the first test's default launches and compares the bits."""
import contextlib
import types

import pytest
import torch

from oracle import nerf_oracle as O
from tests import exact_grid as X

pytestmark = pytest.mark.gpu

FILL = 123.0          # exact in bf16: rows at and beyond m_dev of a pre-filled output must keep it


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    _restore_defaults()
    return torch.device("cuda:0")


def _set(key, value):
    from src.latent_nerf.raymarching import backend as B
    B.call("lnerf_set_tuning", key.encode(), int(value))


def _restore_defaults():
    for k, v in X.TUNING_DEFAULTS.items():
        _set(k, v)


@contextlib.contextmanager
def tuning(**overrides):
    """Sets the overrides; restores the whole default table whatever happens inside."""
    unknown = set(overrides) - set(X.TUNING_DEFAULTS)
    assert not unknown, unknown
    try:
        for k, v in overrides.items():
            _set(k, v)
        yield
    finally:
        _restore_defaults()


def _where(got, ref, offsets=None, rows_are_samples=False):
    """Describes a bit mismatch: how many entries, per level, the first rows (or samples, with their lane) -- enough to
    locate the level, the rows and the lanes of a run."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if got.shape != ref.shape:
        return "shape %s vs %s" % (tuple(got.shape), tuple(ref.shape))
    bad = (got != ref)
    if bad.dim() > 1:
        bad_rows = bad.reshape(bad.shape[0], -1).any(-1)
    else:
        bad_rows = bad
    idx = torch.nonzero(bad_rows).flatten()
    msg = "%d of %d rows differ, max |diff| %.6g" % (len(idx), bad_rows.numel(), float((got - ref).abs().max()))
    if offsets is not None:
        per = [int(bad_rows[a:b].sum()) for a, b in zip(offsets[:-1], offsets[1:])]
        msg += "; per level %s" % per
    first = idx[:12].tolist()
    if rows_are_samples:
        msg += "; first samples (index, lane) %s" % [(i, i % 64) for i in first]
    else:
        msg += "; first rows %s" % first
    for i in first[:4]:
        msg += "\n  [%d] got %s ref %s" % (i, got[i].flatten().tolist(), ref[i].flatten().tolist())
    return msg


def _exact_device(dev, gridtype):
    """The exact inputs on the device, at capacity 3 M (rows beyond M: zero positions / gradients, never read)."""
    case = X.exact_case(gridtype)
    M, cap = X.EXACT_M, X.EXACT_CAPACITY
    x = torch.zeros(cap, 3)
    x[:M] = case["x"]
    return dict(case=case, levels=X.device_levels(gridtype), x=x.to(dev), table=case["table"].to(dev),
                dfeat=X.level_major(case["grad"], 4, cap).to(dev),
                m_dev=torch.tensor([M], dtype=torch.int32, device=dev), ref=case["dtable"].float().to(dev))


def _ordinary_device(dev, gridtype, table_bf16=False):
    from src.latent_nerf.models import encoding as E
    case = X.ordinary_case(gridtype, table_bf16)
    levels = E.GridLevels(X.SMALL["num_levels"], 2, X.SMALL["base_resolution"], X.SMALL["desired_resolution"],
                          X.SMALL["log2_hashmap_size"], gridtype=gridtype)
    assert levels.offsets == case["lv"].offsets
    M = case["x"].shape[0]
    return dict(case=case, levels=levels, M=M, x=case["x"].to(dev), table=case["table"].to(dev),
                dfeat=X.level_major(case["grad"], 16, M).to(dev))


def _close(a, b, rtol, atol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    bad = err > atol + rtol * b.abs()
    assert not bool(bad.any()), "%s: %d/%d outside tol, max abs err %.3e (ref max %.3e)" % (
        what, int(bad.sum()), bad.numel(), float(err.max()), float(b.abs().max()))


# ------------------------------------------------------------------------------ the module's first and last launches
_first = {}


def _default_launches(dev):
    """One default gather (bf16 table, hash layout) and one default scatter (variant 2) on the ordinary inputs."""
    from src.latent_nerf.models import encoding as E
    d = _ordinary_device(dev, "hash", table_bf16=True)
    feat = E.grid_encode_forward(d["x"], 1.0, d["table"].to(torch.bfloat16), d["levels"], d["M"], None, d["M"])
    dtable = torch.zeros(d["levels"].n_rows, 2, device=dev)
    E.grid_encode_backward(d["x"], 1.0, d["dfeat"], d["levels"], d["M"], None, d["M"], dtable, variant=2)
    return feat, dtable


def test_first_default_launches(dev):
    """Recorded for test_last_default_launches_equal_the_first; the library starts out at the default table (the CPU
    suite checks the table against the sources)."""
    feat, dtable = _default_launches(dev)
    assert float(feat.abs().max()) > 0 and float(dtable.abs().max()) > 0
    _first["feat"], _first["dtable"] = feat.clone(), dtable.clone()


# ------------------------------------------------------------------------------ 1. exact inputs: gather
@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_gather_every_load_path(dev, gridtype, table_dtype):
    """k_grid_forward under gather_pair_loads {0, 1, 2} x gather_dedup_max_res {0, 512}: single loads, the dense pair, the
    hashed aligned pair with its swap (x even; with a bf16 table only reachable at pair_loads = 1), the aligned quad
    (bf16 table, pair_loads = 2), the `% hsize` / `% nblk` rows (single loads), and the run de-duplication -- one lane
    fetching, runs of up to 64 lanes reading it through the LDS crossbar -- on and off.  f32 features equal the float64
    oracle, bf16 features its round-to-nearest cast; rows at and beyond m_dev keep the fill value."""
    from src.latent_nerf.models import encoding as E
    d = _exact_device(dev, gridtype)
    M, cap = X.EXACT_M, X.EXACT_CAPACITY
    ref = d["case"]["feat"]
    ref32, ref16 = ref.float(), ref.float().to(torch.bfloat16)
    assert torch.equal(ref32.double(), ref)
    src = d["table"].to(torch.bfloat16) if table_dtype == "bf16" else d["table"]
    failures = []
    for pl, dd in X.GATHER_SETTINGS:
        with tuning(gather_pair_loads=pl, gather_dedup_max_res=dd):
            for odt, want in ((torch.float32, ref32), (torch.bfloat16, ref16)):
                out = torch.full((4, cap, 2), FILL, device=dev, dtype=odt)
                E.grid_encode_forward(d["x"], 1.0, src, d["levels"], cap, d["m_dev"], cap, out=out)
                got = X.sample_major(out.cpu(), M)
                if not torch.equal(got, want):
                    failures.append("pair_loads=%d dedup=%d out=%s: %s" % (
                        pl, dd, odt, _where(got.float(), want.float(), rows_are_samples=True)))
                if not bool((out[:, M:] == FILL).all()):
                    failures.append("pair_loads=%d dedup=%d out=%s: rows beyond m_dev were written" % (pl, dd, odt))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_position_gradient(dev, gridtype, table_dtype):
    """lnerf_grid_encode_backward_input shares the gather's cell, row and weight definitions (the `% hsize` / `% nblk`
    arms included) and takes no tuning key: on the exact inputs every product is exact (dfeat integers x table
    eighths x weights in 1/64 x scale / 2 = 16), so dxyz equals the float64 autograd of the oracle bit for bit."""
    from src.latent_nerf.models import encoding as E
    d = _exact_device(dev, gridtype)
    M, cap = X.EXACT_M, X.EXACT_CAPACITY
    src = d["table"].to(torch.bfloat16) if table_dtype == "bf16" else d["table"]
    out = torch.full((cap, 3), FILL, device=dev)
    E.grid_encode_backward_input(d["x"], 1.0, src, d["levels"], d["dfeat"], cap, d["m_dev"], cap, out=out)
    want = d["case"]["dxyz"].float()
    assert torch.equal(out[:M].cpu(), want), _where(out[:M], want, rows_are_samples=True)
    assert bool((out[M:] == FILL).all())


# ------------------------------------------------------------------------------ 1. exact inputs: scatter
def _scatter_twice(dev, d, variant):
    """dtable after one call on zeros, and after a second call on top."""
    from src.latent_nerf.models import encoding as E
    cap = X.EXACT_CAPACITY
    dtable = torch.zeros(d["levels"].n_rows, 2, device=dev)
    E.grid_encode_backward(d["x"], 1.0, d["dfeat"], d["levels"], cap, d["m_dev"], cap, dtable, variant=variant)
    once = dtable.clone()
    E.grid_encode_backward(d["x"], 1.0, d["dfeat"], d["levels"], cap, d["m_dev"], cap, dtable, variant=variant)
    return once, dtable


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_scatter_every_setting(dev, gridtype, variant):
    """The bucketed scatter under every key that changes a kernel instantiation or a work split: run merging on (the DPP
    run sums: runs of 1 .. 64 lanes over the 16-lane rows and lane 32, zero stretches inside) and off (then the
    ballot-ranked arm on the levels with <= 32 buckets), zeros binned, 4 / 8 persistent binning workgroups (twelve / six
    items each: the prefetch loop and both counter sets), one workgroup per CU, the 512-thread reduce, level groups.  At
    capacity 3 M the one-bucket level is sliced (tests/test_tuning_inputs_cpu.py asserts the two conditions from the
    reference): the sliced sum and its last-arriver finish run.  dtable on zeros equals the float64 oracle bit for bit --
    8-byte records included: every record and run sum fits their 18 significant bits -- and a second call doubles it."""
    d = _exact_device(dev, gridtype)
    ref, offs = d["ref"], X.EXACT_OFFSETS
    assert torch.equal(ref.double().cpu(), d["case"]["dtable"])
    failures = []
    for name, over in X.SCATTER_SETTINGS:
        with tuning(**over):
            once, twice = _scatter_twice(dev, d, variant)
        if not torch.equal(once, ref):
            failures.append("%s: %s" % (name, _where(once, ref, offs)))
        if not torch.equal(twice, 2 * ref):
            failures.append("%s (second call): %s" % (name, _where(twice, 2 * ref, offs)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_scatter_float_atomics(dev, gridtype, variant):
    """Variants 0 / 1 (global float atomics): on the exact inputs no partial sum, in any order, needs more than the 24
    bits of an f32 (asserted on the reference on the CPU), so they equal the oracle bit for bit as well."""
    d = _exact_device(dev, gridtype)
    once, twice = _scatter_twice(dev, d, variant)
    assert torch.equal(once, d["ref"]), _where(once, d["ref"], X.EXACT_OFFSETS)
    assert torch.equal(twice, 2 * d["ref"]), _where(twice, 2 * d["ref"], X.EXACT_OFFSETS)


FUSED_SETTINGS = [("defaults", {}), ("bin_wgs=4, compact_max_res=0", {"scatter_bin_wgs": 4, "scatter_compact_max_res": 0})]


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_scatter_bf16_wire(dev, gridtype, variant):
    """lnerf_grid_encode_backward_bf16: the wire buffer (stale content before) equals the oracle's gradient rounded to
    bf16, the f32 scratch argument is all zero afterwards."""
    from src.latent_nerf.models import encoding as E
    d = _exact_device(dev, gridtype)
    cap = X.EXACT_CAPACITY
    want = d["ref"].to(torch.bfloat16)
    enc = types.SimpleNamespace(levels=d["levels"], grad_sink=E.GradSink(d["table"]))
    for name, over in FUSED_SETTINGS:
        enc.grad_sink.wire.fill_(7.0)
        with tuning(**over):
            E.grid_encode_backward_bf16(d["x"], 1.0, d["dfeat"], enc, cap, d["m_dev"], cap, variant)
        wire = enc.grad_sink.wire
        assert torch.equal(wire, want), "%s: %s" % (name, _where(wire.float(), want.float(), X.EXACT_OFFSETS))
        assert float(enc.grad_sink.zero.abs().max()) == 0.0, name


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_scatter_fused_adam(dev, gridtype, variant):
    """lnerf_grid_encode_backward_adam == lnerf_grid_encode_backward + lnerf_adam_step: parameters, both moments and the
    bf16 shadow, bit for bit (Adam(0.9, 0.99), eps 1e-15, lr 1e-2, as tests/test_gpu_render.py's
    test_fused_table_update_is_bit_identical); here the gradient both sides apply is the exact one."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    d = _exact_device(dev, gridtype)
    levels, cap = d["levels"], X.EXACT_CAPACITY
    lr, b1, b2, eps, step = 1e-2, 0.9, 0.99, 1e-15, 3
    g = torch.Generator().manual_seed(17)
    p0 = (torch.randn(levels.n_rows, 2, generator=g) * 0.1).to(dev)
    m0 = (torch.randn(levels.n_rows, 2, generator=g) * 0.01).to(dev)
    v0 = (torch.rand(levels.n_rows, 2, generator=g) * 1e-3).to(dev)
    # the separate launches
    grad = torch.zeros(levels.n_rows, 2, device=dev)
    E.grid_encode_backward(d["x"], 1.0, d["dfeat"], levels, cap, d["m_dev"], cap, grad, variant=variant)
    assert torch.equal(grad, d["ref"])
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    sr = torch.zeros(levels.n_rows, 2, device=dev, dtype=torch.bfloat16)
    B.call("lnerf_adam_step", _p(pr), _p(grad), B.F32, _p(mr), _p(vr), _p(sr), pr.numel(), lr, b1, b2, eps, step, None,
           1.0, 0, _stream())
    assert not torch.equal(pr, p0)
    for name, over in FUSED_SETTINGS:
        pf, mf, vf = p0.clone(), m0.clone(), v0.clone()
        sf = torch.zeros(levels.n_rows, 2, device=dev, dtype=torch.bfloat16)
        zero = torch.zeros(levels.n_rows, 2, device=dev)
        ws = E.scatter_workspace(levels, cap, dev)
        with tuning(**over):
            B.call("lnerf_grid_encode_backward_adam", *E._grid_args(levels, d["x"], 1.0, cap, d["m_dev"], cap, _p(d["dfeat"])),
                   _p(zero), variant | levels.flag, _p(ws), ws.numel(), _p(pf), _p(mf), _p(vf), _p(sf), lr, b1, b2, eps,
                   step, None, 1.0, _stream())
        E.ws_mark_dirty(dev)
        for what, a, b in (("table", pf, pr), ("exp_avg", mf, mr), ("exp_avg_sq", vf, vr), ("shadow", sf, sr)):
            assert torch.equal(a, b), "%s, %s: %s" % (name, what, _where(a.float(), b.float(), X.EXACT_OFFSETS))
        assert float(zero.abs().max()) == 0.0, name


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_scatter_buckets_without_records(dev, gridtype, variant):
    """m_dev = EXACT_PER_RAY: only the first ray is scattered.  Eight of the dense level's ten buckets (the partial last
    one among them) and two of the fourth level's receive no record, and the one-bucket level, planned sliced, is summed
    by one workgroup (tests/test_tuning_inputs_cpu.py asserts all of it on the reference).  Every way pass 2 finishes a
    bucket is held to the float64 oracle with the gradient rows >= EXACT_PER_RAY zeroed, bit for bit: the plain add leaves
    an empty bucket alone (and doubles on a second call), the wire form overwrites its stale content with zeros, the
    fused form still owes its rows the Adam step with g = 0 -- equal to the separate launches, and different from the
    initial table."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    d = _exact_device(dev, gridtype)
    d["m_dev"] = torch.tensor([X.EXACT_PER_RAY], dtype=torch.int32, device=dev)
    one = X.first_ray_case(gridtype)
    ref = one["dtable"].float().to(dev)
    assert torch.equal(ref.double().cpu(), one["dtable"])
    levels, cap, offs = d["levels"], X.EXACT_CAPACITY, X.EXACT_OFFSETS
    # plain dtable +=
    once, twice = _scatter_twice(dev, d, variant)
    assert torch.equal(once, ref), _where(once, ref, offs)
    assert torch.equal(twice, 2 * ref), _where(twice, 2 * ref, offs)
    # the wire format: stale content before
    enc = types.SimpleNamespace(levels=levels, grad_sink=E.GradSink(d["table"]))
    enc.grad_sink.wire.fill_(7.0)
    E.grid_encode_backward_bf16(d["x"], 1.0, d["dfeat"], enc, cap, d["m_dev"], cap, variant)
    want = ref.to(torch.bfloat16)
    assert torch.equal(enc.grad_sink.wire, want), _where(enc.grad_sink.wire.float(), want.float(), offs)
    # fused Adam against the separate launches (the moments of test_exact_scatter_fused_adam)
    lr, b1, b2, eps, step = 1e-2, 0.9, 0.99, 1e-15, 3
    g = torch.Generator().manual_seed(17)
    p0 = (torch.randn(levels.n_rows, 2, generator=g) * 0.1).to(dev)
    m0 = (torch.randn(levels.n_rows, 2, generator=g) * 0.01).to(dev)
    v0 = (torch.rand(levels.n_rows, 2, generator=g) * 1e-3).to(dev)
    pr, mr, vr = p0.clone(), m0.clone(), v0.clone()
    sr = torch.zeros(levels.n_rows, 2, device=dev, dtype=torch.bfloat16)
    B.call("lnerf_adam_step", _p(pr), _p(once), B.F32, _p(mr), _p(vr), _p(sr), pr.numel(), lr, b1, b2, eps, step, None,
           1.0, 0, _stream())
    pf, mf, vf = p0.clone(), m0.clone(), v0.clone()
    sf = torch.zeros(levels.n_rows, 2, device=dev, dtype=torch.bfloat16)
    zero = torch.zeros(levels.n_rows, 2, device=dev)
    ws = E.scatter_workspace(levels, cap, dev)
    B.call("lnerf_grid_encode_backward_adam", *E._grid_args(levels, d["x"], 1.0, cap, d["m_dev"], cap, _p(d["dfeat"])),
           _p(zero), variant | levels.flag, _p(ws), ws.numel(), _p(pf), _p(mf), _p(vf), _p(sf), lr, b1, b2, eps, step, None,
           1.0, _stream())
    E.ws_mark_dirty(dev)
    for what, a, b in (("table", pf, pr), ("exp_avg", mf, mr), ("exp_avg_sq", vf, vr), ("shadow", sf, sr)):
        assert torch.equal(a, b), "%s: %s" % (what, _where(a.float(), b.float(), offs))
    spans = [s for level in one["empty"] for s in level]
    assert len(spans) >= 10
    for a, b in spans:      # the g = 0 step really ran: m' = beta1 m everywhere, and the table moved
        assert bool((mf[a:b] != m0[a:b]).all()) and bool((pf[a:b] != p0[a:b]).any()), (a, b)


# ------------------------------------------------------------------------------ 2. ordinary inputs
@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_ordinary_gather_settings_equal_the_default(dev, gridtype, table_dtype):
    """Loads and the lane exchange change where a value comes from, not the arithmetic: every (pair_loads, dedup)
    setting gives the default run's bits; the default run meets the oracle at 1e-4 / 1e-6."""
    from src.latent_nerf.models import encoding as E
    d = _ordinary_device(dev, gridtype, table_dtype == "bf16")
    M = d["M"]
    src = d["table"].to(torch.bfloat16) if table_dtype == "bf16" else d["table"]
    base = E.grid_encode_forward(d["x"], 1.0, src, d["levels"], M, None, M)
    _close(X.sample_major(base, M), d["case"]["feat"], 1e-4, 1e-6, "default features")
    failures = []
    for pl, dd in X.GATHER_SETTINGS:
        with tuning(gather_pair_loads=pl, gather_dedup_max_res=dd):
            got = E.grid_encode_forward(d["x"], 1.0, src, d["levels"], M, None, M)
        if not torch.equal(got, base):
            bad = [l for l in range(16) if not torch.equal(got[l], base[l])]
            failures.append("pair_loads=%d dedup=%d: levels %s; level %d: %s" % (
                pl, dd, bad, bad[0], _where(got[bad[0]], base[bad[0]], rows_are_samples=True)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("variant", [2, 3])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_ordinary_scatter_settings_equal_the_default(dev, gridtype, variant):
    """Every setting that leaves the records alone -- who bins an item, how many threads add, in how many launches, zeros
    binned or not -- gives the default run's bits: the sums are integers.  scatter_compact_max_res = 0 changes the
    records (no merged runs), so it is held against the oracle at the tolerances of test_bucketed_scatter_merges_runs_
    along_rays and must lose no row (variant 2); the combination of all non-default values has ITS records, hence its
    bits."""
    from src.latent_nerf.models import encoding as E
    d = _ordinary_device(dev, gridtype)
    M, levels = d["M"], d["levels"]
    ref = d["case"]["dtable"]
    atol = 2e-4 if variant == 3 else 5e-5

    def run():
        dtable = torch.zeros(levels.n_rows, 2, device=dev)
        E.grid_encode_backward(d["x"], 1.0, d["dfeat"], levels, M, None, M, dtable, variant=variant)
        return dtable

    base = run()
    _close(base, ref, 1e-3, atol, "default dtable")
    unmerged = None
    failures = []
    for name, over in X.SCATTER_SETTINGS[1:]:
        with tuning(**over):
            got = run()
        if "scatter_compact_max_res" in over:
            _close(got, ref, 1e-3, atol, name + " dtable")
            if variant == 2:
                nz_ref = ref.abs().sum(-1) > 0
                assert torch.equal((got.abs().sum(-1) > 0).cpu() | ~nz_ref, torch.ones_like(nz_ref)), name  # no row lost
            if unmerged is None:
                unmerged = got
                continue
            want = unmerged
        else:
            want = base
        if not torch.equal(got, want):
            failures.append("%s: %s" % (name, _where(got, want, levels.offsets)))
    assert unmerged is not None
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------ 3. MLP work splits
class _Ctx:
    """Stands in for the autograd context of network_grid._mlp_forward."""

    def save_for_backward(self, *tensors):
        self.saved = tensors

    def set_materialize_grads(self, flag):
        pass


def _mlp_case(dev, M, out_dim, feat_bf16, bf16_oracle):
    torch.manual_seed(M + 1)
    feat = (torch.randn(M, 32) * 0.5).to(torch.bfloat16).float()
    xyz = (torch.rand(M, 3) * 2 - 1) * 0.8
    p = O.init_mlp_params(seed=M + 1, out_dim=out_dim)
    pr = {k: v.clone().requires_grad_() for k, v in p.items()}
    fr = feat.clone().requires_grad_()
    s_ref, c_ref = O.sigma_latent_mlp(fr, xyz, pr, bf16=bf16_oracle)
    gs, gc = torch.randn(M) * 0.1, torch.randn(M, out_dim - 1)
    ((s_ref * gs).sum() + (c_ref * gc).sum()).backward()
    stride = M + 7
    lm = X.level_major(feat, 16, stride).to(dev)
    if feat_bf16:
        lm = lm.to(torch.bfloat16)
    xg = torch.zeros(stride, 3)
    xg[:M] = xyz
    gsp, gcp = torch.zeros(stride), torch.zeros(stride, out_dim - 1)
    gsp[:M], gcp[:M] = gs, gc
    W = tuple(p[k].to(dev) for k in ("w1", "b1", "w2", "b2", "w3", "b3"))
    return dict(M=M, stride=stride, lm=lm, xyz=xg.to(dev), W=W, s_ref=s_ref.detach(), c_ref=c_ref.detach(),
                dfeat_ref=fr.grad, grads_ref=[pr[k].grad for k in ("w1", "b1", "w2", "b2", "w3", "b3")],
                gs=gsp.to(dev), gc=gcp.to(dev), m_dev=torch.tensor([M], dtype=torch.int32, device=dev))


_wps_agree = {}


@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("M", [129, 5000])
def test_mlp_bf16_forward_work_splits(dev, M, out_dim):
    """k_mlp_forward_bf16<2> and <3> with 1, 3 and 768 persistent workgroups: with one or three workgroups every
    workgroup walks several 128-sample tiles (the next tile's features prefetched), with 768 at most one.  A sample's
    arithmetic does not depend on the split: within one `wps` the outputs are bit-identical across block counts; both
    compilations meet the oracle at 2e-2 / 2e-3.  (Whether the two compilations agree bit for bit is printed, not
    asserted.)  out_dim 4: the non-vectorised store of the latent rows."""
    from src.latent_nerf.models import network_grid as NG
    from src.latent_nerf.raymarching import backend as B
    c = _mlp_case(dev, M, out_dim, True, True)
    outs = {}
    for wps in (2, 3):
        for blocks in (1, 3, 768):
            with tuning(mlp_fwd_wps=wps, mlp_fwd_blocks=blocks):
                sig, rgb = NG._mlp_forward(_Ctx(), c["lm"], c["xyz"], c["W"], c["stride"], c["m_dev"], c["stride"], 5.0,
                                           0.2, B.BF16, None)
            outs[wps, blocks] = (sig[:M].clone(), rgb[:M].clone())
        s0, r0 = outs[wps, 768]
        _close(s0, c["s_ref"], 2e-2, 2e-3, "sigma bf16 wps %d" % wps)
        _close(r0, c["c_ref"], 2e-2, 2e-3, "latent bf16 wps %d" % wps)
        for blocks in (1, 3):
            s, r = outs[wps, blocks]
            assert torch.equal(s, s0), "wps %d, %d blocks, sigma: %s" % (wps, blocks, _where(s, s0, rows_are_samples=True))
            assert torch.equal(r, r0), "wps %d, %d blocks, latent: %s" % (wps, blocks, _where(r, r0, rows_are_samples=True))
    agree = torch.equal(outs[2, 768][0], outs[3, 768][0]) and torch.equal(outs[2, 768][1], outs[3, 768][1])
    _wps_agree[M, out_dim] = agree
    print("mlp_fwd_wps 2 and 3 agree bit for bit at M=%d out_dim=%d: %s" % (M, out_dim, agree))


@pytest.mark.parametrize("precision", ["bf16", "f32"])
@pytest.mark.parametrize("out_dim", [5, 4])
@pytest.mark.parametrize("M", [129, 5000])
def test_mlp_backward_work_splits(dev, M, out_dim, precision):
    """mlp_bwd_blocks 1, 3 and 512: lnerf_mlp_backward_slabs returns min(blocks, tiles) (tiles of 128 samples in bf16, 64
    in f32); dfeat, computed per sample, is bit-identical across the splits; the six parameter gradients (slab sums,
    whose order follows the split) meet the oracle at 3e-2 (bf16) / 1e-4 (f32) of the largest reference entry."""
    from src.latent_nerf.models import network_grid as NG
    from src.latent_nerf.raymarching import backend as B
    bf16 = precision == "bf16"
    tag = B.BF16 if bf16 else B.F32
    c = _mlp_case(dev, M, out_dim, bf16, bf16)
    ctx = _Ctx()
    sig, _ = NG._mlp_forward(ctx, c["lm"], c["xyz"], c["W"], c["stride"], c["m_dev"], c["stride"], 5.0, 0.2, tag, None)
    tiles = -(-c["stride"] // (128 if bf16 else 64))
    rel = 3e-2 if bf16 else 1e-4
    dfeats = {}
    for blocks in (1, 3, 512):
        with tuning(mlp_bwd_blocks=blocks):
            assert B.get_lib().lnerf_mlp_backward_slabs(c["stride"], tag) == min(blocks, tiles)
            grads = [torch.full_like(t, FILL) for t in c["W"]]
            ws, wtag, _ = NG._mlp_backward_workspace(None, tag, out_dim, dev)
            dfeat = NG._mlp_backward(c["lm"], c["xyz"], c["W"], sig, c["stride"], c["m_dev"], c["stride"], 5.0, 0.2,
                                     c["gs"], c["gc"], grads, ws, wtag)
        dfeats[blocks] = X.sample_major(dfeat, M).clone()
        for k, got, want in zip(("w1", "b1", "w2", "b2", "w3", "b3"), grads, c["grads_ref"]):
            scale = float(want.abs().max()) + 1e-30
            err = float((got.cpu().double() - want.double()).abs().max())
            assert err <= rel * scale, "%d blocks, d%s: max abs err %.3e vs scale %.3e" % (blocks, k, err, scale)
    if bf16:   # (dfeat against the oracle as tests/test_gpu_parity.py holds it)
        scale = float(c["dfeat_ref"].abs().max())
        assert float((dfeats[512].cpu().double() - c["dfeat_ref"].double()).abs().max()) <= 3e-2 * scale
    else:
        _close(dfeats[512], c["dfeat_ref"], 1e-3, 1e-5, "dfeat f32")
    for blocks in (1, 3):
        assert torch.equal(dfeats[blocks], dfeats[512]), "%d blocks: %s" % (
            blocks, _where(dfeats[blocks], dfeats[512], rows_are_samples=True))
    assert B.get_lib().lnerf_mlp_backward_slabs(c["stride"], tag) == min(512, tiles)   # the default is back


# ------------------------------------------------------------------------------ the tuning state the module leaves
def test_last_default_launches_equal_the_first(dev):
    """The module leaves the default table behind: the launches of the module's first test, run again, give its bits
    (scatter_compact_max_res, for one, changes the bits of this scatter: asserted here, so that the comparison can
    tell)."""
    if "feat" not in _first:
        pytest.fail("test_first_default_launches did not run before this test")
    feat, dtable = _default_launches(dev)
    assert torch.equal(feat, _first["feat"])
    assert torch.equal(dtable, _first["dtable"]), _where(dtable, _first["dtable"])
    with tuning(scatter_compact_max_res=0):
        other = _default_launches(dev)[1]
    assert not torch.equal(other, dtable)
    assert torch.equal(_default_launches(dev)[1], dtable)
