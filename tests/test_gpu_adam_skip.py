"""The fused table update with a moment map (csrc/grid.hip FusedUpdate.live): 16-row groups whose moments are all-zero
bits and which get no gradient are left alone.  The result must not change by a bit, and the map must stay what its
invariant says: byte != 0 <=> some exp_avg / exp_avg_sq word of the group has a non-zero bit pattern.

The table is small and chosen for the finishers of pass 2 (4096-row buckets, capacity 32768 samples, so every level MAY
be cut into two slices and is when a bucket gets more than 16384 records):
  level 0  dense, 4920 rows: a full bucket and a partial one (row-wise finisher);
  level 1  dense, 8000 rows from row 4920 (not a multiple of 16): a full bucket whose groups straddle 128-byte lines
           (pair finisher when it gets few records, last slice + row-wise finisher when it gets many), a partial one;
  level 2..4  hashed, 8192 rows each: two full buckets (pair finisher).
Positions come in two small clusters, so most groups are never touched.  Run merging is off (every sample emits its 8
records), `adam_skip` is restored to its default whatever happens."""
import contextlib
import types

import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

L, BASE, DESIRED, LOG2_T = 5, 16, 31, 13
CAP = 32768                       # m_host: plans two slices per bucket
N_A, N_B = 4096, 1024             # samples of the clusters (<= 4096 per step)
LR, B1, B2, EPS = 1e-2, 0.9, 0.99, 1e-15
CONFIGS = [("blocked", 3, True), ("hash", 2, False)]   # (layout, scatter variant: Rec8 / Rec12, bf16 shadow)


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from src.latent_nerf.raymarching import backend as B
    B.get_lib()
    return torch.device("cuda:0")


def _set(key, value):
    from src.latent_nerf.raymarching import backend as B
    B.call("lnerf_set_tuning", key.encode(), int(value))


@contextlib.contextmanager
def settings(adam_skip=1):
    try:
        _set("scatter_compact_max_res", 0)
        _set("adam_skip", adam_skip)
        yield
    finally:
        _set("scatter_compact_max_res", 512)
        _set("adam_skip", 1)


def _levels(gridtype):
    from src.latent_nerf.models import encoding as E
    lv = E.GridLevels(L, 2, BASE, DESIRED, LOG2_T, gridtype=gridtype)
    assert lv.offsets == [0, 4920, 12920, 21112, 29304, 37496], lv.offsets
    return lv


def _group_ids(lv):
    """Row -> its byte of the map, and the number of bytes."""
    gid, b0 = [], 0
    for a, b in zip(lv.offsets[:-1], lv.offsets[1:]):
        r = np.arange(b - a)
        gid.append((b0 + (r >> 12)) * 256 + ((r & 4095) >> 4))
        b0 += -(-(b - a) // 4096)
    return torch.from_numpy(np.concatenate(gid)), b0 * 256


def _invariant(m, v, gid, nbytes):
    """The map the moments imply, on the host, from their bit patterns."""
    bits = (m.cpu().view(torch.int32) != 0).any(-1) | (v.cpu().view(torch.int32) != 0).any(-1)
    return (torch.zeros(nbytes, dtype=torch.int64).index_add_(0, gid, bits.to(torch.int64)) > 0).to(torch.uint8)


def _per_group(flag_rows, gid, nbytes):
    return torch.zeros(nbytes, dtype=torch.int64).index_add_(0, gid, flag_rows.to(torch.int64)) > 0


def _clusters(seed=3):
    """Cluster A around (0.30, 0.30, 0.30) and B around (0.62, 0.55, 0.70) of the unit cube, 0.05 wide: a few cells of
    the finest level each.  World positions at bound 1."""
    g = torch.Generator().manual_seed(seed)
    a = torch.tensor([0.30, 0.30, 0.30]) + 0.05 * torch.rand(N_A, 3, generator=g)
    b = torch.tensor([0.62, 0.55, 0.70]) + 0.05 * torch.rand(N_B, 3, generator=g)
    return a * 2 - 1, b * 2 - 1


def _bucket_records(x_world, lv, gridtype, l):
    """Records per bucket of level l for these samples (8 per sample, none merged), from the oracle's row rule."""
    x01 = (x_world + 1) / 2
    pos = x01 * torch.tensor(lv.scales[l], dtype=torch.float32) + 0.5
    pg = torch.floor(pos).to(torch.int64)
    hs = lv.offsets[l + 1] - lv.offsets[l]
    cnt = torch.zeros(-(-hs // 4096), dtype=torch.int64)
    for c in range(8):
        corner = pg + torch.tensor([c & 1, (c >> 1) & 1, (c >> 2) & 1])
        rows = O.grid_corner_indices(corner, lv.resolutions[l], hs, blocked=gridtype == "blocked")
        cnt += torch.bincount(rows >> 12, minlength=len(cnt))
    return cnt


def _sequence(dev):
    """The five steps: (positions, samples, dfeat is zero)."""
    xa, xb = _clusters()
    return [(xa, False), (xb, False), (xa, True), (xa, False), (torch.cat([xa[:N_A - N_B], xb]), False)]


def _device_inputs(dev, steps, seed=5):
    g = torch.Generator().manual_seed(seed)
    out = []
    for x, zero in steps:
        n = x.shape[0]
        xs = torch.zeros(CAP, 3)
        xs[:n] = x
        d = torch.zeros(L, CAP, 2)
        if not zero:
            d[:, :n] = torch.randn(L, n, 2, generator=g) * 0.1 + 0.2      # no exact zeros: every record is emitted
        out.append((xs.to(dev), d.to(dev), torch.tensor([n], dtype=torch.int32, device=dev)))
    return out


class _State:
    def __init__(self, dev, lv, shadow, seed=11):
        g = torch.Generator().manual_seed(seed)
        self.p = (torch.randn(lv.n_rows, 2, generator=g) * 0.1).to(dev)
        self.p[7, 0] = -0.0                                               # a clean row's -0.0 must survive
        self.m = torch.zeros(lv.n_rows, 2, device=dev)
        self.v = torch.zeros(lv.n_rows, 2, device=dev)
        self.s = self.p.to(torch.bfloat16) if shadow else None            # (the shadow equals bf16(p) from the start)
        self.zero = torch.zeros(lv.n_rows, 2, device=dev)

    def bits(self):
        t = [self.p, self.m, self.v] + ([] if self.s is None else [self.s])
        return [x.detach().cpu().contiguous().view(torch.int32 if x.dtype == torch.float32 else torch.int16) for x in t]


def _same(a, b, what):
    for name, x, y in zip(("table", "exp_avg", "exp_avg_sq", "shadow"), a.bits(), b.bits()):
        bad = (x != y).reshape(x.shape[0], -1).any(-1)
        assert not bool(bad.any()), "%s, %s: %d rows differ, first %s" % (what, name, int(bad.sum()),
                                                                           torch.nonzero(bad).flatten()[:8].tolist())


def _fused_step(lv, variant, st, inp, step, betas=(B1, B2), step_dev=None):
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    x, d, m_dev = inp
    ws = E.scatter_workspace(lv, CAP, x.device)
    B.call("lnerf_grid_encode_backward_adam", *E._grid_args(lv, x, 1.0, CAP, m_dev, CAP, _p(d)), _p(st.zero),
           variant | lv.flag, _p(ws), ws.numel(), _p(st.p), _p(st.m), _p(st.v), _p(st.s), LR, betas[0], betas[1], EPS, step,
           step_dev, 1.0, _stream())
    E.ws_mark_dirty(x.device)


def _unfused_step(lv, variant, st, inp, step):
    """-> the step's gradient (rows x 2), on the host."""
    from src.latent_nerf.models import encoding as E
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    x, d, m_dev = inp
    grad = torch.zeros(lv.n_rows, 2, device=x.device)
    E.grid_encode_backward(x, 1.0, d, lv, CAP, m_dev, CAP, grad, variant=variant)
    B.call("lnerf_adam_step", _p(st.p), _p(grad), B.F32, _p(st.m), _p(st.v), _p(st.s), st.p.numel(), LR, B1, B2, EPS, step,
           None, 1.0, 0, _stream())
    return grad.cpu()


@contextlib.contextmanager
def bound_map(lv, st):
    """A moment map built from st's moments and bound to them; unbound on the way out."""
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    n = int(B.get_lib().lnerf_moment_map_bytes(lv.num_levels, lv.c_offsets))
    mp = torch.full((n,), 77, device=st.m.device, dtype=torch.uint8)      # (the build writes every byte)
    B.call("lnerf_moment_map_build", _p(st.m), _p(st.v), lv.num_levels, 2, lv.c_offsets, _p(mp), n, _stream())
    B.call("lnerf_moment_map_bind", _p(st.m), _p(mp), n)
    try:
        yield mp
    finally:
        B.call("lnerf_moment_map_bind", _p(st.m), None, 0)


@pytest.mark.parametrize("gridtype,variant,shadow", CONFIGS)
def test_five_steps_equal_the_unskipped_and_the_unfused_step(dev, gridtype, variant, shadow):
    """A, B, nothing, A, A + B.  After every step table, moments and shadow equal, bit for bit, the same sequence with
    adam_skip = 0 and the un-fused backward + lnerf_adam_step, and both maps equal the invariant computed on the host.
    The reference run's own gradient and moments say which case each group is in; the test asserts that every case the
    sequence is built for occurs, and that at least half of the groups stay clean throughout."""
    lv = _levels(gridtype)
    gid, nbytes = _group_ids(lv)
    groups = int(torch.zeros(nbytes).index_fill_(0, gid, 1).sum())       # groups that own rows
    steps = _sequence(dev)
    # what the finishers get, from the oracle's row rule: step 1 slices the first bucket of both dense levels (the last
    # slice finishes it row by row), cluster B alone never slices a bucket (8192 records per level)
    for l in (0, 1):
        assert int(_bucket_records(steps[0][0], lv, gridtype, l)[0]) > 16384
    assert all(int(_bucket_records(steps[1][0], lv, gridtype, l).max()) <= 16384 for l in range(L))
    assert int((_bucket_records(steps[1][0], lv, gridtype, 2) > 0).sum()) >= 1
    inputs = _device_inputs(dev, steps)
    on, off, ref = (_State(dev, lv, shadow) for _ in range(3))
    with bound_map(lv, on) as map_on, bound_map(lv, off) as map_off:
        assert int(map_on.max()) == 0 and int(map_off.max()) == 0
        for k, inp in enumerate(inputs, 1):
            before = _invariant(ref.m, ref.v, gid, nbytes).bool()
            with settings():
                grad = _unfused_step(lv, variant, ref, inp, k)
                _fused_step(lv, variant, on, inp, k)
            with settings(adam_skip=0):
                _fused_step(lv, variant, off, inp, k)
            torch.cuda.synchronize()
            _same(on, off, "step %d, skip on against off" % k)
            _same(on, ref, "step %d, fused against un-fused" % k)
            want = _invariant(ref.m, ref.v, gid, nbytes)
            assert torch.equal((map_on.cpu() != 0).to(torch.uint8), want), "step %d: map (skip on)" % k
            assert torch.equal((map_off.cpu() != 0).to(torch.uint8), want), "step %d: map (skip off)" % k
            # coverage, from the reference run
            nz = _per_group((grad != 0).any(-1), gid, nbytes)
            first, idle, skipped = int((~before & nz).sum()), int((before & ~nz).sum()), int((~before & ~nz).sum())
            stepped = int((before & nz).sum())
            print("step %d: groups %d, live+grad %d, live idle %d, first touch %d, skipped %d" %
                  (k, groups, stepped, idle, first, skipped - (nbytes - groups)))
            assert int(want.sum()) * 2 <= groups, "step %d: more than half of the groups are live" % k
            assert skipped - (nbytes - groups) >= groups // 2
            if k == 1:
                assert first > 0 and stepped == 0 and idle == 0
            if k == 2:
                assert first > 0 and idle > 0       # first touches next to live groups that get no gradient
            if k == 3:
                assert first == 0 and stepped == 0 and idle > 0 and float(grad.abs().max()) == 0.0
            if k >= 4:
                assert stepped > 0
        assert float(on.zero.abs().max()) == 0.0
        assert int(on.p.cpu().view(torch.int32)[7, 0]) == -(1 << 31)      # the clean row's -0.0


@pytest.mark.parametrize("gridtype,variant,shadow", CONFIGS)
def test_groups_return_to_clean_when_the_moments_decay_to_zero(dev, gridtype, variant, shadow):
    """beta1 = beta2 = 0: a step with gradient, then one without -- every moment is +0 again and so is every byte."""
    lv = _levels(gridtype)
    gid, nbytes = _group_ids(lv)
    steps = _sequence(dev)
    inputs = _device_inputs(dev, [steps[0], steps[2]])
    on, off = _State(dev, lv, shadow), _State(dev, lv, shadow)
    with bound_map(lv, on) as map_on, bound_map(lv, off) as map_off:
        for k, inp in enumerate(inputs, 1):
            with settings():
                _fused_step(lv, variant, on, inp, k, betas=(0.0, 0.0))
            with settings(adam_skip=0):
                _fused_step(lv, variant, off, inp, k, betas=(0.0, 0.0))
            torch.cuda.synchronize()
            _same(on, off, "step %d" % k)
            assert torch.equal((map_on.cpu() != 0).to(torch.uint8), _invariant(on.m, on.v, gid, nbytes)), k
            assert torch.equal(map_on.cpu() != 0, map_off.cpu() != 0), k
            if k == 1:
                assert int(map_on.max()) == 1
        assert int(map_on.max()) == 0 and int(map_off.max()) == 0
        assert int(on.m.view(torch.int32).abs().max()) == 0 and int(on.v.view(torch.int32).abs().max()) == 0


class _Encoder:
    """What FusedAdam and the armed backward use of a GridEncoder."""

    def __init__(self, lv, table):
        self.levels, self.embeddings = lv, torch.nn.Parameter(table)
        self.fused_update, self.grad_sink, self.scatter_variant = None, None, 3

    def shadow(self):
        return None


def _armed_step(opt, enc, inp):
    from src.latent_nerf.models import encoding as E
    x, d, m_dev = inp
    opt.arm()
    E.run_backward(E.Route("adam", 3 | 0), x, 1.0, d, enc, CAP, m_dev, CAP)
    opt.step()


@pytest.mark.parametrize("how", ["load_state_dict", "unarmed_step"])
def test_the_optimiser_never_lets_a_stale_map_be_read(dev, how):
    """FusedAdam owns the map.  Moments that arrive from outside the fused step -- a checkpoint whose exp_avg is non-zero
    in groups the map holds clean, or an un-armed step through lnerf_adam_step -- are followed by a rebuild: the next armed
    step equals the one with adam_skip = 0, and the map equals the invariant."""
    from src.latent_nerf.training.optimizer import FusedAdam
    lv = _levels("blocked")
    gid, nbytes = _group_ids(lv)
    steps = _sequence(dev)
    inputs = _device_inputs(dev, [steps[0], steps[1]])
    g = torch.Generator().manual_seed(23)
    table = torch.randn(lv.n_rows, 2, generator=g) * 0.1
    foreign_m = torch.randn(lv.n_rows, 2, generator=g) * 0.01             # non-zero everywhere: no group is clean
    foreign_v = torch.rand(lv.n_rows, 2, generator=g) * 1e-3
    got = []
    for skip in (1, 0):
        enc = _Encoder(lv, table.clone().to(dev))
        opt = FusedAdam([{"params": [enc.embeddings], "lr": LR}], betas=(B1, B2), eps=EPS, encoder=enc,
                        fuse_table_update=True)
        fu = opt.fused
        assert fu.map is not None and fu.map.numel() == nbytes and int(fu.map.max()) == 0
        assert "map" not in str(sorted(opt.state_dict()))
        with settings(adam_skip=skip):
            _armed_step(opt, enc, inputs[0])
            torch.cuda.synchronize()
            clean = int((fu.map == 0).sum())
            assert clean * 2 >= nbytes                                    # most groups are clean: a stale map would skip them
            if how == "load_state_dict":
                state = opt.state_dict()
                opt.load_state_dict({"step": state["step"], "exp_avg": [foreign_m.to(dev)], "exp_avg_sq": [foreign_v.to(dev)],
                                     "lr": state["lr"]})
            else:
                grad = (torch.randn(lv.n_rows, 2, generator=torch.Generator().manual_seed(29)) * 0.1).to(dev)
                opt.step(grads={enc.embeddings: grad})                    # every row gets moments
            torch.cuda.synchronize()
            assert torch.equal((fu.map.cpu() != 0).to(torch.uint8), _invariant(fu.exp_avg, fu.exp_avg_sq, gid, nbytes))
            assert int((fu.map == 0).sum()) == nbytes - int(torch.zeros(nbytes).index_fill_(0, gid, 1).sum())
            _armed_step(opt, enc, inputs[1])
            torch.cuda.synchronize()
        assert torch.equal((fu.map.cpu() != 0).to(torch.uint8), _invariant(fu.exp_avg, fu.exp_avg_sq, gid, nbytes))
        got.append(types.SimpleNamespace(p=enc.embeddings.detach(), m=fu.exp_avg, v=fu.exp_avg_sq, s=None, bits=None))
    for name in ("p", "m", "v"):
        a, b = getattr(got[0], name).cpu().view(torch.int32), getattr(got[1], name).cpu().view(torch.int32)
        assert torch.equal(a, b), name
    assert not torch.equal(got[0].p.cpu(), table)


def test_a_captured_step_replays_with_a_valid_map(dev):
    """One armed step captured in a graph and replayed three times, the positions buffer rewritten in between (A, B, A):
    the same bits as three eager calls.  The map a replay reads is the one the replay before left."""
    gridtype, variant, shadow = CONFIGS[0]
    lv = _levels(gridtype)
    gid, nbytes = _group_ids(lv)
    xa, xb = _clusters()
    xb = torch.cat([xb, xb + 1e-3, xb - 1e-3, xb + 2e-3])                 # (as many samples as A: one m_dev for all)
    (xbuf, d, m_dev), = _device_inputs(dev, [(xa, False)])
    frames = [_device_inputs(dev, [(x, False)])[0][0] for x in (xa, xb, xa)]
    eager, graph = _State(dev, lv, shadow), _State(dev, lv, shadow)
    with settings(), bound_map(lv, eager), bound_map(lv, graph) as map_g:
        for f in frames:
            xbuf.copy_(f)
            _fused_step(lv, variant, eager, (xbuf, d, m_dev), 3)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _fused_step(lv, variant, graph, (xbuf, d, m_dev), 3)
        for f in frames:
            xbuf.copy_(f)
            g.replay()
        torch.cuda.synchronize()
        _same(graph, eager, "replayed against eager")
        assert torch.equal((map_g.cpu() != 0).to(torch.uint8), _invariant(graph.m, graph.v, gid, nbytes))
        assert 0 < int((map_g != 0).sum()) * 2 <= nbytes
