"""Adam's bias corrections published once per step (include/lnerf_hip.h, lnerf_adam_constants_bind; csrc/adam_shared.h).

With a record bound to the device step counter, whoever advances the counter leaves  1 - powf(beta, t)  and its
reciprocal for the new step there, and every kernel that reads the counter takes them as data where the record's tag
equals the step it read.  The values are adam_bias_at's own, so `lnerf_set_tuning("adam_consts", 1)` and `0` (every lane
computes them, the record is neither read nor written) must produce the same bits everywhere -- as must a counter that
the host has written behind the record's back (the tag is stale: the cold arm), and a counter with no record at all.

The table is the small one of tests/test_gpu_adam_skip.py, chosen for the finishers of pass 2: partial buckets
(finish_adam), full buckets with few records (RowState) and, in the first step's cluster, first buckets of the dense
levels that are cut into two slices (the last slice to arrive finishes them); 4096 samples or fewer per step; the MLP's
six tensors are stepped from random gradient slabs by the slab blocks of the closing launch and mirrored into the
fragment image.  `adam_consts` is restored to its default whatever happens."""
import contextlib
import ctypes

import pytest
import torch

from tests import exact_mlp as XM
from tests.test_gpu_adam_skip import (B1, B2, CAP, EPS, LR, _device_inputs, _levels, _sequence, _State)

pytestmark = pytest.mark.gpu

OUT_DIM, MLP_LR, VARIANT, GRIDTYPE = 5, 1e-3, 3, "blocked"
SHAPES = {"w1": (64, 32), "b1": (64,), "w2": (64, 64), "b2": (64,), "w3": (OUT_DIM, 64), "b3": (OUT_DIM,)}
FORMS = ["inline_tail", "step_tail", "adam_step_and_tick", "adam_multi_tick"]


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    _lib()
    return torch.device("cuda:0")


def _B():
    from src.latent_nerf.raymarching import backend as B
    return B


def _lib():
    return _B().get_lib()


def _E():
    from src.latent_nerf.models import encoding as E
    return E


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from src.latent_nerf.raymarching.raymarching import _stream as s
    return s()


@contextlib.contextmanager
def settings(adam_consts):
    try:
        _B().call("lnerf_set_tuning", b"scatter_compact_max_res", 0)
        _B().call("lnerf_set_tuning", b"adam_consts", adam_consts)
        yield
    finally:
        _B().call("lnerf_set_tuning", b"scatter_compact_max_res", 512)
        _B().call("lnerf_set_tuning", b"adam_consts", 1)


@pytest.fixture(scope="module")
def shared(dev):
    """What every run reads and none writes: the level table, the five steps' inputs, the MLP's gradient slabs (random: a
    workspace as a deferred backward leaves it), a dense table gradient and the six small gradients."""
    lv = _levels(GRIDTYPE)
    g = torch.Generator().manual_seed(41)
    n_slabs = int(_lib().lnerf_mlp_backward_slabs(CAP, _B().BF16))
    ws_bytes = int(_lib().lnerf_mlp_backward_workspace_bytes(OUT_DIM))
    slabs = torch.randn((ws_bytes - XM.FRAGMENT_BYTES) // 4, generator=g) * 0.05
    return {"lv": lv, "inputs": _device_inputs(dev, _sequence(dev)), "n_slabs": n_slabs, "ws_bytes": ws_bytes,
            "slabs": slabs.to(dev), "table_grad": (torch.randn(lv.n_rows, 2, generator=g) * 0.1).to(dev),
            "small_grads": [(torch.randn(SHAPES[k], generator=g) * 0.1).to(dev) for k in XM.W_NAMES]}


class Rig:
    """One seeded optimiser state: table + moments + shadow (+ moment map), the six MLP tensors + moments, the MLP
    workspace (fragment image, slabs), the counter pair and -- bound unless `bind` is False -- its constants record."""

    def __init__(self, dev, shared, bind=True):
        lv = shared["lv"]
        self.dev, self.sh, self.lv = dev, shared, lv
        self.t = _State(dev, lv, True)
        g = torch.Generator().manual_seed(43)
        self.P = [(torch.randn(SHAPES[k], generator=g) * 0.1).to(dev) for k in XM.W_NAMES]
        self.M = [torch.zeros_like(p) for p in self.P]
        self.V = [torch.zeros_like(p) for p in self.P]
        self.mlp_ws = torch.zeros(shared["ws_bytes"], device=dev, dtype=torch.uint8)
        self.mlp_ws[XM.FRAGMENT_BYTES:].view(torch.float32).copy_(shared["slabs"])
        self.maps = [torch.full((self.P[k].numel() * 2,), -1, device=dev, dtype=torch.int32) for k in (0, 2, 4)]
        _B().call("lnerf_mlp_fragment_maps", OUT_DIM, *[_p(m) for m in self.maps], _stream())
        n = int(_lib().lnerf_moment_map_bytes(lv.num_levels, lv.c_offsets))
        self.map = torch.zeros(n, device=dev, dtype=torch.uint8)              # (the moments start at zero)
        _B().call("lnerf_moment_map_bind", _p(self.t.m), _p(self.map), n)
        self.step_dev = torch.tensor([1, 0], device=dev, dtype=torch.int32)
        self.rec = torch.full((_B().ADAM_CONSTANTS_BYTES // 4,), -1, device=dev, dtype=torch.int32)
        self.bound = bind
        if bind:
            _B().call("lnerf_adam_constants_bind", _p(self.step_dev), B1, B2, _p(self.rec))
        arr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        self.cP, self.cM, self.cV, self.cmaps = arr(self.P), arr(self.M), arr(self.V), arr(self.maps)
        self.cG = arr(shared["small_grads"])
        self.cN = (ctypes.c_int64 * 6)(*[p.numel() for p in self.P])
        self.cLR = (ctypes.c_float * 6)(*([MLP_LR] * 6))

    def close(self):
        _B().call("lnerf_moment_map_bind", _p(self.t.m), None, 0)
        if self.bound:
            _B().call("lnerf_adam_constants_unbind", _p(self.step_dev))
        _E().ws_mark_dirty(self.dev)

    # ---- one optimisation step in each form; the host's step number is wrong on purpose: the counter decides
    def _scatter_args(self, inp):
        x, d, m_dev = inp
        E, lv, t = _E(), self.lv, self.t
        ws = E.scatter_workspace(lv, CAP, self.dev)
        return ws, (*E._grid_args(lv, x, 1.0, CAP, m_dev, CAP, _p(d)), _p(t.zero), VARIANT | lv.flag, _p(ws), ws.numel(),
                    _p(t.p), _p(t.m), _p(t.v), _p(t.s), LR)

    def _tail_args(self):
        return (_p(self.mlp_ws), self.mlp_ws.numel(), _B().BF16, OUT_DIM, self.cP, self.cM, self.cV, MLP_LR, self.cmaps,
                B1, B2, EPS, 1000, _p(self.step_dev), 1.0, _B().TAIL_TICK | _B().TAIL_CLEAR_SCATTER, _stream())

    def step(self, form, inp):
        B, lv, t = _B(), self.lv, self.t
        if form == "inline_tail":          # the scatter whose pass 2 closes the step
            ws, args = self._scatter_args(inp)
            B.call("lnerf_grid_encode_backward_adam_tail", *args, *self._tail_args())
        elif form == "step_tail":          # the fused scatter, then the tail as a launch of its own
            ws, args = self._scatter_args(inp)
            B.call("lnerf_grid_encode_backward_adam", *args, B1, B2, EPS, 1000, _p(self.step_dev), 1.0, _stream())
            B.call("lnerf_step_tail", lv.num_levels, lv.level_dim, lv.c_offsets, lv.c_scales, lv.c_res, CAP,
                   VARIANT | lv.flag, _p(ws), ws.numel(), _p(t.zero), _p(t.p), _p(t.m), _p(t.v), _p(t.s), LR,
                   *self._tail_args())
        elif form == "adam_step_and_tick":  # the streaming table step on a dense gradient, then the one-thread tick
            B.call("lnerf_adam_step", _p(t.p), _p(self.sh["table_grad"]), B.F32, _p(t.m), _p(t.v), _p(t.s), t.p.numel(), LR,
                   B1, B2, EPS, 1000, _p(self.step_dev), 1.0, 0, _stream())
            B.call("lnerf_adam_tick", _p(self.step_dev), _stream())
        else:                               # the multi-tensor launch that also advances the counter (LNERF_ADAM_TICK = 2)
            B.call("lnerf_adam_step_multi_shadow", 6, self.cP, self.cG, self.cM, self.cV, self.cN, self.cLR, B1, B2, EPS,
                   1000, _p(self.step_dev), 1.0, 2, None, None, _stream())
        _E().ws_mark_dirty(self.dev)

    def bits(self):
        """Everything a step may write, as integers (NaN-proof); the record is not part of it."""
        out = dict(zip(("table", "exp_avg", "exp_avg_sq", "shadow"), self.t.bits()))
        for k, p, m, v in zip(XM.W_NAMES, self.P, self.M, self.V):
            out[k], out[k + ".m"], out[k + ".v"] = (x.cpu().view(torch.int32) for x in (p, m, v))
        out["fragments"] = self.mlp_ws[:XM.FRAGMENT_BYTES].cpu()
        out["counter"] = self.step_dev.cpu()
        out["moment map"] = (self.map.cpu() != 0)
        return out

    def record(self):
        r = self.rec.cpu()
        return int(r[4]), r[:4].clone()


def _same(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), "%s: %s differs" % (what, k)


@contextlib.contextmanager
def rigs(dev, shared, binds):
    made = []
    try:
        for bind in binds:
            made.append(Rig(dev, shared, bind))
        yield made
    finally:
        for r in made:
            r.close()
        torch.cuda.synchronize()


@pytest.mark.parametrize("form", FORMS)
def test_four_steps_equal_bit_for_bit(dev, shared, form):
    """Four steps with adam_consts = 1, four with 0 and four on an UNBOUND counter, from the same seeded state: table,
    moments, shadow, the six MLP tensors and their moments, the fragment image, the counter pair and the moment map are
    equal after every step.  With the record in use its tag follows the counter; switched off or unbound it is never
    written."""
    with rigs(dev, shared, (True, True, False)) as (on, off, unbound):
        start = on.bits()
        for k in range(4):
            inp = shared["inputs"][k]
            with settings(1):
                on.step(form, inp)
                unbound.step(form, inp)
            with settings(0):
                off.step(form, inp)
            torch.cuda.synchronize()
            _same(on.bits(), off.bits(), "%s step %d, adam_consts 1 against 0" % (form, k + 1))
            _same(on.bits(), unbound.bits(), "%s step %d, bound against unbound" % (form, k + 1))
            tag, vals = on.record()
            assert tag == k + 2 == int(on.step_dev[0]), (tag, k + 2)
            assert bool(torch.isfinite(vals.view(torch.float32)).all()) and bool((vals.view(torch.float32) > 0).all())
            assert int(on.step_dev[1]) == 0
            assert bool((off.rec == -1).all()) and bool((unbound.rec == -1).all())
        # the form stepped what it is there to step: the table (all but the multi-tensor launch), the MLP (all but the
        # streaming table step), the fragment image (the two tails)
        moved = {k for k, v in on.bits().items() if not torch.equal(v, start[k])}
        assert "counter" in moved
        assert ("table" in moved and "exp_avg_sq" in moved) == (form != "adam_multi_tick"), sorted(moved)
        assert ("w2" in moved and "b3.v" in moved) == (form != "adam_step_and_tick"), sorted(moved)
        assert ("fragments" in moved) == (form in ("inline_tail", "step_tail")), sorted(moved)


@pytest.mark.parametrize("form", FORMS)
def test_a_stale_tag_falls_back_and_the_record_recovers(dev, shared, form):
    """Two steps, then the counter is filled from the host as FusedAdam.load_state_dict does (nothing is published) and
    the record's values are overwritten with NaN: the next step must equal the adam_consts = 0 form bit for bit -- it
    may not have read them --, it publishes again, and the step after it finds tag == counter.  That the record IS what
    a matching tag makes the kernels use shows in the last step: with the values of an earlier step under the current
    tag the results differ."""
    with rigs(dev, shared, (True, True)) as (on, off):
        def both(k):
            with settings(1):
                on.step(form, shared["inputs"][k])
            with settings(0):
                off.step(form, shared["inputs"][k])
            torch.cuda.synchronize()

        both(0)
        early = on.record()[1]                               # the constants of step 2
        both(1)
        for r in (on, off):
            r.step_dev[0:1].fill_(17)
        on.rec[:4] = torch.tensor([float("nan")] * 4).view(torch.int32).to(dev)
        assert on.record()[0] == 3
        both(2)
        _same(on.bits(), off.bits(), "%s: the step behind a host-written counter" % form)
        assert on.record()[0] == 18 == int(on.step_dev[0])
        both(3)
        _same(on.bits(), off.bits(), "%s: the step after it" % form)
        assert on.record()[0] == 19 == int(on.step_dev[0])
        on.rec[:4] = early.to(dev)                           # step 2's corrections under step 19's tag
        both(4)
        a, b = on.bits(), off.bits()
        assert any(not torch.equal(a[k], b[k]) for k in a), "%s: a matching tag's values were not used" % form
        assert torch.equal(a["counter"], b["counter"])
