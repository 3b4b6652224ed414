"""The route of a backward through the hash-grid encoder (encoding.backward_route: which scatter delivers the table
gradient, what the fused MLP launch in front of it owes) and the bookkeeping run_backward does for each route, on stub
state -- no GPU."""
from types import SimpleNamespace as NS

import pytest
import torch

from src.latent_nerf.models import encoding as E
from src.latent_nerf.raymarching import backend as B

C = B.SCATTER_CLEARED
MLP = [torch.zeros(64, 32), torch.zeros(64), torch.zeros(64, 64), torch.zeros(64), torch.zeros(5, 64), torch.zeros(5)]
GROUPS = [(0, 8), (8, 16)]


def _fu(armed=True, tail=False, inline=False):
    return NS(armed=armed, tail=tail, inline_tail=inline)


def _bucket(tensors=MLP):
    """GradSink.small_direct of a flat bucket that holds `tensors`: {data_ptr: view}."""
    flat = torch.zeros(sum(t.numel() for t in tensors))
    out, o = {}, 0
    for t in tensors:
        out[t.data_ptr()] = flat[o:o + t.numel()].view(t.shape)
        o += t.numel()
    return out


BUCKET = _bucket()
WRONG_SHAPE = {**BUCKET, MLP[5].data_ptr(): torch.zeros(6)}
MISSING = {k: v for k, v in BUCKET.items() if k != MLP[0].data_ptr()}

# (fu, sink, variant, m_host, mlp, own_ws, ws_clean) -> (route, scatter variant, MLP launch clears, bucket views)
ROWS = {
    "plain": ((None, None, 3, 1000, MLP, True, False), ("plain", 3 | C, True, False)),
    "wire": ((None, NS(groups=None, small_direct=None), 3, 1000, MLP, True, False), ("wire", 3 | C, True, False)),
    "bin": ((None, NS(groups=GROUPS, small_direct=None), 3, 1000, MLP, True, False), ("bin", 3 | C, True, False)),
    "bin, bucket views": ((None, NS(groups=GROUPS, small_direct=BUCKET), 3, 1000, MLP, True, False),
                          ("bin", 3 | C, True, True)),
    "bin, a view of the wrong shape": ((None, NS(groups=GROUPS, small_direct=WRONG_SHAPE), 3, 1000, MLP, True, False),
                                       ("bin", 3 | C, True, False)),
    "bin, a tensor without a view": ((None, NS(groups=GROUPS, small_direct=MISSING), 3, 1000, MLP, True, False),
                                     ("bin", 3 | C, True, False)),
    "adam": ((_fu(), None, 3, 1000, MLP, True, False), ("adam", 3 | C, True, False)),
    "adam_tail": ((_fu(tail=True), None, 3, 1000, MLP, True, False), ("adam_tail", 3, False, False)),
    "adam_closing_tail": ((_fu(tail=True, inline=True), None, 3, 1000, MLP, True, False),
                          ("adam_closing_tail", 3, False, False)),
    # precedence and the conditions of the tail routes
    "unarmed fused update": ((_fu(armed=False), None, 3, 1000, MLP, True, False), ("plain", 3 | C, True, False)),
    "unarmed fused update, sink": ((_fu(armed=False, tail=True), NS(groups=None, small_direct=None), 2, 1000, MLP,
                                    True, False), ("wire", 2 | C, True, False)),
    "armed, sink": ((_fu(), NS(groups=None, small_direct=None), 3, 1000, MLP, True, False), ("adam", 3 | C, True, False)),
    "armed, pipelined sink with views": ((_fu(), NS(groups=GROUPS, small_direct=BUCKET), 3, 1000, MLP, True, False),
                                         ("adam", 3 | C, True, True)),
    "tail, pipelined sink with views": ((_fu(tail=True), NS(groups=GROUPS, small_direct=BUCKET), 3, 1000, MLP, True,
                                         False), ("adam_tail", 3, False, False)),
    "tail, m_host == 0": ((_fu(tail=True, inline=True), None, 3, 0, MLP, True, True), ("adam", 3, False, False)),
    "tail, borrowed workspace": ((_fu(tail=True, inline=True), None, 3, 1000, MLP, False, True),
                                 ("adam", 3 | C, True, False)),
    "tail, atomic scatter": ((_fu(tail=True), None, 1, 1000, MLP, True, True), ("adam", 1, False, False)),
    "tail, clean workspace": ((_fu(tail=True), None, 3, 1000, MLP, True, True), ("adam_tail", 3 | C, False, False)),
    "closing tail, clean workspace": ((_fu(tail=True, inline=True), None, 2, 1000, MLP, True, True),
                                      ("adam_closing_tail", 2 | C, False, False)),
    "plain, atomic scatter": ((None, None, 0, 1000, MLP, True, True), ("plain", 0, False, False)),
    # the bare encoder (no MLP launch): no clearing, no SCATTER_CLEARED, no views, no tail
    "bare": ((None, None, 3, 1000, None, False, True), ("plain", 3, False, False)),
    "bare, armed tail": ((_fu(tail=True, inline=True), None, 3, 1000, None, True, True), ("adam", 3, False, False)),
    "bare, pipelined sink with views": ((None, NS(groups=GROUPS, small_direct=BUCKET), 3, 1000, None, False, True),
                                        ("bin", 3, False, False)),
}


@pytest.mark.parametrize("case", list(ROWS))
def test_backward_route(case):
    (fu, sink, variant, m_host, mlp, own_ws, ws_clean), (name, want_variant, clear, views) = ROWS[case]
    before = None if fu is None else dict(vars(fu))
    r = E.backward_route(fu, sink, variant, m_host, mlp, own_ws, ws_clean)
    assert (r.name, r.variant, r.clear) == (name, want_variant, clear)
    assert r.tail == (name in ("adam_tail", "adam_closing_tail"))
    if views:
        assert len(r.views) == 6 and all(v is BUCKET[t.data_ptr()] for v, t in zip(r.views, MLP))
    else:
        assert r.views is None
    assert fu is None or vars(fu) == before                       # the decision changes nothing
    if not r.clear:                                               # (the clear bytes are the library's)
        assert r.mlp_args(None, m_host) == (B.MLP_DEFER_REDUCE if r.tail else 0, None, 0)


def test_run_backward_bookkeeping(monkeypatch):
    """Each route issues its one scatter call and leaves the state the optimiser and the exchange read."""
    calls = []
    monkeypatch.setattr(E, "grid_encode_backward", lambda *a: calls.append(("plain", a[-1])) or a[-2])
    monkeypatch.setattr(E, "grid_encode_backward_adam", lambda *a: calls.append(("adam", a[-1])))
    monkeypatch.setattr(E, "grid_encode_backward_adam_tail", lambda *a: calls.append(("adam_tail", a[7], a[8:])))

    def bf16(*a, binned=False):
        calls.append(("bin" if binned else "wire", a[-1]))
        return "scatter ws"
    monkeypatch.setattr(E, "grid_encode_backward_bf16", bf16)

    def encoder(fu=None, sink=None):
        return NS(fused_update=fu, grad_sink=sink, levels="levels", scatter_variant=3, embeddings=torch.zeros(10, 2))

    def run(route, enc):
        return E.run_backward(route, torch.zeros(4, 3), 1.0, None, enc, 1000, None, 4, "mlp ws", B.BF16, 5)

    enc = encoder()
    dtable = run(E.Route("plain", 3 | C, True), enc)
    assert dtable.shape == (10, 2) and float(dtable.abs().sum()) == 0 and calls[-1] == ("plain", 3 | C)
    sink = NS(groups=None, pending=None, small_written=False)
    assert run(E.Route("wire", 3 | C, True), encoder(sink=sink)) is None and calls[-1] == ("wire", 3 | C)
    assert sink.pending is None and not sink.small_written
    sink = NS(groups=GROUPS, pending=None, small_written=False)
    assert run(E.Route("bin", 3 | C, True, [None] * 6), encoder(sink=sink)) is None and calls[-1] == ("bin", 3 | C)
    assert sink.pending == (1.0, "levels", 1000, 4, 3 | C, "scatter ws") and sink.small_written
    run(E.Route("bin", 3 | C, True), encoder(sink=sink))
    assert sink.small_written                                     # sticky: replays write the views without Python
    for name, closed, pending in (("adam", False, None), ("adam_tail", False, ("levels", 1000, 3, "scatter ws",
                                                                               "mlp ws", B.BF16, 5)),
                                  ("adam_closing_tail", True, None)):
        fu = NS(armed=True, applied=0, closed=False, pending_tail=None)
        assert run(E.Route(name, 3 | C, ws="scatter ws"), encoder(fu=fu)) is None
        assert not fu.armed and fu.applied == 1 and fu.closed == closed and fu.pending_tail == pending
        assert calls[-1][:2] == ("adam_tail" if name == "adam_closing_tail" else "adam", 3 | C)
    assert calls[-1][2] == ("mlp ws", B.BF16, 5)
