"""Static guard on the PROLOGUES of the bf16 MLP kernels (csrc/mlp_bf16.hip): one exposed memory round trip, not two.

The persistent workgroups of a launch all start together and nothing else is resident, so whatever a prologue waits for
is waited for by the whole GPU.  The kernels therefore request the cached weight fragments and the biases first, the
inputs of the first step behind them, and only then write fragments and biases to LDS: vector loads return in issue
order, so the writes wait for the fragments only -- with `s_waitcnt vmcnt(n)`, n > 0 -- and the inputs cross the writes
and the workgroup's barrier in flight.  As with the step loops (tests/test_mlp_isa_cpu.py) none of this is written in the
source: a register copy, a select or a merge of two arms behind a load makes the compiler wait where the value stands.
So this test compiles the file with the flags of the product build and reads the two benched instantiations.  No GPU.

Terms.  The PROLOGUE is the program text from the kernel's entry to the head of its step loop (test_mlp_isa_cpu's
definition), without the text of any OTHER loop that stands there: the only loop the source has in front of the step loop
is build_fragments, the arm of a launch without a fragment cache (a.frag_global == nullptr), which does its own
dependent loads as it always did.  The copy of the cached fragments is fully unrolled."""
import os
import re

import pytest

from tests import test_mlp_isa_cpu as T

pytestmark = pytest.mark.skipif(not os.path.exists(T.HIPCC), reason="needs hipcc")

WHICH = pytest.mark.parametrize("which", ["forward", "backward"])

# 16-byte fragment words a thread copies: 14 / 30 fragments of 64 words over 256 threads, rounded up
FRAGMENT_LOADS = {"forward": 4, "backward": 8}


@pytest.fixture(scope="module")
def kernels():
    return T.kernels_of(T._mlp_asm())


def prologue(body):
    """The instructions (text, program order) in front of the step loop that are in no other loop."""
    items = T._instructions(body)
    where = {name: i for i, (name, _) in enumerate(items) if name}
    mfma = [i for i, (_, ins) in enumerate(items) if ins and ins.startswith("v_mfma")]
    loops = []
    for i, (_, ins) in enumerate(items):
        if ins and ins.startswith(("s_cbranch", "s_branch")):
            head = where.get(ins.split()[-1])
            if head is not None and head <= i:
                loops.append((head, i))
    step = min((l for l in loops if l[0] <= mfma[0] and mfma[-1] <= l[1]), key=lambda l: l[1] - l[0])
    other = [l for l in loops if l[1] < step[0]]
    return [ins for i, (_, ins) in enumerate(items[:step[0]]) if ins and not any(a <= i <= b for a, b in other)]


@WHICH
def test_every_load_is_issued_before_the_first_barrier(kernels, which):
    """a) Every global_load of the prologue -- fragments, biases, the first step's inputs -- stands in front of the first
    s_barrier: nothing is requested only after the workgroup has met."""
    pro = prologue(T._benched(kernels, which)[0])
    barriers = [i for i, ins in enumerate(pro) if ins.startswith("s_barrier")]
    loads = [i for i, ins in enumerate(pro) if ins.startswith("global_load")]
    print("%s prologue: %d instructions, %d global_load, first s_barrier at %s" % (which, len(pro), len(loads), barriers[:1]))
    assert barriers and loads, (barriers, loads)
    late = [pro[i] for i in loads if i > barriers[0]]
    assert not late, late
    wide = [i for i in loads if pro[i].startswith("global_load_dwordx4")]
    assert len(wide) >= FRAGMENT_LOADS[which], (which, len(wide))


@WHICH
def test_at_most_one_full_wait(kernels, which):
    """b) At most one `s_waitcnt vmcnt(0)` between the kernel's entry and the loop (the pin of the first step's inputs): the
    LDS writes of the fragments wait with a count that leaves the inputs in flight."""
    pro = prologue(T._benched(kernels, which)[0])
    full = [i for i, ins in enumerate(pro) if T._is_vm_wait(ins) and "vmcnt(0)" in ins]
    print("%s prologue: vm waits %s" % (which, [ins for ins in pro if T._is_vm_wait(ins)]))
    assert len(full) <= 1, [pro[i] for i in full]


@WHICH
def test_the_fragment_writes_leave_the_inputs_in_flight(kernels, which):
    """c) What a) and b) are for: the last global_load of the prologue stands in front of the first 16-byte LDS write, and
    no vmcnt(0) stands in front of the last one -- the fragments go to LDS while the inputs are on their way."""
    pro = prologue(T._benched(kernels, which)[0])
    loads = [i for i, ins in enumerate(pro) if ins.startswith("global_load")]
    writes = [i for i, ins in enumerate(pro) if re.match(r"ds_write_b128|ds_store_b128", ins)]
    assert len(writes) >= FRAGMENT_LOADS[which], (which, len(writes))
    assert loads[-1] < writes[0], (pro[loads[-1]], pro[writes[0]])
    early = [ins for ins in pro[:writes[-1]] if T._is_vm_wait(ins) and "vmcnt(0)" in ins]
    assert not early, early
