"""Static guard on the step loops of the bf16 MLP kernels (csrc/mlp_bf16.hip): the inputs of the NEXT step of a
persistent workgroup stay in flight across the whole arithmetic of a step.

Neither kernel is near its memory or its MFMA limit; what they lose is memory round trips that stand in series with the
arithmetic.  Where the compiler puts its `s_waitcnt vmcnt` is not written in the source: a
select behind a load, a load used under a lane predicate only, a run-time branch around two load forms, a load still
pending at the back edge -- each puts a wait (mostly vmcnt(0), which also covers the previous stores) directly behind
the loads it was meant to overlap, and the source looks the same.  So this test compiles the file to gfx950 assembly
with the flags of the product build and reads the two loops that the benched configuration runs: the forward and the
backward (four waves of two tiles) with bf16 features and out_dim 5.  No GPU is needed.

Terms.  The STEP LOOP of a kernel is the innermost loop (label .. backward branch to it) that holds all of the kernel's
v_mfma.  The instructions that are RELEVANT to the vector-memory queue are vector-memory instructions (global_*,
buffer_*, flat_*, scratch_*), `s_waitcnt` with a vmcnt field, and v_mfma (the arithmetic a load is meant to fly under);
everything else (address arithmetic, LDS, scalar code) is skipped when the test looks for "the next" one."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-nerf-test_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# The same reading of the PARENT's source (aa4d2b3: k_mlp_forward_bf16<3>, k_mlp_backward_bf16<4, 2>, the run-time
# a.feat_bf16 / a.out_dim arms inside the loops), with the compiler below.  `waits_under_loads`: s_waitcnt vmcnt between
# the first global_load and the last v_mfma of the step loop; `loads_waited_at_once`: global_load whose next relevant
# instruction is s_waitcnt vmcnt(0).
HIPCC_VERSION_OF_THE_COUNTS = "HIP 7.2.26015-fc0010cf6a, AMD clang 22.0.0git (roc-7.2.0 26014)"
PARENT = {
    # 8 dword + 8 dwordx2 feature loads on two arms and one dwordx3 position load; all 10 waits of the loop stand
    # between its first load and its last MFMA; the second tile's position load is followed at once by vmcnt(0)
    "forward": {"vgprs": 164, "global_loads": 17, "waits_under_loads": 10, "loads_waited_at_once": 1},
    # the upstream's dword / dwordx3 / dword offset:12 loads are waited for with vmcnt(1), vmcnt(0) behind them, the
    # feature loads with vmcnt(0) in front of the first MFMA: 5 of the loop's 7 waits stand under its loads
    "backward": {"vgprs": 190, "global_loads": 14, "waits_under_loads": 5, "loads_waited_at_once": 0},
}

# mlp_fwd_wps stays 3 (three waves per SIMD: 512 / 3 rounded down to the allocation granule of 8)
VGPR_LIMIT = {"forward": 168, "backward": 256}

# (mangled-name pattern of the instantiation the bench runs: bf16 features = Lb1, out_dim 5 = Lb1)
BENCHED = {
    "forward": r"_ZN5lnerf18k_mlp_forward_bf16ILi3ELb1ELb1EEE\w+",
    "backward": r"_ZN5lnerf19k_mlp_backward_bf16ILb1ELb1EEE\w+",
}


def _build_flags():
    spec = importlib.util.spec_from_file_location("lnerf_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FLAGS)


def _mlp_asm(source=None):
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "mlp_bf16.s")
        subprocess.check_call([HIPCC] + _build_flags() + ['-DLNERF_BUILD_TAG="asm"', "--cuda-device-only", "-S", "-o", out,
                                                         source or os.path.join(PKG, "csrc", "mlp_bf16.hip")],
                              stderr=subprocess.DEVNULL)
        return open(out).read()


def _instructions(body):
    """[(label or None, text)] in program order: labels as (name, None), instructions as (None, 'op operands')."""
    out = []
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if not line or line.startswith("."):
            m = re.match(r"^(\.LBB\d+_\d+):", line)
            if m:
                out.append((m.group(1), None))
            continue
        if line.endswith(":"):
            continue
        out.append((None, line))
    return out


def _is_vmem(ins):
    return ins.startswith(("global_", "buffer_", "flat_", "scratch_"))


def _is_vm_wait(ins):
    return ins.startswith("s_waitcnt") and "vmcnt" in ins


def _relevant(ins):
    return _is_vmem(ins) or _is_vm_wait(ins) or ins.startswith("v_mfma")


def step_loop(body):
    """The instructions (text only, program order) of the innermost loop that holds every v_mfma of the kernel."""
    items = _instructions(body)
    where = {name: i for i, (name, _) in enumerate(items) if name}
    mfma = [i for i, (_, ins) in enumerate(items) if ins and ins.startswith("v_mfma")]
    assert mfma, "no v_mfma in the kernel"
    best = None
    for i, (_, ins) in enumerate(items):
        if not ins or not ins.startswith(("s_cbranch", "s_branch")):
            continue
        head = where.get(ins.split()[-1])
        if head is None or head > i:
            continue                                       # a forward branch
        if head <= mfma[0] and mfma[-1] <= i and (best is None or i - head < best[1] - best[0]):
            best = (head, i)
    assert best, "no loop around the kernel's v_mfma"
    return [ins for _, ins in items[best[0]:best[1] + 1] if ins]


def loop_report(loop):
    loads = [i for i, ins in enumerate(loop) if ins.startswith("global_load")]
    mfma = [i for i, ins in enumerate(loop) if ins.startswith("v_mfma")]
    assert loads and mfma, (len(loads), len(mfma))
    under = [ins for ins in loop[loads[0]:mfma[-1] + 1] if _is_vm_wait(ins)]
    at_once = []
    for i in loads:
        nxt = next((ins for ins in loop[i + 1:] if _relevant(ins)), None)
        if nxt is not None and _is_vm_wait(nxt) and "vmcnt(0)" in nxt:
            at_once.append(loop[i])
    return {"global_loads": len(loads), "mfma": len(mfma), "waits_under_loads": len(under),
            "loads_waited_at_once": len(at_once), "vm_waits": sum(1 for ins in loop if _is_vm_wait(ins)),
            "first_load_before_first_mfma": loads[0] < mfma[0]}


def kernels_of(asm):
    """{mangled name: (body, vgprs, scratch bytes)} of every kernel of the file."""
    found = {}
    for m in re.finditer(r"^(_ZN5lnerf\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(name), asm, flags=re.S)
        if not meta:
            continue                                       # a device function, not a kernel
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta.group(1)).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta.group(1)).group(1))
        found[name] = (body, vgprs, scratch)
    return found


@pytest.fixture(scope="module")
def kernels():
    found = kernels_of(_mlp_asm())
    assert len(found) >= 4, sorted(found)
    return found


def _benched(kernels, which):
    names = [n for n in kernels if re.fullmatch(BENCHED[which], n)]
    assert len(names) == 1, (which, sorted(kernels))
    return kernels[names[0]]


pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

WHICH = pytest.mark.parametrize("which", ["forward", "backward"])


@WHICH
def test_no_wait_between_the_loads_and_the_last_mfma(kernels, which):
    """a) From the first global_load of a step (the next step's inputs, requested at its top) to its last v_mfma there is
    no s_waitcnt vmcnt: the loads are in flight under all of the step's arithmetic."""
    rep = loop_report(step_loop(_benched(kernels, which)[0]))
    print("%s step loop: %s (parent: %s)" % (which, rep, PARENT[which]))
    assert rep["first_load_before_first_mfma"], rep
    assert rep["waits_under_loads"] == 0, rep


@WHICH
def test_no_load_is_waited_for_at_once(kernels, which):
    """b) No global_load of the loop has `s_waitcnt vmcnt(0)` as its next instruction that matters to the memory queue."""
    rep = loop_report(step_loop(_benched(kernels, which)[0]))
    assert rep["loads_waited_at_once"] == 0, rep


@WHICH
def test_registers(kernels, which):
    """c) The forward stays at three waves per SIMD (mlp_fwd_wps = 3 is the default that was kept): <= 168 VGPRs; the
    backward runs two: <= 256."""
    vgprs = _benched(kernels, which)[1]
    print("%s: %d VGPRs (parent: %d)" % (which, vgprs, PARENT[which]["vgprs"]))
    assert vgprs <= VGPR_LIMIT[which], (which, vgprs)


def test_no_scratch_anywhere(kernels):
    """d) No kernel of the file has a private segment."""
    with_scratch = {n: s for n, (_, _, s) in kernels.items() if s}
    assert not with_scratch, with_scratch


@WHICH
def test_fewer_loads_than_the_parent(kernels, which):
    """e) One load form per input: the loop holds no more global loads than the parent's (which carried both feature forms
    in the forward), and strictly fewer vmcnt waits under them."""
    rep = loop_report(step_loop(_benched(kernels, which)[0]))
    assert rep["global_loads"] <= PARENT[which]["global_loads"], (rep, PARENT[which])
    assert rep["waits_under_loads"] < PARENT[which]["waits_under_loads"], (rep, PARENT[which])


# The arithmetic of a step, counted in the source (csrc/mlp_bf16.hip).  Forward: layers 1-2 8 + 16, layer 3 4.  Backward:
# layers 1-2 8 + 16; dW3 / db3 4 k-steps x 2; dA2 8; dW2 / db2 4 x 5; dA1 16; dW1 / db1 4 x 3; dX 8.  One pair of
# barriers per weight-gradient stage.
MFMA_PER_STEP = {"forward": 8 + 16 + 4, "backward": 8 + 16 + 4 * 2 + 8 + 4 * 5 + 16 + 4 * 3 + 8}   # 28, 96
BARRIERS_PER_BACKWARD_STEP = 6


@WHICH
def test_arithmetic_of_a_step(kernels, which):
    """f) The named parts of the step neither duplicate nor drop arithmetic: the step loop holds exactly the v_mfma the
    source counts (28 forward, 96 backward), and the backward's its six s_barrier."""
    loop = step_loop(_benched(kernels, which)[0])
    mfma = sum(1 for ins in loop if ins.startswith("v_mfma"))
    barriers = sum(1 for ins in loop if ins.startswith("s_barrier"))
    print("%s step loop: %d v_mfma, %d s_barrier" % (which, mfma, barriers))
    assert mfma == MFMA_PER_STEP[which], (which, mfma)
    if which == "backward":
        assert barriers == BARRIERS_PER_BACKWARD_STEP, barriers
