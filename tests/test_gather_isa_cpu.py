"""Static guard on the ISA of the forward gather (csrc/grid_gather.hip, k_grid_forward<bf16 table, bf16 features>).

Half of the vector instructions the gather used to issue per launch (27.5 M, now 14.3 M) computed addresses, repeated a
wave-uniform reciprocal per lane, cleared registers nobody read or selected two dwords out of sixteen bytes; taking them
out was worth 4.7 us of its 65.5.  None of that is visible in the results, and most of it is
not visible in the source either -- whether a load takes `scalar base + 32-bit offset` or a 64-bit vector address is the
compiler's reading of the pointer arithmetic.  So this test compiles the file to gfx950 assembly with the flags of the
product build and reads the kernel.  No GPU is needed."""
import importlib.util
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "latent-nerf-test_amd")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# The kernel on the commit before the addresses went into scalar registers (515da39), counted with the compiler below,
# statically over all arms of the instantiation: 701 vector instructions at 53 VGPRs, among them 30 v_lshl_add_u64 (the
# address of every table load and of the store) and 2 v_mad_u64_u32 (the position's), 78 v_cndmask_b32, 63 v_mov_b32 and
# four IEEE division sequences (v_div_scale / v_rcp_f32 / v_div_fmas / v_div_fixup): three in the arm of a bound that is
# no power of two, one in front of the tile loop, run by every wave.
HIPCC_VERSION_OF_THE_COUNTS = "HIP 7.2.26015-fc0010cf6a, AMD clang 22.0.0git (roc-7.2.0 26014)"
PARENT_VECTOR_INSTRUCTIONS = 701
PARENT_VGPRS = 53
VGPR_LIMIT = 64                      # eight waves per SIMD

# every spelling of a 64-bit vector add or multiply-add on gfx950 (an address computed per lane)
WIDE_ADDS = ("v_lshl_add_u64", "v_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_u32", "v_addc_co_u32",
             "v_add_co_ci_u32")
DIVISION = ("v_rcp_f32", "v_div_scale_f32", "v_div_fmas_f32", "v_div_fixup_f32")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


def _build_flags():
    spec = importlib.util.spec_from_file_location("lnerf_build", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.FLAGS)


def _gather_asm():
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "grid_gather.s")
        subprocess.check_call([HIPCC] + _build_flags() + ['-DLNERF_BUILD_TAG="asm"', "--cuda-device-only", "-S", "-o", out,
                                                         os.path.join(PKG, "csrc", "grid_gather.hip")], stderr=subprocess.DEVNULL)
        return open(out).read()


@pytest.fixture(scope="module")
def kernel():
    """(blocks, vgprs, scratch bytes) of k_grid_forward<uint16_t, uint16_t>; blocks = the basic blocks in program order,
    each a list of (opcode, operands); block 0 is the entry block."""
    asm = _gather_asm()
    m = re.search(r"^(_ZN5lnerf14k_grid_forwardIttE\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, flags=re.S | re.M)
    assert m, "k_grid_forward<uint16_t, uint16_t> not found"
    name, body = m.group(1), m.group(2)
    blocks = [[]]
    for line in body.splitlines():
        line = line.split(";")[0].strip()
        if not line or line.startswith("."):
            if re.match(r"\.LBB\d+_\d+:", line):
                blocks.append([])
            continue
        op, _, rest = line.partition(" ")
        blocks[-1].append((op, rest.strip()))
        if op.startswith(("s_cbranch", "s_branch")):
            blocks.append([])
    meta = re.search(r"\.name:\s+%s\n(.*?)\.wavefront_size" % re.escape(name), asm, flags=re.S)
    assert meta, "no metadata of %s" % name
    vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", meta.group(1)).group(1))
    scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", meta.group(1)).group(1))
    return [b for b in blocks if b], vgprs, scratch


def _flat(blocks):
    return [ins for b in blocks for ins in b]


def test_registers_and_scratch(kernel):
    """Eight waves per SIMD need <= 64 VGPRs; no scratch."""
    _, vgprs, scratch = kernel
    print("%d VGPRs (before: %d), %d bytes of scratch" % (vgprs, PARENT_VGPRS, scratch))
    assert vgprs <= VGPR_LIMIT, vgprs
    assert scratch == 0, scratch


def test_no_address_arithmetic_on_the_vector_unit(kernel):
    """From the first table load to the feature store -- in fact in the whole kernel -- there is no 64-bit vector add:
    every global access is `scalar base + 32-bit vector offset`, and none is a flat access."""
    ins = _flat(kernel[0])
    mem = [i for i, (op, _) in enumerate(ins) if op.startswith(("global_", "flat_", "buffer_"))]
    loads = [i for i in mem if ins[i][0].startswith("global_load") and ins[i][0] != "global_load_dwordx3"]
    stores = [i for i in mem if ins[i][0].startswith("global_store")]
    assert loads and len(stores) == 1, (len(loads), len(stores))
    assert loads[0] < stores[0]
    between = [op for op, _ in ins[loads[0]:stores[0]] if op.startswith(WIDE_ADDS)]
    anywhere = [op for op, _ in ins if op.startswith(WIDE_ADDS)]
    print("%d global accesses, %d 64-bit vector adds between the first table load and the store, %d in the kernel"
          % (len(mem), len(between), len(anywhere)))
    assert between == [], between
    assert anywhere == [], anywhere
    for i in mem:
        op, operands = ins[i]
        assert op.startswith("global_"), op
        assert re.search(r"s\[\d+:\d+\]\s*$", operands) and not operands.endswith("off"), (op, operands)


def test_divisions_only_in_the_arm_of_other_bounds(kernel):
    """x / (2 bound) is three IEEE divisions in ONE block behind a branch (a bound that is no power of two); the
    reciprocal of a power-of-two bound comes from the host: no v_rcp_f32 and no v_div_* anywhere else, in particular not
    in front of the tile loop."""
    blocks = kernel[0]
    where = [k for k, b in enumerate(blocks) if any(op.startswith(DIVISION) for op, _ in b)]
    print("division instructions in blocks %s of %d" % (where, len(blocks)))
    assert len(where) == 1 and where[0] != 0, where
    ops = [op for op, _ in blocks[where[0]]]
    assert sum(1 for op in ops if op.startswith("v_rcp_f32")) == 3, ops
    assert sum(1 for op in ops if op.startswith("v_div_fixup_f32")) == 3, ops
    # the block is entered by a branch on the host's reciprocal: the block in front of it ends in one
    assert blocks[where[0] - 1][-1][0].startswith("s_cbranch"), blocks[where[0] - 1][-1]


def test_fewer_vector_instructions_than_before(kernel):
    """The whole kernel, all arms: fewer vector instructions than the 701 of the kernel before."""
    ops = [op for op, _ in _flat(kernel[0])]
    valu = [op for op in ops if op.startswith("v_")]
    counts = {}
    for op in valu:
        counts[op] = counts.get(op, 0) + 1
    top = sorted(counts.items(), key=lambda kv: -kv[1])[:8]
    print("%d vector instructions (before: %d); most frequent %s" % (len(valu), PARENT_VECTOR_INSTRUCTIONS, top))
    assert len(valu) < PARENT_VECTOR_INSTRUCTIONS, len(valu)
