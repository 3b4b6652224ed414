"""What tests/test_gpu_tuning_paths.py rests on, checked where it can be checked without a GPU:
  * the table of tuning defaults the GPU tests restore (tests/exact_grid.py) equals the initialisers in the C sources --
    a changed default cannot silently leave later tests on a non-default path;
  * the exactness claim of the exact-arithmetic inputs: the f32 oracle equals the f64 oracle bit for bit, the runs are
    as long as the kernels' run logic needs them, and every sum fits the number formats it travels in."""
import os
import re

import torch

from tests import exact_grid as X

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "latent-nerf-test_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_default_table_equals_the_initialisers_in_the_sources():
    grid, mlp = _read("grid.hip"), _read("mlp.hip")
    # key -> global, from lnerf_set_tuning itself
    body = grid[grid.index("int lnerf_set_tuning("):]
    body = body[:body.index("unknown key")]
    key_to_global = {}
    for m in re.finditer(r'strcmp\(key, "(\w+)"\) == 0\) \{(.*?)return LNERF_OK;', body, flags=re.S):
        (glob,) = set(re.findall(r"\b(g_\w+) = ", m.group(2)))
        key_to_global[m.group(1)] = glob
    assert sorted(key_to_global) == sorted(X.TUNING_DEFAULTS) and len(key_to_global) == 12
    assert len(set(key_to_global.values())) == 12
    constants = {}
    for name in sorted(os.listdir(CSRC)):
        for m in re.finditer(r"constexpr int (\w+) = (\d+)\s*[;,]", _read(name)):
            constants[m.group(1)] = int(m.group(2))
    for key, glob in key_to_global.items():
        found = re.findall(r"^int %s = (\w+);" % glob, grid + "\n" + mlp, flags=re.M)
        assert len(found) == 1, (key, glob, found)
        value = int(found[0]) if found[0].isdigit() else constants[found[0]]
        assert value == X.TUNING_DEFAULTS[key], (key, glob, value)
    # every default lies inside its own range
    for key, refused in X.TUNING_REFUSED.items():
        assert X.TUNING_DEFAULTS[key] not in refused


def test_exact_level_table_is_what_the_tests_say():
    sizes = [b - a for a, b in zip(X.EXACT_OFFSETS[:-1], X.EXACT_OFFSETS[1:])]
    assert tuple(sizes) == X.EXACT_SIZES
    lattice = (X.EXACT_RES + 1) ** 3
    assert sizes[0] == lattice and all(s < lattice for s in sizes[1:])           # dense, then three hashed levels
    assert [-(-s // 4096) for s in sizes] == [10, 4, 1, 4]                        # buckets
    pow2 = [s & (s - 1) == 0 for s in sizes]
    assert pow2 == [False, True, True, False]
    nblk = sizes[3] // 16
    assert nblk == 771 and nblk & (nblk - 1) != 0                                 # the `% nblk` arm of the blocked layout
    assert all(o % 8 == 0 for o in X.EXACT_OFFSETS)                               # 16-byte loads stay aligned
    assert X.EXACT_M == 5917 and X.EXACT_M % 64 and X.EXACT_M % 256
    # capacity 3 M: the one-bucket level is planned with more than one slice (8 m_host / nb > 65536 records) ...
    assert 8 * X.EXACT_CAPACITY // 1 > 65536
    # ... and, merging off, its bucket holds more than one slice's 16384 records: the sliced sum runs
    grad = X.exact_inputs()[3].reshape(X.EXACT_M, 4, 2)
    assert 8 * int((grad[:, 2].abs().sum(-1) > 0).sum()) > 16384
    # scatter_bin_wgs = 4: one workgroup per level, twelve items each
    assert -(-X.EXACT_M // 512) == 12


def test_exact_positions_have_the_runs_the_kernels_merge():
    J = X.exact_lattice()
    assert J.shape == (X.EXACT_M, 3) and int(J.min()) == 0 and int(J.max()) == 256
    assert bool((J == 0).all(-1).any()) and bool((J == 256).all(-1).any())       # both corners of the box
    x = X.exact_inputs()[1]
    assert torch.equal((x.double() + 1.0) * 128.0, J.double())                    # x = J / 128 - 1 exactly
    # the helper's integer cell equals the oracle's floor(pos)
    pos = (x + 1.0) / 2.0 * X.EXACT_SCALE + 0.5
    assert torch.equal(torch.floor(pos).long(), (J + 4) // 8) and int(((J + 4) // 8).max()) + 1 <= X.EXACT_RES
    lengths, _ = X.cell_runs(J)
    assert int(lengths.max()) >= 65 and int((lengths > 1).sum()) > 500
    # in a wavefront: runs that cross a row of 16 lanes, lane 32, and one that fills the wavefront
    wl, rid = X.cell_runs(J, wave=64)
    first = torch.zeros(len(wl), dtype=torch.long).scatter_reduce(0, rid, torch.arange(X.EXACT_M) % 64, "amin",
                                                                  include_self=False)
    last = first + wl - 1
    assert int(wl.max()) == 64
    assert bool(((first < 16) & (last >= 16)).any()) and bool(((first < 32) & (last >= 32)).any())
    assert bool(((first % 16 != 0) & (first // 16 != last // 16)).any())          # ... starting inside a row
    # zero gradients inside and across runs
    grad = X.exact_inputs()[3]
    zero = grad.abs().sum(-1) == 0
    nz_per_run = torch.zeros(len(wl)).index_add_(0, rid, (~zero).float())
    assert bool(((nz_per_run > 0) & (nz_per_run < wl)).any()) and bool((nz_per_run == 0).any())


def test_exact_inputs_are_exact_in_f32():
    """The f32 oracle equals the f64 oracle bit for bit (features and table gradient), for all three layouts, and every
    intermediate sum fits: run sums in the 18 significant bits of an 8-byte record, row sums in an f32."""
    J, x, table, grad = X.exact_inputs()
    assert torch.equal(table * 8, (table * 8).round()) and float(table.abs().max()) <= 4.0
    assert torch.equal(table, table.to(torch.bfloat16).float())                   # exact in bf16 too
    assert torch.equal(grad, grad.round()) and float(grad.abs().max()) == 3.0
    assert bool((grad[(torch.arange(X.EXACT_M) % X.EXACT_PER_RAY) > 70] == 0).all())
    _, rid = X.cell_runs(J, wave=64)
    pos = (x.double() + 1.0) / 2.0 * X.EXACT_SCALE + 0.5
    frac = pos - torch.floor(pos)
    for gridtype in X.LAYOUTS:
        case = X.exact_case(gridtype)
        f32, d32 = X.oracle_forward_backward(x, table, grad, case["lv"], torch.float32)
        assert f32.dtype == torch.float32 and case["feat"].dtype == torch.float64
        assert torch.equal(f32.double(), case["feat"]) and torch.equal(d32.double(), case["dtable"])
        assert torch.equal(case["feat"] * 4096, (case["feat"] * 4096).round())
        dt = case["dtable"]
        assert torch.equal(dt * 512, (dt * 512).round())
        assert float(dt.abs().max()) * 512 < 2 ** 24
        assert float(dt.abs().max()) > 8 and int((dt.abs().sum(-1) > 0).sum()) > 5000
        # no partial sum of a row, in any order, leaves the f32 integers either: sum of |w g| per row
        _, dabs = X.oracle_forward_backward(x, torch.zeros_like(table), grad.abs(), case["lv"], torch.float64)
        assert float(dabs.max()) * 512 < 2 ** 24
        # position gradient: multiples of 2^-5 (16 x 1/512) far below 2^24 of them
        dx = case["dxyz"]
        assert torch.equal(dx * 32, (dx * 32).round()) and float(dx.abs().max()) * 32 < 2 ** 24
        assert torch.equal(dx.float().double(), dx) and float(dx.abs().max()) > 0
    # run sums (per corner, level and feature; the lanes of one wavefront): below 2^17 / 512
    worst = 0.0
    for c in range(8):
        w = torch.ones(X.EXACT_M, dtype=torch.float64)
        for a in range(3):
            w = w * (frac[:, a] if (c >> a) & 1 else 1.0 - frac[:, a])
        assert torch.equal(w * 512, (w * 512).round())
        sums = torch.zeros(int(rid.max()) + 1, 8, dtype=torch.float64).index_add_(0, rid, w[:, None] * grad.double().abs())
        worst = max(worst, float(sums.max()))
    assert 3 < worst < 2 ** 17 / 512          # (above 3: larger than any single record, i.e. runs do add up)


def test_first_ray_case_leaves_buckets_without_records():
    """m_dev = EXACT_PER_RAY (test_exact_scatter_buckets_without_records): the no-records arm of every finisher of pass 2
    needs buckets that receive nothing, next to buckets that do, and the one-bucket level planned sliced but summed by
    one workgroup."""
    assert X.EXACT_PER_RAY == 97
    for gridtype in X.LAYOUTS:
        full, one = X.exact_case(gridtype)["dtable"], X.first_ray_case(gridtype)
        dt, empty = one["dtable"], one["empty"]
        assert float(dt.abs().max()) > 0 and not torch.equal(dt, full)
        assert torch.equal(dt.float().double(), dt)                               # exact in f32, as the whole case is
        nb = [-(-s // 4096) for s in X.EXACT_SIZES]
        # the dense level: a full bucket and the partial last bucket stay empty
        assert any(b - a == 4096 for a, b in empty[0]), gridtype
        assert (X.EXACT_OFFSETS[1] - X.EXACT_SIZES[0] % 4096, X.EXACT_OFFSETS[1]) in empty[0], gridtype
        assert len(empty[0]) == 8 and len(empty[2]) == 0 and len(empty[3]) == 2, (gridtype, [len(e) for e in empty])
        # every level keeps a bucket with records, the one-bucket level among them
        assert all(len(e) < n for e, n in zip(empty, nb)), gridtype
        for spans in empty:
            for a, b in spans:
                assert float(dt[a:b].abs().max()) == 0.0
    # the one-bucket level is still PLANNED sliced (8 m_host / nb > 65536) and holds far less than one slice's records
    assert 8 * X.EXACT_CAPACITY // 1 > 65536 and 8 * X.EXACT_PER_RAY < 16384


def test_ordinary_inputs_shape():
    x, grad = X.ordinary_inputs()
    assert x.shape == (29100, 3) and x.shape[0] <= 30000 and grad.shape == (29100, 32)
    assert float(x.abs().max()) < 1.0
    dead = grad.abs().sum(-1) == 0
    assert 0.1 < float(dead.float().mean()) < 0.9
