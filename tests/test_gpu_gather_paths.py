"""The load paths, the shapes and the addressing of the forward gather (csrc/grid_gather.hip, k_grid_forward).

The gather addresses everything with a wave-uniform base and a 32-bit byte offset, fetches the x pair of a cell of the
blocked layout with one dword-aligned 8-byte load when x mod 4 != 3, and leaves the registers of a lane that fetches
nothing as they are.  What can go wrong with that is a wrong row, a pair read across the end of a block, a level or the
table, a lane that blends registers nobody loaded, or a tile / level base that is off -- each of them a wrong feature,
so all checks are on values:

  * EXACT inputs (tests/exact_grid.py: the hand-set table, lattice positions, small-integer values).  Every feature
    equals the float64 oracle BIT FOR BIT: f32 features are the oracle, bf16 features its round-to-nearest cast, rows at
    and beyond m_dev keep what the output held.  The samples are the exact lattice plus cells chosen for the edges of
    the blocked layout, and the test asserts that they are there: cells with x mod 4 = 0, 1, 2, 3, cells whose y or z
    neighbour lies in the next block, cells that read the last block of a hashed level (of the levels of 4096 and
    12344 rows; the latter is the last level, its last block the end of the table).
  * shapes: M = 1, 63, 64, 65, 255, 257 and 5003 of those samples, with m_dev < m_host and level_stride > m_host, and
    once without m_dev; the first 80 samples are one point, a run across a 64-lane boundary.
  * ORDINARY inputs: every (gather_pair_loads, gather_dedup_max_res) setting gives the bytes of the plain path
    (single loads, no run sharing), the one tests/test_gpu_parity.py holds against the oracle.
  * a bound that is no power of two takes the division arm of the position: against the oracle at the tolerance of the
    other ordinary checks.
"""
import contextlib
import functools

import pytest
import torch

from oracle import nerf_oracle as O
from tests import exact_grid as X

pytestmark = pytest.mark.gpu

FILL = 123.0          # exact in bf16
SHAPES = (1, 63, 64, 65, 255, 257, 5003)
PAD_HOST, PAD_STRIDE = 300, 21          # m_host = M + 300 (tiles beyond m_dev), level_stride = m_host + 21
VERTS = X.EXACT_RES + 1                 # 34 vertices per axis


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
    try:
        for k, v in overrides.items():
            _set(k, v)
        yield
    finally:
        _restore_defaults()


# ------------------------------------------------------------------------------ the samples
def _cell_to_J(cells):
    """A lattice position inside cell (gx, gy, gz): pos = J / 8 + 0.5, so J = 8 g - 4 + r with r in [0, 8); r differs per
    axis and per cell so that no weight is zero by accident."""
    cells = torch.as_tensor(cells, dtype=torch.int64)
    r = (torch.arange(cells.shape[0]).view(-1, 1) * torch.tensor([1, 3, 5]) + torch.tensor([1, 2, 3])) % 8
    return (cells * 8 - 4 + r).clamp(0, 256)


def _last_block_cells():
    """Per hashed level of the exact table, up to 6 cells (gx, gy, gz in [0, 32]) with at least one vertex in the highest
    block of the level that the lattice reaches in the blocked layout, found with the oracle's row formula: the LAST
    block of the levels of 4096 and of 12344 rows (the latter ends the table)."""
    g = torch.arange(VERTS)
    verts = torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cells = []
    for a, b in zip(X.EXACT_OFFSETS[1:-1], X.EXACT_OFFSETS[2:]):
        hsize = b - a
        rows = O.grid_corner_indices(verts, X.EXACT_RES, hsize, blocked=True)
        # (the 16384-row level: the 34^3 lattice reaches 1008 of its 1024 blocks, the highest is block 1007)
        last = verts[rows >= (int(rows.max()) // 16) * 16]
        # the vertex is the cell's own corner (cell = vertex) or its +1 neighbour on every axis (cell = vertex - 1)
        picked = [v.clamp(max=VERTS - 2) for v in last[:3]] + [(v - 1).clamp(min=0) for v in last[:3]]
        cells += [c.tolist() for c in picked]
    return cells


@functools.lru_cache(maxsize=None)
def samples():
    """J int64 [5003, 3]: 80 times one point (a run over a wave boundary), the chosen cells, then the exact lattice."""
    lattice = X.exact_lattice()
    chosen = [(gx, gy, gz) for gx in (4, 5, 6, 7) for gy in (10, 11) for gz in (20, 21)]     # x mod 4 x (y, z) parity
    chosen += [(0, 0, 0), (32, 32, 32), (31, 32, 3), (3, 1, 32), (32, 0, 1)]                 # the corners of the lattice
    chosen += _last_block_cells()
    J = torch.cat([lattice[:80], _cell_to_J(chosen), lattice[80:]])[:SHAPES[-1]]
    assert J.shape[0] == SHAPES[-1]
    return J


@functools.lru_cache(maxsize=None)
def exact_reference(gridtype):
    """(x f32 [M, 3], table f32, features float64 [M, 8]) of the float64 oracle on `samples()`."""
    J = samples()
    x = J.float() / 128.0 - 1.0
    _, _, table, _ = X.exact_inputs()
    lv = X.exact_oracle_levels(gridtype)
    feat = O.grid_encode((x.double() + 1.0) / 2.0, table.double(), lv)
    assert torch.equal(feat.float().double(), feat)       # exact in f32, as exact_grid.py argues
    return x, table, feat


def test_samples_cover_the_edges_of_the_blocked_layout():
    """The claims of the module docstring about `samples()`, on the first 255 samples and on all of them."""
    J = samples()
    for n in (255, J.shape[0]):
        cell = (J[:n] + 4) // 8
        gx, gy, gz = cell[:, 0], cell[:, 1], cell[:, 2]
        assert sorted(set((gx % 4).tolist())) == [0, 1, 2, 3]
        for k in range(4):                                  # every x class with y / z neighbours inside and outside the block
            sel = (gx % 4) == k
            assert set(zip((gy[sel] % 2).tolist(), (gz[sel] % 2).tolist())) == {(0, 0), (0, 1), (1, 0), (1, 1)}, k
        corner = torch.tensor([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])
        verts = cell[:, None, :] + corner[None]
        for a, b in zip(X.EXACT_OFFSETS[1:-1], X.EXACT_OFFSETS[2:]):
            rows = O.grid_corner_indices(verts, X.EXACT_RES, b - a, blocked=True)
            last = (b - a) // 16 - 1 if b - a != 16384 else 1007     # (block 1007: see _last_block_cells)
            assert bool((rows >= last * 16).any()), "no sample reads the last block of the level of %d rows" % (b - a)
            assert int(rows.max()) < b - a
    assert bool((J[:80] == J[0]).all())                    # one run over lanes 0..63 and on into the next wave


def _describe(got, want):
    bad = torch.nonzero((got != want).reshape(got.shape[0], -1).any(-1)).flatten()
    J = samples()
    first = [(int(i), int(i) % 64, ((J[i] + 4) // 8).tolist()) for i in bad[:6]]
    return "%d of %d samples differ; first (sample, lane, cell) %s" % (len(bad), got.shape[0], first)


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_exact_features_every_path_and_shape(dev, gridtype, table_dtype):
    """Every (pair_loads, dedup) setting x every shape x both feature types on the exact inputs, bit for bit."""
    from src.latent_nerf.models import encoding as E
    x, table, ref = exact_reference(gridtype)
    levels = X.device_levels(gridtype)
    src = (table.to(torch.bfloat16) if table_dtype == "bf16" else table).to(dev)
    want = {torch.float32: ref.float(), torch.bfloat16: ref.float().to(torch.bfloat16)}
    failures = []
    for M in SHAPES:
        m_host, stride = M + PAD_HOST, M + PAD_HOST + PAD_STRIDE
        xd = torch.zeros(m_host, 3)
        xd[:M] = x[:M]
        xd = xd.to(dev)
        m_dev = torch.tensor([M], dtype=torch.int32, device=dev)
        for pl, dd in X.GATHER_SETTINGS:
            with tuning(gather_pair_loads=pl, gather_dedup_max_res=dd):
                for odt in (torch.float32, torch.bfloat16):
                    out = torch.full((4, stride, 2), FILL, device=dev, dtype=odt)
                    E.grid_encode_forward(xd, 1.0, src, levels, m_host, m_dev, stride, out=out)
                    out = out.cpu()
                    got = X.sample_major(out, M)
                    if not torch.equal(got, want[odt][:M]):
                        failures.append("M=%d pair_loads=%d dedup=%d out=%s: %s" % (
                            M, pl, dd, odt, _describe(got.float(), want[odt][:M].float())))
                    if not bool((out[:, M:] == FILL).all()):
                        failures.append("M=%d pair_loads=%d dedup=%d out=%s: rows beyond m_dev were written" % (M, pl, dd, odt))
    # without a device-side count: m_host is the count, level_stride == m_host
    M = 257
    for odt in (torch.float32, torch.bfloat16):
        out = E.grid_encode_forward(x[:M].to(dev), 1.0, src, levels, M, None, M, out_dtype=odt).cpu()
        if not torch.equal(X.sample_major(out, M), want[odt][:M]):
            failures.append("M=%d, no m_dev, out=%s: %s" % (M, odt, _describe(X.sample_major(out, M).float(), want[odt][:M].float())))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("table_dtype", ["f32", "bf16"])
@pytest.mark.parametrize("gridtype", X.LAYOUTS)
def test_ordinary_features_equal_the_plain_path(dev, gridtype, table_dtype):
    """Single loads without run sharing (pair_loads = 0, dedup = 0) is the reference: every other setting, the default
    included, gives its bytes, for f32 and bf16 features."""
    from src.latent_nerf.models import encoding as E
    case = X.ordinary_case(gridtype, table_dtype == "bf16")
    levels = E.GridLevels(X.SMALL["num_levels"], 2, X.SMALL["base_resolution"], X.SMALL["desired_resolution"],
                          X.SMALL["log2_hashmap_size"], gridtype=gridtype)
    x = case["x"].to(dev)
    M = x.shape[0]
    src = (case["table"].to(torch.bfloat16) if table_dtype == "bf16" else case["table"]).to(dev)
    failures = []
    for odt in (torch.float32, torch.bfloat16):
        with tuning(gather_pair_loads=0, gather_dedup_max_res=0):
            plain = E.grid_encode_forward(x, 1.0, src, levels, M, None, M, out_dtype=odt)
        assert float(plain.float().abs().max()) > 0
        for pl, dd in X.GATHER_SETTINGS:
            with tuning(gather_pair_loads=pl, gather_dedup_max_res=dd):
                got = E.grid_encode_forward(x, 1.0, src, levels, M, None, M, out_dtype=odt)
            if not torch.equal(got.view(torch.uint8), plain.view(torch.uint8)):
                bad = [l for l in range(16) if not torch.equal(got[l], plain[l])]
                failures.append("out=%s pair_loads=%d dedup=%d: levels %s differ" % (odt, pl, dd, bad))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("bound", [1.5, 2.0])
def test_bounds_take_their_arm_of_the_position(dev, bound):
    """2 * bound = 3 divides (x + bound) / (2 bound) per lane, 2 * bound = 4 multiplies by the reciprocal the host
    passes: both against the f32 oracle, which divides, at the tolerance of the ordinary checks (1e-4 / 1e-6)."""
    from src.latent_nerf.models import encoding as E
    case = X.ordinary_case("blocked", True)
    levels = E.GridLevels(X.SMALL["num_levels"], 2, X.SMALL["base_resolution"], X.SMALL["desired_resolution"],
                          X.SMALL["log2_hashmap_size"], gridtype="blocked")
    x = case["x"] * bound
    M = x.shape[0]
    ref = O.grid_encode((x + bound) / (2.0 * bound), case["table"], case["lv"])
    got = E.grid_encode_forward(x.to(dev), bound, case["table"].to(torch.bfloat16).to(dev), levels, M, None, M)
    err = (X.sample_major(got.cpu(), M).double() - ref.double()).abs()
    bad = err > 1e-6 + 1e-4 * ref.double().abs()
    assert not bool(bad.any()), "%d of %d outside the tolerance, max error %.3e" % (int(bad.sum()), bad.numel(), float(err.max()))
