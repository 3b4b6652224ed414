"""lnerf_decimate on the MI355X off the marching-cubes path: every case of tests/decimate_cases.py (each one asserted to
be what it claims in tests/test_decimate_edges_cpu.py) against the numpy restatement -- faces equal, vertices and normals
bit for bit (a NaN normal compares as NaN), the same rounds and collapses -- and, without the restatement, against
check_properties, the oracle written from the header; the raw C entry point with guard rows behind every output and
behind the scratch; repeatability.  No tolerance anywhere: bits, counts and exact topology.

Which case takes which branch for the first time on the device (csrc/decimate.hip, csrc/mesh_shared.h):
  k_dc_status, `len != deg` (two closed fans, every edge count 1)     bowtie, mixed (the pinch's faces lie in one plane,
    so without the lock an edge at it is round 1's cheapest collapse: the lock is what the result depends on)
  k_dc_status, the edge counts other than through a border            fin (an edge in three faces), dupface (a face
    twice), flipped (a face wound the other way), mixed.  (`nn != 1` and `pp != 1` alone can not decide a vertex: a
    neighbour that follows w in two faces precedes it in one, where `np` counts the two, or in none, where `pn` does.)
  k_dc_check clears a keep flag; compaction with F < n_faces;         repeats+isolated, alldegenerate
    outputs sized for n_faces that hold fewer
  deg == 0; k_dc_used / scan / k_dc_out_faces renumber around         repeats+isolated (unreferenced vertices at 0, in
    unreferenced input vertices                                         the middle and at V - 1), alldegenerate, nofaces
  F = 0 after compaction, n_faces = 0, n_verts = 0: launches over     alldegenerate, nofaces, nothing
    no items, scan_flat(n = 0), the pointers that may be NULL
  max_rounds other than the default                                   rounds0, rounds1, rounds3 (stops above the target)
  max_error between 1e-12 and inf                                     ceiling (1e-6 ends the run at 332 faces, not 0)
  targets F - 1, F - 3, 0, odd                                        target-1, target-3, target0, targetodd
  k_dc_rank over more than one tile of 256 (S = 568: three tiles),    rank1, rank257, rankS-1
    m in the first tile, just past it and S - 1
  lists longer than a wave and than a workgroup (k_vf_sort,           valence70, valence300
    k_dc_status's fan walk, k_dc_eval's link count)
  dc_face_quadric `l == 0`, dc_face_blocks `!nz0 -> nz1`              coincident
  a cost that is not finite; NaN and inf through quadrics, flip       nonfinite
    checks and normals
  f64 cancellation in d and in the cost                               faraway"""
import functools

import numpy as np
import pytest
import torch

from tests import decimate_cases as C
from tests import decimate_reference as D

pytestmark = pytest.mark.gpu

GUARD_ROWS = 64
GUARD_BYTES = 4096
SENTINEL = -7.0
SCRATCH_FILL = 0xA5


@pytest.fixture(scope="module")
def dev(built_lib):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(verts, faces, normals, info) of the restatement, computed once per case."""
    v, f, target, max_error, max_rounds = C.case(name)
    with np.errstate(invalid="ignore", over="ignore"):
        return D.decimate(v, f, target, max_error, max_rounds)


def _op(dev, name):
    from src.latent_nerf.raymarching import decimate_mesh
    v, f, target, max_error, max_rounds = C.case(name)
    st = {}
    ov, of, on = decimate_mesh(torch.from_numpy(v.copy()).to(dev), torch.from_numpy(f.copy()).to(dev), target, max_error,
                               max_rounds, stats=st)
    torch.cuda.synchronize()
    return ov.cpu().numpy(), of.cpu().numpy(), on.cpu().numpy(), st


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_normals(got, want):
    """Bit for bit where the restatement's normal is a number, NaN where it is NaN (payloads may differ)."""
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(_bits(a[0]), _bits(b[0])) and _same_normals(a[2], b[2]) and \
        _same_normals(b[2], a[2]) and a[3] == b[3]


@pytest.mark.parametrize("name", C.CASES)
def test_case_matches_restatement_and_header(dev, name):
    v, f, target, max_error, max_rounds = C.case(name)
    gv, gf, gn, st = _op(dev, name)
    rv, rf, rn, info = _ref(name)
    assert gf.dtype == np.int32 and gf.shape == rf.shape and np.array_equal(gf, rf)
    assert gv.shape == rv.shape and np.array_equal(_bits(gv), _bits(rv))
    assert _same_normals(gn, rn)
    assert st == info
    C.check_properties(v, f, gv, gf, st, target, max_rounds, C.marks(name)["end"])     # the GPU's own output


RAW = ["repeats+isolated", "mixed", "alldegenerate", "nofaces", "rank257", "valence300"]


@pytest.mark.parametrize("name", RAW)
def test_raw_entry_point_stays_inside_its_buffers(dev, name):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    v, f, target, max_error, max_rounds = C.case(name)
    rv, rf, rn, info = _ref(name)
    V, F = len(v), len(f)
    lib = B.get_lib()
    nbytes = lib.lnerf_decimate_scratch_bytes(V, F)
    assert nbytes > 0
    scratch = torch.full((nbytes + GUARD_BYTES,), SCRATCH_FILL, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    tv = torch.from_numpy(v.copy()).to(dev)
    tf = torch.from_numpy(f.astype(np.int32)).to(dev) if F else None
    out_v = torch.full((V + GUARD_ROWS, 3), SENTINEL, device=dev)
    out_n = torch.full((V + GUARD_ROWS, 3), SENTINEL, device=dev)
    out_f = torch.full((F + GUARD_ROWS, 3), -7, dtype=torch.int32, device=dev)
    B.call("lnerf_decimate", _p(tv), V, _p(tf), F, target, max_error, max_rounds, _p(scratch), nbytes, _p(out_v),
           _p(out_f), _p(out_n), _p(counts), _stream())
    torch.cuda.synchronize()
    assert counts.tolist() == [len(rv), len(rf), info["rounds"], info["collapses"]]
    Vo, Fo = len(rv), len(rf)
    assert Vo <= V and Fo <= F
    assert np.array_equal(_bits(out_v[:Vo].cpu().numpy()), _bits(rv)) and np.array_equal(out_f[:Fo].cpu().numpy(), rf)
    assert _same_normals(out_n[:Vo].cpu().numpy(), rn)
    # nothing behind the capacities (n_verts rows, n_faces rows, scratch_bytes) was written
    assert bool((out_v[V:] == SENTINEL).all()) and bool((out_n[V:] == SENTINEL).all())
    assert bool((out_f[F:] == -7).all())
    assert bool((scratch[nbytes:] == SCRATCH_FILL).all())
    if name in ("repeats+isolated", "alldegenerate", "nofaces"):
        assert Vo < V                        # unreferenced input vertices: the output is renumbered around them
    if name in ("repeats+isolated", "alldegenerate"):
        assert F > len(C.kept_faces(f))      # the input compaction dropped faces


def test_raw_entry_point_with_nothing_and_null_pointers(dev):
    from src.latent_nerf.raymarching import backend as B
    from src.latent_nerf.raymarching.raymarching import _p, _stream
    v, f, target, max_error, max_rounds = C.case("nothing")
    assert len(v) == 0 and len(f) == 0
    lib = B.get_lib()
    nbytes = lib.lnerf_decimate_scratch_bytes(0, 0)
    assert nbytes > 0
    scratch = torch.full((nbytes + GUARD_BYTES,), SCRATCH_FILL, dtype=torch.uint8, device=dev)
    counts = torch.full((4,), -1, dtype=torch.int64, device=dev)
    rc = lib.lnerf_decimate(None, 0, None, 0, target, max_error, max_rounds, _p(scratch), nbytes, None, None, None,
                            _p(counts), _stream())
    torch.cuda.synchronize()
    assert rc == B.LNERF_OK, lib.lnerf_last_error()
    assert counts.tolist() == [0, 0, 0, 0]
    assert bool((scratch[nbytes:] == SCRATCH_FILL).all())
    # vertices without faces, normals not asked for
    v, f, target, max_error, max_rounds = C.case("nofaces")
    V = len(v)
    nbytes = lib.lnerf_decimate_scratch_bytes(V, 0)
    scratch = torch.full((nbytes + GUARD_BYTES,), SCRATCH_FILL, dtype=torch.uint8, device=dev)
    counts.fill_(-1)
    tv = torch.from_numpy(v.copy()).to(dev)
    out_v = torch.full((V + GUARD_ROWS, 3), SENTINEL, device=dev)
    rc = lib.lnerf_decimate(_p(tv), V, None, 0, target, max_error, max_rounds, _p(scratch), nbytes, _p(out_v), None, None,
                            _p(counts), _stream())
    torch.cuda.synchronize()
    assert rc == B.LNERF_OK, lib.lnerf_last_error()
    assert counts.tolist() == [0, 0, 0, 0]
    assert bool((out_v == SENTINEL).all()) and bool((scratch[nbytes:] == SCRATCH_FILL).all())


@pytest.mark.parametrize("name", ["mixed", "rank257"])
def test_two_runs_give_identical_bits(dev, name):
    a, b = _op(dev, name), _op(dev, name)
    assert _same(a, b) and a[3]["collapses"] > 0


def test_a_nonfinite_mesh_leaves_nothing_behind(dev):
    before = _op(dev, "sphere")
    bad = _op(dev, "nonfinite")
    after = _op(dev, "sphere")
    assert not np.isfinite(bad[0]).all() and _same(before, after)
    assert np.isfinite(after[0]).all() and np.isfinite(after[2]).all()
