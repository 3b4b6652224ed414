"""Mesh decimation off the marching-cubes path, without a GPU: every case of tests/decimate_cases.py goes through the
numpy restatement (tests/decimate_reference.py; its own per-round assertion that a collapse removes two faces must hold)
and the result through check_properties, the oracle written from the header.  Each case's premise -- that it is the
input it claims to be and reaches the branch it is there for -- is asserted from the brute-force oracle or the
restatement's trace, so tests/test_gpu_decimate_edges.py sends the GPU only inputs that passed here."""
import functools

import numpy as np
import pytest

from tests import decimate_cases as C
from tests import decimate_reference as D
from tests import mc_reference as R


@functools.lru_cache(maxsize=None)
def _run(name):
    """(verts, faces, normals, info, trace) of the restatement on a case."""
    v, f, target, max_error, max_rounds = C.case(name)
    trace = []
    with np.errstate(invalid="ignore", over="ignore"):
        out = D.decimate(v, f, target, max_error, max_rounds, trace=trace)
    return (*out, tuple(trace))


def _restatement_locked(v, f):
    f = C.kept_faces(f)
    if len(f) == 0:                     # (the restatement runs no round then; every vertex is without a face)
        return np.ones(len(v), bool)
    fan, deg = D._fan(f, len(v))
    return D.vertex_status(f, fan, deg)[0]


@pytest.mark.parametrize("name", C.CASES)
def test_restatement_keeps_the_headers_promises(name):
    v, f, target, max_error, max_rounds = C.case(name)
    ov, of, on, info, trace = _run(name)
    C.check_properties(v, f, ov, of, info, target, max_rounds, C.marks(name)["end"])
    assert info["rounds"] == sum(1 for _, S, _ in trace if S) and info["collapses"] == sum(m for _, _, m in trace)
    assert len(on) == len(ov)
    assert set(C.marks(name)) >= {"end"} and name in C.CASES


@pytest.mark.parametrize("name", C.CASES)
def test_both_oracles_lock_the_same_vertices(name):
    v, f = C.case(name)[:2]
    if len(v) == 0:
        return
    assert np.array_equal(C.locked_vertices(len(v), C.kept_faces(f)), _restatement_locked(v, f))


def test_base_sphere_is_clean():
    v, f = C.sphere()
    assert (len(v), len(f)) == (312, 620) and R.is_closed_oriented_manifold(f)
    assert not C.locked_vertices(len(v), f).any()


# ---------------------------------------------------------------- topology
def _edge_counts(f, a, b):
    f = C.kept_faces(f)
    d = R.directed_edges(f)
    return int(((d[:, 0] == a) & (d[:, 1] == b)).sum()), int(((d[:, 0] == b) & (d[:, 1] == a)).sum())


def test_bowtie_pinch_is_locked_by_its_two_fans_alone():
    v, f = C.case("bowtie")[:2]
    p = C.marks("bowtie")["pinch"]
    assert R.is_closed_oriented_manifold(f)                     # every edge once each way: only the fan rule locks
    locked = C.locked_vertices(len(v), f)
    assert np.array_equal(np.nonzero(locked)[0], [p]) and _restatement_locked(v, f)[p]
    V0 = len(C.sphere()[0])
    around = f[(f == p).any(1)]
    assert (around[around != p] < V0).any() and (around[around != p] >= V0).any()      # faces of both spheres
    ov, of = _run("bowtie")[:2]
    assert (ov == v[p]).all(1).any()
    # the lock is all that holds it: its faces lie in one plane, and with the lock lifted by hand the cheapest candidate
    # of round 1 (the smallest key of all, which is always selected) is an edge at the pinch
    assert (v[np.unique(around), 0] == 0.5).all()
    f64 = C.kept_faces(f)
    fan, deg = D._fan(f64, len(v))
    lk, nxt = D.vertex_status(f64, fan, deg)
    lk[p] = False
    keys, _ = D.evaluate(v, f64, D.vertex_quadrics(v, f64), fan, deg, lk, nxt, np.inf)
    e = int(np.argmin(keys))
    assert keys[e] != D.KEY_NONE and p in (f64.reshape(-1)[e], np.roll(f64, -1, axis=1).reshape(-1)[e])


@pytest.mark.parametrize("name", ["fin", "dupface", "flipped"])
def test_non_manifold_corners_are_locked(name):
    v, f = C.case(name)[:2]
    corners = C.marks(name)["locked"]
    assert len(corners) == 3
    locked = C.locked_vertices(len(v), f)
    assert locked[corners].all() and _restatement_locked(v, f)[corners].all()
    a, b, c = corners
    if name == "fin":
        assert sorted(_edge_counts(f, a, b)) == [1, 2]          # the edge is in three faces
        assert _edge_counts(f, b, c) == (1, 0) and _edge_counts(f, c, a) == (1, 0)      # the fin's border
        assert c == len(v) - 1
    if name == "dupface":
        assert [_edge_counts(f, *e) for e in ((a, b), (b, c), (c, a))] == [(2, 1)] * 3
        assert int((f == [a, b, c]).all(1).sum()) == 2
    if name == "flipped":
        assert [_edge_counts(f, *e) for e in ((a, b), (b, c), (c, a))] == [(2, 0)] * 3
    # the run went on around them: they are in the output bit for bit, and the mesh did shrink to the target
    ov, of, _, info, _ = _run(name)
    for w in corners:
        assert (ov.view(np.uint32) == v[w].view(np.uint32)).all(1).any()
    assert info["collapses"] > 100


def test_mixed_holds_all_four_apart():
    v, f = C.case("mixed")[:2]
    m = C.marks("mixed")
    locked = C.locked_vertices(len(v), C.kept_faces(f))
    assert sorted(set(m["locked"])) == np.nonzero(locked)[0].tolist()
    assert np.array_equal(locked, _restatement_locked(v, f))
    # the one-rings of the four locked sets are disjoint
    rings = []
    for g in m["groups"]:
        rings.append(set(f[np.isin(f, g).any(1)].reshape(-1).tolist()))
    for i in range(4):
        for j in range(i):
            assert not rings[i] & rings[j]
    assert len(f) < 1500


# ---------------------------------------------------------------- input hygiene
def test_repeats_and_isolated_are_where_they_should_be():
    v, f = C.case("repeats+isolated")[:2]
    m = C.marks("repeats+isolated")
    rep = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])
    assert rep[0] and rep[-1] and rep[1:-1].any() and int(rep.sum()) == m["repeats"]
    assert (f[rep][:, 0] == f[rep][:, 1]).any() and (f[rep][:, 0] == f[rep][:, 2]).any()     # (a, a, b) and (a, b, a)
    unused = np.setdiff1d(np.arange(len(v)), f[~rep])
    assert unused.tolist() == m["isolated"] == [0, len(v) // 2, len(v) - 1]
    assert R.is_closed_oriented_manifold(f[~rep])
    # the clean sphere under other numbers: the same run, renumbered
    ov, of, on, info, _ = _run("repeats+isolated")
    sv, sf, sn, sinfo, _ = _run("targetodd")
    assert C.case("targetodd")[2] in (C.case("repeats+isolated")[2], C.case("repeats+isolated")[2] + 1)
    assert info == sinfo and np.array_equal(of, sf) and np.array_equal(ov.view(np.uint32), sv.view(np.uint32))


@pytest.mark.parametrize("name", ["alldegenerate", "nofaces", "nothing"])
def test_empty_after_hygiene(name):
    v, f, target = C.case(name)[:3]
    assert len(C.kept_faces(f)) == 0 and target == 0
    assert (len(f) > 0) == (name == "alldegenerate") and (len(v) > 0) == (name != "nothing")
    ov, of, on, info, trace = _run(name)
    assert ov.shape == (0, 3) and of.shape == (0, 3) and on.shape == (0, 3)
    assert info == {"rounds": 0, "collapses": 0} and trace == ()


# ---------------------------------------------------------------- numeric arms
def _areas2(v, f):
    p = v[C.kept_faces(f)].astype(np.float64)
    return np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)


def test_coincident_has_zero_area_faces_that_stay_flat():
    v, f = C.case("coincident")[:2]
    a, b = C.marks("coincident")["pair"]
    assert a != b and np.array_equal(v[a], v[b])
    assert int((_areas2(v, f) == 0).sum()) >= 2
    q = D.face_quadrics(v, C.kept_faces(f))
    assert int((q == 0).all(1).sum()) >= 2                       # the l == 0 quadric
    ov, of, _, info, _ = _run("coincident")
    assert info["collapses"] > 100
    # a flat face may go or stay flat, and no face may become flat (m . m' > 0 needs m' != 0): never more than before
    assert int((_areas2(ov, of) == 0).sum()) <= int((_areas2(v, f) == 0).sum())
    # the neighbourhood of the pair did not collapse as the clean sphere's does: the flat faces took part in round 1
    assert _run("coincident")[4][0] != _run("sphere")[4][0]


def test_nonfinite_stays_put_and_does_not_spread():
    v, f = C.case("nonfinite")[:2]
    i, j = C.marks("nonfinite")["bad"]
    assert np.isnan(v[i, 0]) and v[j, 1] == np.inf and int((~np.isfinite(v)).sum()) == 2
    assert not set(f[(f == i).any(1)].reshape(-1).tolist()) & set(f[(f == j).any(1)].reshape(-1).tolist())
    ov, of, on, info, _ = _run("nonfinite")
    bad = ~np.isfinite(ov).all(1)
    assert int(bad.sum()) == 2
    b0, b1 = np.nonzero(bad)[0]
    assert np.array_equal(ov[b0].view(np.uint32), v[i].view(np.uint32)) == (i < j)
    assert sorted([ov[b0].tobytes(), ov[b1].tobytes()]) == sorted([v[i].tobytes(), v[j].tobytes()])
    assert info["collapses"] > 100
    # and every face they had is still theirs: nothing next to a bad vertex collapsed
    for w_in, w_out in zip(sorted((i, j)), (b0, b1)):
        assert int((of == w_out).any(1).sum()) == int((f == w_in).any(1).sum())


def test_faraway_is_the_sphere_a_long_way_off():
    v, f = C.case("faraway")[:2]
    assert (np.abs(v).min(0) > [999, 1999, 499]).all() and np.array_equal(f, C.sphere()[1])
    ov, of, _, info, _ = _run("faraway")
    assert R.is_closed_oriented_manifold(of) and R.euler_characteristic(ov, of) == 2 and info["collapses"] == 155


# ---------------------------------------------------------------- control arms
def test_max_rounds_ends_the_run():
    F = len(C.sphere()[1])
    for name, k in (("rounds0", 0), ("rounds1", 1), ("rounds3", 3)):
        v, f, target, _, max_rounds = C.case(name)
        ov, of, _, info, trace = _run(name)
        assert max_rounds == k and info["rounds"] == k == len(trace) and len(of) > target
        assert all(S > 0 for _, S, _ in trace)                   # the limit, not an empty round, ended it
    assert len(_run("rounds0")[1]) == F and np.array_equal(_run("rounds0")[0], C.sphere()[0])
    assert len(_run("rounds3")[1]) < len(_run("rounds1")[1]) < F


def test_max_error_ends_the_run_above_the_target():
    v, f, target, max_error, max_rounds = C.case("ceiling")
    ov, of, _, info, trace = _run("ceiling")
    assert max_error == 1e-6 and target == 0
    assert len(of) > target and info["rounds"] < max_rounds
    assert trace[-1] == (len(of), 0, 0) and len(trace) == info["rounds"] + 1
    assert (len(of), info["rounds"]) == (332, 12)
    # without the ceiling the same mesh goes on: the ceiling is what stopped it
    assert len(_run("target0")[1]) < len(of)


def test_targets_land_exactly():
    F = len(C.sphere()[1])
    for name, target, m in (("target-1", F - 1, 1), ("target-3", F - 3, 2)):
        assert C.case(name)[2] == target
        ov, of, _, info, trace = _run(name)
        assert trace == ((F, 22, m),) and len(of) == F - 2 * m and info == {"rounds": 1, "collapses": m}
    assert C.case("targetodd")[2] % 2 == 1 and len(_run("targetodd")[1]) == C.case("targetodd")[2] - 1
    ov, of, _, info, trace = _run("target0")
    assert len(of) == 4 and trace[-1] == (4, 0, 0)               # a tetrahedron is where a sphere stops


# ---------------------------------------------------------------- the ranking round
@pytest.mark.parametrize("name", C.RANKING)
def test_ranking_round_selects_more_than_two_tiles(name):
    v, f, target, _, _ = C.case(name)
    S, m = C.marks(name)["S"], C.marks(name)["m"]
    ov, of, _, info, trace = _run(name)
    assert S == C.RANK_SELECTED > 2 * 256 and m == {"rank1": 1, "rank257": 257, "rankS-1": S - 1}[name]
    assert trace == ((len(f), S, m),)                            # round 1 is the ranking round, and the only one
    assert len(f) - 2 * S < target and len(of) == target and info == {"rounds": 1, "collapses": m}


def test_ranking_keeps_the_smallest_keys():
    """The m collapses of the ranking round are those of the m cheapest selected edges: the ranked runs nest."""
    v, f = C.case("rank1")[:2]
    moved = {}
    for name in C.RANKING:
        ov = _run(name)[0]
        moved[name] = set(C._rows(v)) - set(C._rows(ov))           # positions a collapse removed or moved
    assert moved["rank1"] < moved["rank257"] < moved["rankS-1"]


# ---------------------------------------------------------------- valence
@pytest.mark.parametrize("name", C.VALENCE)
def test_bipyramid_apexes_have_long_lists(name):
    v, f, target = C.case(name)[:3]
    n = C.marks(name)["apex_degree"]
    deg = np.bincount(f.reshape(-1))
    assert n in (70, 300) and deg[0] == deg[1] == n and (deg[2:] == 4).all() and len(f) == 2 * n
    assert n > 64 and (n > 256) == (name == "valence300")
    assert R.is_closed_oriented_manifold(f) and not C.locked_vertices(len(v), f).any()
    ov, of, _, info, _ = _run(name)
    assert target == 8 and len(of) == 8 and R.is_closed_oriented_manifold(of)


# ---------------------------------------------------------------- the oracle itself can fail
def test_property_oracle_rejects_broken_outputs():
    v, f, target, _, max_rounds = C.case("fin")
    ov, of, _, info, _ = _run("fin")
    C.check_properties(v, f, ov, of, info, target, max_rounds, "target")
    a = C.marks("fin")["locked"][0]
    j = int(np.nonzero((ov.view(np.uint32) == v[a].view(np.uint32)).all(1))[0][0])
    moved = ov.copy()
    moved[j, 0] = np.nextafter(moved[j, 0], np.float32(2))
    for bad_v, bad_f, bad_info in ((moved, of, info),                                   # a locked vertex moved one ulp
                                   (ov, of[:-1], info),                                 # a face missing
                                   (ov, of[::-1], info),                                # faces out of order
                                   (np.concatenate([ov, ov[:1]]), of, info),            # an unreferenced vertex
                                   (ov, of, dict(info, collapses=info["collapses"] + 1))):
        with pytest.raises(AssertionError):
            C.check_properties(v, f, bad_v, bad_f, bad_info, target, max_rounds, "target")
    with pytest.raises(AssertionError):
        C.check_properties(v, f, ov, of, info, target, max_rounds, "stuck")
