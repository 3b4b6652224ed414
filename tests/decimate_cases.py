"""Inputs for lnerf_decimate (include/lnerf_hip.h) that marching cubes never produces -- non-manifold, degenerate and
ragged meshes, the control arguments at their edges, the ranking round over more than one tile, vertex-to-face lists
longer than a workgroup -- and check_properties, an oracle written from the header text alone: it shares no code with
tests/decimate_reference.py, so a misreading that the kernel and its restatement have in common still shows.

case(name) -> (verts [V,3] f32, faces [F,3] int, target_faces, max_error, max_rounds), built with numpy only and
read-only (the tests share them); marks(name) -> what the case promises (vertex indices, the expected end of the run),
which tests/test_decimate_edges_cpu.py asserts before any of it goes to the GPU."""
import functools

import numpy as np

from tests import mc_reference as R

DEFAULT_ROUNDS = 128      # LNERF_DECIMATE_DEFAULT_ROUNDS
INF = float("inf")

# how a run ends: no round was needed, the target was reached (F_out = target or target - 1), max_rounds ran out, the
# max_error ceiling left nothing to select, or the topology did (locks, the link condition, the tetrahedron rule)
ENDS = ("none", "target", "max_rounds", "max_error", "stuck")


# ---------------------------------------------------------------- building blocks
@functools.lru_cache(maxsize=None)
def _mc_sphere(n, r=0.6):
    x = np.linspace(-1, 1, n, dtype=np.float32)
    X, Y, Z = np.meshgrid(x, x, x, indexing="ij")
    v, f, _ = R.marching_cubes((r - np.sqrt(X * X + Y * Y + Z * Z)).astype(np.float32), 0.0, (-1, -1, -1), (1, 1, 1))
    return v.astype(np.float32), f.astype(np.int32)


def sphere(n=14):
    """The base mesh: a closed marching-cubes sphere, every vertex used (n = 14: 312 vertices, 620 faces)."""
    v, f = _mc_sphere(n)
    return v.copy(), f.copy()


def _face_towards(v, f, d):
    """The face whose centroid lies furthest along d."""
    return int(np.argmax(v[f].astype(np.float64).mean(1) @ np.asarray(d, np.float64)))


def _vertex_towards(v, d):
    return int(np.argmax(v.astype(np.float64) @ np.asarray(d, np.float64)))


def _bowtie(v, f):
    """Two copies of (v, f) that share one vertex: the second is moved so that its -x pole lies on the first's +x pole
    and its pole index is replaced by the first's.  The pinch and all its neighbours are then put into the plane
    x = 0.5 exactly: the pinch's quadric is that one plane's, so each edge from it to a neighbour v costs 0 at v -- were
    the pinch not locked, one of its edges would be the cheapest collapse of round 1 and it would move or go.
    -> (verts, faces, pinch index, faces of the second copy from)."""
    V = len(v)
    p, q = _vertex_towards(v, (1, 0, 0)), _vertex_towards(v, (-1, 0, 0))
    v2 = np.delete(v + (v[p] - v[q]), q, axis=0)
    ren = np.arange(V) + V
    ren[q + 1:] -= 1
    ren[q] = p
    v, f = np.concatenate([v, v2]).astype(np.float32), np.concatenate([f, ren[f].astype(f.dtype)])
    v[:, 0] += np.float32(0.5) - v[p, 0]
    ring = np.unique(f[(f == p).any(1)])
    v[ring, 0] = 0.5
    ring2 = ring[ring >= V]                    # the second copy's neighbours mirror the first's: pull them half way in,
    v[ring2, 1:] = v[p, 1:] + np.float32(0.5) * (v[ring2, 1:] - v[p, 1:])    # so that moving the pinch onto one of
    #                                            them flattens or flips no face of either fan
    return v, f, p, len(f) // 2


def _add_fin(v, f, face):
    """One more triangle on the edge faces[face][0] -> faces[face][1], its third corner a new vertex (the last one)
    outside the surface; the fin goes into the middle of the face array.  -> (verts, faces, (a, b, c))."""
    a, b = int(f[face, 0]), int(f[face, 1])
    c = len(v)
    tip = (1.5 * 0.5 * (v[a].astype(np.float64) + v[b].astype(np.float64))).astype(np.float32)
    return np.concatenate([v, tip[None]]), np.insert(f, len(f) // 2, [a, b, c], axis=0), (a, b, c)


def _add_dup(f, face, at):
    """faces[face] listed a second time, at row `at` (after `face`, so `face` keeps its index)."""
    assert at > face
    return np.insert(f, at, f[face], axis=0), tuple(int(x) for x in f[face])


def _flip(f, face):
    f = f.copy()
    f[face] = f[face, ::-1]
    return f, tuple(int(x) for x in f[face])


def bipyramid(n):
    """Apexes 0 (top) and 1 (bottom) over a regular n-gon 2 .. n + 1, outward faces: 2 n faces, the apexes have n."""
    t = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0, 0, 1], [0, 0, -1]], np.stack([np.cos(t), np.sin(t), 0 * t], -1)]).astype(np.float32)
    i = np.arange(n)
    a, b = 2 + i, 2 + (i + 1) % n
    f = np.concatenate([np.stack([0 * i, a, b], -1), np.stack([0 * i + 1, b, a], -1)]).astype(np.int32)
    return v, f


RANK_LATTICE = 64         # round 1 of this sphere (6744 vertices, 13484 faces) selects RANK_SELECTED edges:
RANK_SELECTED = 568       # more than two tiles of k_dc_rank (the restatement's trace, asserted on the CPU)


# ---------------------------------------------------------------- the cases
def _build(name):
    """-> ((verts, faces, target_faces, max_error, max_rounds), marks)."""
    v, f = sphere()
    F = len(f)
    if name == "sphere":          # the control: nothing odd about it
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target")
    # ---- topology
    if name == "bowtie":
        v, f, p, _ = _bowtie(v, f)
        return (v, f, len(f) // 2, INF, DEFAULT_ROUNDS), dict(end="target", pinch=p, locked=[p])
    if name == "fin":
        v, f, abc = _add_fin(v, f, _face_towards(v, f, (0, 0, 1)))
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", locked=list(abc))
    if name == "dupface":
        k = _face_towards(v, f, (0, 0, 1))
        f, abc = _add_dup(f, k, F - 5)
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", locked=list(abc))
    if name == "flipped":
        f, abc = _flip(f, _face_towards(v, f, (0, 0, 1)))
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", locked=list(abc))
    if name == "mixed":
        # first sphere: pinch at +x, fin at -x; second sphere: pinch at its -x, duplicate at +x, flipped face at +y
        v0, f0 = v, f
        v, f, p, F2 = _bowtie(v0, f0)
        v, f, fin = _add_fin(v, f, _face_towards(v0, f0, (-1, 0, 0)))
        second = np.arange(len(f)) >= F2 + 1          # (the fin went into row (2 F) // 2 = F2, before the second copy)
        c2 = v[f].astype(np.float64).mean(1) - v[f[second]].astype(np.float64).mean((0, 1))
        kd = int(np.argmax(np.where(second, c2[:, 0], -np.inf)))
        kf = int(np.argmax(np.where(second, c2[:, 1], -np.inf)))
        f, flp = _flip(f, kf)
        f, dup = _add_dup(f, kd, len(f))
        return (v, f, len(f) // 2, INF, DEFAULT_ROUNDS), dict(end="target", pinch=p, locked=[p, *fin, *dup, *flp],
                                                            groups=[[p], list(fin), list(dup), list(flp)])
    # ---- input hygiene
    if name == "repeats+isolated":
        V = len(v)
        mid = V // 2
        ren = np.arange(V) + 1                      # unreferenced vertices at 0, mid + 1 and the end
        ren[mid:] += 1
        v = np.concatenate([[[9, 9, 9]], v[:mid], [[-9, 9, 0.5]], v[mid:], [[0, -9, 9]]]).astype(np.float32)
        f = ren[f].astype(np.int64)
        a, b, c, d = (int(x) for x in (f[0, 0], f[0, 1], f[F // 2, 0], f[F // 2, 2]))
        f = np.concatenate([[[a, a, b]], f[:F // 3], [[c, d, c]], f[F // 3:2 * F // 3], [[d, d, d], [b, a, a]],
                            f[2 * F // 3:], [[c, c, d], [a, b, a]]])
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", isolated=[0, mid + 1, V + 2], repeats=6)
    if name == "alldegenerate":
        v = np.arange(15, dtype=np.float32).reshape(5, 3) * np.float32(0.25)
        f = np.array([[0, 0, 1], [1, 2, 1], [3, 3, 3], [2, 4, 4], [4, 0, 4], [1, 1, 0]], np.int32)
        return (v, f, 0, INF, DEFAULT_ROUNDS), dict(end="none", repeats=6)
    if name == "nofaces":
        v = np.arange(21, dtype=np.float32).reshape(7, 3) * np.float32(0.5)
        return (v, np.zeros((0, 3), np.int32), 0, INF, DEFAULT_ROUNDS), dict(end="none")
    if name == "nothing":
        return (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0, INF, DEFAULT_ROUNDS), dict(end="none")
    # ---- numeric arms
    if name == "coincident":
        k = _face_towards(v, f, (0, 1, 0))
        a, b = int(f[k, 0]), int(f[k, 1])
        v[b] = v[a]
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", pair=(a, b))
    if name == "nonfinite":
        i, j = _vertex_towards(v, (0, 0, 1)), _vertex_towards(v, (0, 0, -1))
        v[i, 0] = np.nan
        v[j, 1] = np.inf
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target", bad=(i, j))
    if name == "faraway":
        v = v + np.float32([1000, -2000, 500])
        return (v, f, F // 2, INF, DEFAULT_ROUNDS), dict(end="target")
    # ---- control arms
    if name in ("rounds0", "rounds1", "rounds3"):
        k = int(name[-1])
        return (v, f, 0, INF, k), dict(end="max_rounds" if k else "none")
    if name == "ceiling":
        return (v, f, 0, 1e-6, DEFAULT_ROUNDS), dict(end="max_error")
    if name == "target-1":
        return (v, f, F - 1, INF, DEFAULT_ROUNDS), dict(end="target")
    if name == "target-3":
        return (v, f, F - 3, INF, DEFAULT_ROUNDS), dict(end="target")
    if name == "target0":
        return (v, f, 0, INF, DEFAULT_ROUNDS), dict(end="stuck")
    if name == "targetodd":
        return (v, f, 311, INF, DEFAULT_ROUNDS), dict(end="target")
    # ---- the ranking round: round 1 selects S edges and would pass the target, so only the m smallest keys collapse
    if name.startswith("rank"):
        v, f = _mc_sphere(RANK_LATTICE)
        v, f = v.copy(), f.copy()
        S = RANK_SELECTED
        m = {"rank1": 1, "rank257": 257, "rankS-1": S - 1}[name]
        return (v, f, len(f) - 2 * m, INF, DEFAULT_ROUNDS), dict(end="target", S=S, m=m)
    # ---- valence: lists longer than a wave (70) and than a workgroup (300)
    if name in ("valence70", "valence300"):
        v, f = bipyramid(int(name[7:]))
        return (v, f, 8, INF, DEFAULT_ROUNDS), dict(end="target", apex_degree=int(name[7:]))
    raise KeyError(name)


TOPOLOGY = ["bowtie", "fin", "dupface", "flipped", "mixed"]
HYGIENE = ["repeats+isolated", "alldegenerate", "nofaces", "nothing"]
NUMERIC = ["coincident", "nonfinite", "faraway"]
CONTROL = ["rounds0", "rounds1", "rounds3", "ceiling", "target-1", "target-3", "target0", "targetodd"]
RANKING = ["rank1", "rank257", "rankS-1"]
VALENCE = ["valence70", "valence300"]
CASES = ["sphere"] + TOPOLOGY + HYGIENE + NUMERIC + CONTROL + RANKING + VALENCE


@functools.lru_cache(maxsize=None)
def _cached(name):
    (v, f, target, max_error, max_rounds), m = _build(name)
    v, f = np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f)
    assert v.ndim == 2 and v.shape[1] == 3 and f.ndim == 2 and f.shape[1] == 3 and f.dtype.kind == "i"
    assert m["end"] in ENDS
    v.setflags(write=False)
    f.setflags(write=False)
    return (v, f, int(target), float(max_error), int(max_rounds)), m


def case(name):
    return _cached(name)[0]


def marks(name):
    return _cached(name)[1]


# ---------------------------------------------------------------- the property oracle (from the header, nothing else)
def _rows(a):
    """Each row's bit pattern as bytes (so NaN equals the same NaN and -0 differs from +0)."""
    a = np.ascontiguousarray(a)
    return [r.tobytes() for r in a]


def kept_faces(faces):
    """The faces that do not repeat an index ("faces that repeat an index are dropped first"), int64."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])]


def _edge_uses(faces):
    """{(a, b): the number of faces that hold the directed edge a -> b}."""
    uses = {}
    for a, b, c in np.asarray(faces).tolist():
        for e in ((a, b), (b, c), (c, a)):
            uses[e] = uses.get(e, 0) + 1
    return uses


def locked_vertices(n_verts, faces):
    """The header's locked set of `faces` (none repeating an index), by brute force: a vertex with no face, an end of an
    edge that is not in exactly one face each way round, a vertex whose faces are more than one fan.  Fans: a union-find
    over each vertex's corners that joins two faces of the vertex when they share an edge at it."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    locked = np.ones(n_verts, bool)
    locked[faces.reshape(-1)] = False                                   # no face
    uses = _edge_uses(faces)
    for (a, b), n in uses.items():
        if n != 1 or uses.get((b, a), 0) != 1:
            locked[a] = locked[b] = True
    parent = list(range(3 * len(faces)))                                # corner 3 f + k

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}                                                          # (w, x) -> a corner of w in a face holding x
    for i, face in enumerate(faces.tolist()):
        for k, w in enumerate(face):
            for x in face:
                if x != w:
                    j = first.setdefault((w, x), 3 * i + k)
                    parent[find(3 * i + k)] = find(j)
    fans = {}
    for i, face in enumerate(faces.tolist()):
        for k, w in enumerate(face):
            fans.setdefault(w, set()).add(find(3 * i + k))
    for w, roots in fans.items():
        if len(roots) != 1:
            locked[w] = True
    return locked


def component_euler(v, f):
    """Euler characteristic of every connected component, sorted."""
    f = np.asarray(f, np.int64)
    lab = np.arange(len(v))
    while True:
        m = lab[f].min(1)
        new = lab.copy()
        for j in range(3):
            np.minimum.at(new, f[:, j], m)
        new = new[new]
        if np.array_equal(new, lab):
            break
        lab = new
    chis = []
    for c in np.unique(lab[f[:, 0]]):
        fc = f[lab[f[:, 0]] == c]
        chis.append(R.euler_characteristic(v, fc))
    return sorted(chis)


def _is_subsequence(xs, ys):
    it = iter(ys)
    return all(any(x == y for y in it) for x in xs)


def _monotone_match(rows_in, rows_out):
    """The longest order-preserving matching of equal rows: match[j] = the input index of output row j, or -1.  (A
    longest common subsequence as a longest increasing subsequence: each output row lists the input indices with its
    bits in descending order.)"""
    import bisect
    where = {}
    for i, r in enumerate(rows_in):
        where.setdefault(r, []).append(i)
    tails, tail_node, nodes = [], [], []           # nodes: (input index, output index, previous node)
    for j, r in enumerate(rows_out):
        for i in reversed(where.get(r, ())):
            k = bisect.bisect_left(tails, i)
            nodes.append((i, j, tail_node[k - 1] if k else -1))
            if k == len(tails):
                tails.append(i)
                tail_node.append(len(nodes) - 1)
            else:
                tails[k] = i
                tail_node[k] = len(nodes) - 1
    match = -np.ones(len(rows_out), np.int64)
    n = tail_node[-1] if tail_node else -1
    while n >= 0:
        i, j, n = nodes[n]
        match[j] = i
    return match


def _edge_census(faces, locked):
    """Sorted [(uses of a -> b, uses of b -> a)] over the undirected edges whose two ends are locked; the number of
    border edges (one way round only); the number of edges in three or more faces; {k: directed edges used k times}
    for k != 1."""
    uses = _edge_uses(faces)
    both, border, many, hist = [], 0, 0, {}
    for (a, b), n in uses.items():
        r = uses.get((b, a), 0)
        if n != 1:
            hist[n] = hist.get(n, 0) + 1
        if a < b or r == 0:                                            # each undirected edge once
            border += (n == 0) != (r == 0)
            many += n + r >= 3
            if locked[a] and locked[b]:
                both.append((min(n, r), max(n, r)))
    return sorted(both), border, many, hist


def check_properties(verts_in, faces_in, verts_out, faces_out, stats, target_faces=None, max_rounds=None, end=None):
    """What the header of lnerf_decimate promises of any run, asserted on one: stats = {rounds, collapses}.  With
    target_faces, max_rounds and end (one of ENDS) also how the run ended.
      1. the locked set of the input, by brute force (locked_vertices)
      2. every locked input vertex that has a face is in the output, bit for bit, in input order
      3. no output face repeats an index, every output vertex is referenced, each collapse took one vertex away; the
         vertices no collapse moved are in their old order (at most `collapses` survivors moved, so an order-preserving
         matching of equal bit patterns misses no more than that), and the faces no collapse touched -- all three
         corners matched -- are all there, renumbered, in their old order
      4. F_out = F_kept - 2 collapses, and the end of the run
      5. the locked vertices of the output are those of the input; the edges between two locked vertices keep their use
         counts each way round; the numbers of border edges, of edges in three or more faces and of directed edges used
         k != 1 times are unchanged; so is the Euler characteristic of every component.
         (An edge with only ONE locked end can go: where two unlocked neighbours x, y of a locked w collapse, w-x and
         w-y become one edge, as along every open border.  Such edges are in exactly one face each way round, so the
         counts above lose nothing by leaving them out.)"""
    vi = np.ascontiguousarray(verts_in, np.float32).reshape(-1, 3)
    vo = np.ascontiguousarray(verts_out, np.float32).reshape(-1, 3)
    fi = kept_faces(faces_in)
    fo = np.asarray(faces_out, np.int64).reshape(-1, 3)
    rounds, collapses = int(stats["rounds"]), int(stats["collapses"])
    Vi, Vo = len(vi), len(vo)
    assert fo.size == 0 or (fo.min() >= 0 and fo.max() < Vo)

    # 1. the locked set of the input
    locked = locked_vertices(Vi, fi)
    has_face = np.zeros(Vi, bool)
    has_face[fi.reshape(-1)] = True
    rows_in, rows_out = _rows(vi), _rows(vo)

    # 2. locked vertices keep their exact positions (and their order)
    held = np.nonzero(locked & has_face)[0]
    assert _is_subsequence([rows_in[i] for i in held], rows_out), "a locked vertex moved or went"

    # 3. output hygiene: no repeated index, every vertex referenced, a collapse removes one vertex, order kept
    assert len(kept_faces(fo)) == len(fo), "an output face repeats an index"
    assert np.array_equal(np.unique(fo), np.arange(Vo)), "an output vertex is in no face"
    assert Vo == int(has_face.sum()) - collapses
    match = _monotone_match(rows_in, rows_out)
    assert int((match >= 0).sum()) >= Vo - collapses, "fewer vertices in their old order than collapses allow"
    # an input face whose three corners are all matched was touched by no collapse: it is still there, renumbered, and
    # those faces are in their old order
    out_of = -np.ones(Vi, np.int64)
    out_of[match[match >= 0]] = np.nonzero(match >= 0)[0]
    whole = (out_of[fi] >= 0).all(1) if len(fi) else np.zeros(0, bool)
    assert _is_subsequence(_rows(out_of[fi[whole]]), _rows(fo)), "untouched faces went or changed their order"

    # 4. the face count
    assert len(fo) == len(fi) - 2 * collapses
    assert (rounds == 0) == (collapses == 0)
    if end is not None:
        assert end in ENDS
        if end == "none":
            assert rounds == 0 and (len(fi) <= target_faces or max_rounds == 0)
        elif end == "target":
            assert len(fi) > target_faces and len(fo) in (target_faces, target_faces - 1) and 0 < rounds <= max_rounds
        elif end == "max_rounds":
            assert rounds == max_rounds and len(fo) > target_faces
        else:                                                          # a round selected nothing
            assert rounds < max_rounds and len(fo) > target_faces

    # 5. edge topology
    locked_out = locked_vertices(Vo, fo)
    assert _rows(vo[locked_out]) == [rows_in[i] for i in held], "the locked set changed"
    assert _edge_census(fi, locked) == _edge_census(fo, locked_out)
    assert component_euler(vo, fo) == component_euler(vi, fi)
