"""Mesh cleaning without a GPU: the numpy restatement (tests/meshclean_reference.py) against known answers -- the
components of a volume with floaters, clean_mesh's keep rule, the filter, what Taubin smoothing does to a staircase
sphere that plain Laplacian smoothing does not -- and the plumbing: config fields and their validation, export_mesh's
argument checks, the host-side checks of the C entry points, and the wrappers' refusal of CPU tensors."""
import ctypes
import functools
import inspect
import types

import numpy as np
import pytest
import torch

from tests import mc_reference as R
from tests import meshclean_reference as M

BOX = (-1, -1, -1), (1, 1, 1)


@functools.lru_cache(maxsize=None)
def floaters():
    v, f, _ = R.marching_cubes(M.floaters_volume(), 0.0, *BOX)
    return v, f


@functools.lru_cache(maxsize=None)
def staircase():
    v, f, _ = R.marching_cubes(M.staircase_volume(), 0.5, *BOX)
    return v, f


def _radii(p):
    r = np.linalg.norm(np.asarray(p, np.float64), axis=1)
    return r.mean(), np.sqrt(((r - r.mean()) ** 2).mean())


def test_floaters_components_counts_and_boxes():
    """The numbers asserted here come from a run of this restatement (and agree with the figures the feature was
    specified with: 4548 faces in 6 components)."""
    v, f = floaters()
    c = M.components(v, f)
    assert (len(v), len(f)) == (2286, 4548) and c["components"] == 6 and c["referenced"] == 2286
    assert c["comp_faces"].tolist() == [8, 68, 3596, 108, 544, 224]
    assert c["vert_comp"].min() == 0 and np.array_equal(c["face_comp"], c["vert_comp"][f[:, 0]])
    # numbered by the smallest vertex: the first vertex of each component appears in ascending order
    first = [int(np.nonzero(c["vert_comp"] == k)[0][0]) for k in range(6)]
    assert first == sorted(first) and first[0] == 0
    for k in range(6):
        p = v[c["vert_comp"] == k]
        assert np.array_equal(c["comp_box"][k], np.concatenate([p.min(0), p.max(0)]))
    b = c["comp_box"].astype(np.float64)
    d = b[:, 3:] - b[:, :3]
    D = b[:, 3:].max(0) - b[:, :3].min(0)
    frac = np.sqrt((d * d).sum(1) / (D * D).sum())
    assert np.round(frac, 3).tolist() == [0.029, 0.075, 0.539, 0.091, 0.215, 0.129]
    # every face's three corners agree, and no face joins two components
    assert (c["vert_comp"][f] == c["face_comp"][:, None]).all()


def test_keep_rule_on_the_floaters():
    v, f = floaters()
    c = M.components(v, f)
    n, box = c["comp_faces"], c["comp_box"]
    # 108 faces pass min_faces = 100, but 0.091 of the diagonal fails min_diameter = 0.1
    assert M.keep_rule(n, box, 100, 0.1, 0).tolist() == [False, False, True, False, True, True]
    assert M.keep_rule(n, box, 100, 0.0, 0).tolist() == [False, False, True, True, True, True]
    assert M.keep_rule(n, box, 0, 0.1, 0).tolist() == [False, False, True, False, True, True]
    assert M.keep_rule(n, box, 0, 0.0, 1).tolist() == [False, False, True, False, False, False]
    assert M.keep_rule(n, box, 8, 0.05, 2).tolist() == [False, False, True, False, True, False]
    assert M.keep_rule(n, box, 0, 0.0, 0).all() and M.keep_rule(n, box, 0, 0.0, 9).all()
    assert not M.keep_rule(n, box, 4000, 0.0, 3).any()
    # ties go to the smaller id
    assert M.keep_rule([5, 7, 7, 7], np.tile(np.float32([0, 0, 0, 1, 1, 1]), (4, 1)), 0, 0.0, 2).tolist() == [False, True,
                                                                                                             True, False]
    from src.latent_nerf.raymarching.raymarching import component_keep
    for args in ((100, 0.1, 0), (0, 0.0, 1), (8, 0.05, 2), (0, 0.0, 0), (0, 1.0, 0), (68, 0.075, 3)):
        assert np.array_equal(component_keep(n, box, *args), M.keep_rule(n, box, *args)), args


def test_clean_keeps_order_and_reindexes():
    v, f = floaters()
    ov, of, src, info = M.clean(v, f, 100, 0.1, 0)
    assert info == dict(components=6, kept=3, faces_before=4548, faces_after=3596 + 544 + 224)
    assert sorted(M.components(ov, of)["comp_faces"].tolist()) == [224, 544, 3596]
    assert (np.diff(src) > 0).all() and np.array_equal(ov, v[src])
    keep = np.isin(M.components(v, f)["face_comp"], [2, 4, 5])
    assert np.array_equal(src[of], f[keep])
    assert M.clean(v, f, 0, 0.0, 1)[3]["faces_after"] == 3596
    # everything at 0: only the unreferenced vertices go
    v2 = np.concatenate([np.float32([[9, 9, 9]]), v, np.float32([[8, 8, 8]])])
    ov, of, src, info = M.clean(v2, f + 1, 0, 0.0, 0)
    assert np.array_equal(ov, v) and np.array_equal(of, f) and np.array_equal(src, np.arange(1, len(v) + 1))
    # a face that repeats an index still links its distinct vertices; unreferenced vertices are in no component
    c = M.components(np.zeros((6, 3), np.float32), [[4, 4, 1], [1, 3, 3]])
    assert c["vert_comp"].tolist() == [-1, 0, -1, 0, 0, -1] and c["comp_faces"].tolist() == [2] and c["referenced"] == 3
    e = M.components(np.zeros((3, 3), np.float32), np.zeros((0, 3), np.int64))
    assert e["components"] == 0 and e["vert_comp"].tolist() == [-1, -1, -1] and e["comp_box"].shape == (0, 6)
    with pytest.raises(ValueError):
        M.components(np.zeros((3, 3), np.float32), [[0, 1, 3]])


def test_taubin_smooths_the_staircase_without_shrinking_it():
    v, f = staircase()
    assert len(v) == 2592 and R.is_closed_oriented_manifold(f)
    m0, s0 = _radii(v)
    p, n = M.smooth(v, f, 10)
    m1, s1 = _radii(p)
    q, _ = M.smooth(v, f, 10, 0.5, 0.0)              # plain Laplacian
    m2, _ = _radii(q)
    print("rms %.5f -> %.5f, mean radius %+.5f (Taubin) %+.5f (Laplacian)" % (s0, s1, m1 - m0, m2 - m0))
    assert s1 <= 0.6 * s0
    assert abs(m1 - m0) < 0.002
    assert abs(m2 - m0) >= 5 * abs(m1 - m0)
    # outward unit normals
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-5 and (np.einsum("ij,ij->i", n, p) > 0).all()
    # on a closed manifold mesh the step is the uniform umbrella operator: neighbours counted twice
    nb = {}
    for a, b, c in f.tolist():
        for x, y in ((a, b), (b, c), (c, a)):
            nb.setdefault(x, set()).add(y)
            nb.setdefault(y, set()).add(x)
    one = M.smooth(v, f, 1, 0.5, 0.0)[0]
    for w in (0, 17, 2591):
        mean = v[sorted(nb[w])].astype(np.float64).mean(0)
        want = v[w] + 0.5 * (mean - v[w])
        assert np.abs(one[w] - want).max() < 1e-6
    # iterations = 0: the vertices themselves; a vertex in no face, or only in faces that repeat an index, stays
    z, zn = M.smooth(v, f, 0)
    assert np.array_equal(z, v) and np.array_equal(zn, M.normals(v, f))
    v3 = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [7, 7, 7]])
    f3 = np.int32([[0, 1, 2], [3, 3, 0]])
    s3, n3 = M.smooth(v3, f3, 2)
    assert np.array_equal(s3[3:], v3[3:]) and not np.array_equal(s3[:3], v3[:3]) and np.array_equal(n3[3:], np.zeros((2, 3)))
    inc, deg = M.incidences(f3, 5)
    assert deg.tolist() == [1, 1, 1, 0, 0] and inc[:3, 0].tolist() == [0, 1, 2]
    for bad in ((1001, 0.5, -0.53), (1, 0.0, -0.53), (1, 1.5, -0.53), (1, 0.5, 0.1), (1, 0.5, -2.0), (-1, 0.5, -0.53)):
        with pytest.raises(ValueError):
            M.smooth(v3, f3, *bad)


def test_config_fields_and_validation():
    from src.latent_nerf.configs.train_config import TrainConfig, apply_overrides
    log = TrainConfig().log
    assert (log.mesh_min_component_faces, log.mesh_min_component_diameter, log.mesh_keep_largest,
            log.mesh_smooth_iterations) == (0, 0.0, 0, 0)
    cfg = apply_overrides(TrainConfig(), {"log.mesh_min_component_faces": "8", "log.mesh_min_component_diameter": "0.05",
                                          "log.mesh_keep_largest": "2", "log.mesh_smooth_iterations": "10"})
    assert (cfg.log.mesh_min_component_faces, cfg.log.mesh_min_component_diameter, cfg.log.mesh_keep_largest,
            cfg.log.mesh_smooth_iterations) == (8, 0.05, 2, 10)
    for key, bad in (("mesh_min_component_faces", -1), ("mesh_min_component_diameter", -0.1),
                     ("mesh_min_component_diameter", 1.5), ("mesh_keep_largest", -2), ("mesh_smooth_iterations", -1)):
        cfg = TrainConfig()
        setattr(cfg.log, key, bad)
        with pytest.raises(ValueError, match="log." + key):
            cfg.__post_init__()


def test_export_mesh_arguments_are_checked_before_any_gpu_work():
    from src.latent_nerf.models.renderer import NeRFRenderer
    from src.latent_nerf.training.trainer import Trainer
    par = inspect.signature(NeRFRenderer.export_mesh).parameters
    assert [par[k].default for k in ("min_component_faces", "min_component_diameter", "keep_largest",
                                     "smooth_iterations")] == [0, 0.0, 0, 0]
    nobody = types.SimpleNamespace()          # the checks come before the first use of the model
    for kw in (dict(min_component_faces=-1), dict(keep_largest=-1), dict(min_component_diameter=-0.5),
               dict(min_component_diameter=1.01), dict(min_component_diameter=float("nan")),
               dict(smooth_iterations=-1), dict(smooth_iterations=1001)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            NeRFRenderer.export_mesh(nobody, "unused", **kw)
    src = inspect.getsource(Trainer.full_eval)
    for key in ("mesh_min_component_faces", "mesh_min_component_diameter", "mesh_keep_largest", "mesh_smooth_iterations"):
        assert key in src


def test_entry_points_check_their_arguments_on_the_host(built_lib):
    from src.latent_nerf.raymarching import backend as B
    lib = B.get_lib()
    P = ctypes.c_void_p
    ok = P(4096)
    assert (B.MESH_MAX_ROUNDS, B.MESH_MAX_FACES, B.SMOOTH_MAX_ITER) == (256, 1 << 28, 1000)
    header = open(B.HEADER_PATH).read()
    for line in ("#define LNERF_MESH_MAX_ROUNDS 256", "#define LNERF_MESH_JUMP_HOPS 4", "#define LNERF_SMOOTH_MAX_ITER 1000",
                 "#define LNERF_MESH_MAX_FACES (1 << 28)", "#define LNERF_SMOOTH_LAMBDA 0.5f", "#define LNERF_SMOOTH_MU (-0.53f)"):
        assert line in header
    assert (B.SMOOTH_LAMBDA, B.SMOOTH_MU) == (0.5, -0.53)
    for fn in (lib.lnerf_mesh_components_scratch_bytes, lib.lnerf_mesh_filter_scratch_bytes,
               lib.lnerf_mesh_smooth_scratch_bytes):
        assert fn(1000, 2000) > 0 and fn(0, 0) > 0
        assert fn(-1, 5) == 0 and fn(5, -1) == 0 and fn(5, (1 << 28) + 1) == 0
    nb = lib.lnerf_mesh_smooth_scratch_bytes(8, 4)

    def smooth(it=1, lam=0.5, mu=-0.53, scratch=ok, nbytes=nb, out=P(8192)):
        rc = lib.lnerf_mesh_smooth(ok, 8, ok, 4, it, lam, mu, scratch, nbytes, out, None, None)
        return rc, lib.lnerf_last_error()

    for kw, word in ((dict(it=-1), b"iterations"), (dict(it=1001), b"iterations"), (dict(lam=0.0), b"lambda"),
                     (dict(lam=1.25), b"lambda"), (dict(lam=float("nan")), b"lambda"), (dict(mu=0.01), b"mu"),
                     (dict(mu=-1.75), b"mu"), (dict(mu=float("nan")), b"mu"), (dict(nbytes=16), b"scratch"),
                     (dict(scratch=P(4096 + 4)), b"aligned"), (dict(out=ok), b"verts_out")):
        rc, msg = smooth(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    rc = lib.lnerf_mesh_filter(ok, 8, 4, ok, ok, 16, ok, ok, ok, None)
    assert rc == -1 and b"scratch" in lib.lnerf_last_error()
    rc = lib.lnerf_mesh_components_finish(ok, 8, ok, 4, ok, ok, 16, ok, ok, ok, ok, ok, None)
    assert rc == -1 and b"scratch" in lib.lnerf_last_error()
    rc = lib.lnerf_mesh_components_begin(ok, -1, 4, ok, ok, None)
    assert rc == -1 and b"out of range" in lib.lnerf_last_error()
    rc = lib.lnerf_mesh_components_round(ok, 8, 4, ok, None, None)
    assert rc == -1 and b"null" in lib.lnerf_last_error()


def test_wrappers_refuse_cpu_tensors_and_bad_arguments(built_lib):
    import src.latent_nerf.raymarching as rm
    v, f = torch.zeros(4, 3), torch.tensor([[0, 1, 2], [1, 2, 3]])
    for op in (lambda: rm.mesh_components(v, f), lambda: rm.clean_mesh(v, f), lambda: rm.smooth_mesh(v, f, 1),
               lambda: rm.mesh_filter(v, f, torch.ones(2, dtype=torch.bool))):
        with pytest.raises(ValueError, match="no CPU path"):
            op()
    for kw in (dict(min_faces=-1), dict(keep_largest=-1), dict(min_diameter=-0.1), dict(min_diameter=2.0)):
        with pytest.raises(ValueError, match="clean_mesh"):
            rm.clean_mesh(v, f, **kw)
    for args in ((-1,), (1001,), (1, 0.0), (1, 1.5), (1, 0.5, 0.5), (1, 0.5, -1.6)):
        with pytest.raises(ValueError, match="smooth_mesh"):
            rm.smooth_mesh(v, f, *args)
    with pytest.raises(ValueError, match=r"\[V,3\]"):
        rm.mesh_components(torch.zeros(4, 2), f)
