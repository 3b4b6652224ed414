"""The moment map's entry points (include/lnerf_hip.h, lnerf_moment_map_*), as far as they go without a GPU: exported,
declared and bound; the ABI number unchanged; every argument check in front of the launch; the switch between the
skipping and the all-groups form of the fused step."""
import ctypes
import re
import subprocess

from src.latent_nerf.raymarching import backend as B

NAMES = ("lnerf_moment_map_bytes", "lnerf_moment_map_build", "lnerf_moment_map_bind")
P = ctypes.c_void_p


def test_entry_points_are_exported_declared_and_bound(built_lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    exported = set(re.findall(r"\b(lnerf_[a-z0-9_]+)\b", out))
    declared = B.header_symbols()
    for name in NAMES:
        assert name in exported and name in declared and name in B._SIGNATURES, name
    lib = B.get_lib()
    assert lib.lnerf_abi_version() == B.ABI_VERSION == 7          # additive: the number stays
    assert lib.lnerf_moment_map_bytes.restype is ctypes.c_size_t


def test_map_size_follows_the_bucket_plan(built_lib):
    """256 bytes per bucket of 4096 rows, a level's last bucket may be partial; nothing for a table without a plan."""
    lib = B.get_lib()
    offs = (ctypes.c_int32 * 4)(0, 4920, 4920 + 8000, 4920 + 8000 + 8192)
    assert lib.lnerf_moment_map_bytes(3, offs) == (2 + 2 + 2) * 256
    assert lib.lnerf_moment_map_bytes(1, offs) == 2 * 256
    from src.latent_nerf.models.encoding import GridLevels
    lv = GridLevels()
    want = sum(-(-(b - a) // 4096) for a, b in zip(lv.offsets[:-1], lv.offsets[1:])) * 256
    assert lib.lnerf_moment_map_bytes(lv.num_levels, lv.c_offsets) == want
    assert lib.lnerf_moment_map_bytes(0, offs) == 0
    assert lib.lnerf_moment_map_bytes(33, offs) == 0
    assert lib.lnerf_moment_map_bytes(3, None) == 0
    big = (ctypes.c_int32 * 2)(0, 4096 * 257)                       # more buckets than a level may have
    assert lib.lnerf_moment_map_bytes(1, big) == 0


def test_build_and_bind_refuse_bad_arguments_before_any_launch(built_lib):
    """The pointers are made up: a call that got past its checks would need a GPU."""
    lib = B.get_lib()
    offs = (ctypes.c_int32 * 3)(0, 4920, 4920 + 8192)
    need = lib.lnerf_moment_map_bytes(2, offs)
    ok = P(4096)

    def build(m=ok, v=ok, levels=2, dim=2, o=offs, mp=ok, n=need):
        rc = lib.lnerf_moment_map_build(m, v, levels, dim, o, mp, n, None)
        return rc, lib.lnerf_last_error()

    for kw in (dict(m=None), dict(v=None), dict(mp=None)):
        rc, msg = build(**kw)
        assert rc == -1 and b"null pointer" in msg, kw
    rc, msg = build(dim=4)
    assert rc == -1 and b"level_dim" in msg
    rc, msg = build(levels=0)
    assert rc == -1 and b"bad level table" in msg
    rc, msg = build(o=None)
    assert rc == -1 and b"bad level table" in msg
    rc, msg = build(n=need - 1)
    assert rc == -1 and b"map too small" in msg
    rc, msg = build(m=P(4096 + 4))
    assert rc == -1 and b"aligned" in msg
    rc, msg = build(mp=P(4096 + 8))
    assert rc == -1 and b"aligned" in msg

    assert lib.lnerf_moment_map_bind(None, ok, need) == -1 and b"null exp_avg" in lib.lnerf_last_error()
    assert lib.lnerf_moment_map_bind(ok, ok, 0) == -1 and b"whole buckets" in lib.lnerf_last_error()
    assert lib.lnerf_moment_map_bind(ok, ok, need - 1) == -1 and b"whole buckets" in lib.lnerf_last_error()
    assert lib.lnerf_moment_map_bind(ok, P(4096 + 8), need) == -1 and b"aligned" in lib.lnerf_last_error()
    # a binding that is too short for the level table of a fused call is refused by that call, in front of its launches
    key = P(1 << 20)
    assert lib.lnerf_moment_map_bind(key, ok, 256) == 0
    try:
        sc = (ctypes.c_float * 2)(15.0, 31.0)
        rs = (ctypes.c_int32 * 2)(16, 32)
        rc = lib.lnerf_grid_encode_backward_adam(P(16), 1.0, P(16), B.F32, 2, 2, offs, sc, rs, 1024, None, 1024, P(16), 2, P(16),
                                                 1 << 30, P(16), key, P(16), None, 1e-3, 0.9, 0.99, 1e-15, 1, None, 1.0, None)
        assert rc == -1 and b"moment map is too small" in lib.lnerf_last_error()
    finally:
        assert lib.lnerf_moment_map_bind(key, None, 0) == 0          # a null map unbinds
    assert lib.lnerf_moment_map_bind(key, None, 0) == 0              # ... and unbinding twice is fine


def test_adam_skip_is_a_switch_of_set_tuning(built_lib):
    lib = B.get_lib()
    assert '"adam_skip"' in open(B.HEADER_PATH).read()
    try:
        assert lib.lnerf_set_tuning(b"adam_skip", 0) == 0
        assert lib.lnerf_set_tuning(b"adam_skip", 7) == 0           # any value is taken as on / off
    finally:
        assert lib.lnerf_set_tuning(b"adam_skip", 1) == 0
