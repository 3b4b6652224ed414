"""Host side of lnerf_grid_encode_forward's 32-bit addressing (csrc/grid_gather.hip): the kernel keeps sample indices
and byte offsets into a level's table in 32 bits, so the entry point refuses what does not fit BEFORE anything is
launched -- 2^31 samples or more, a level of more than 4 GiB.  No kernel runs here."""
import ctypes

from src.latent_nerf.raymarching import backend as B

P = ctypes.c_void_p


def _call(lib, m_host, rows_level1, table_dtype):
    offs = (ctypes.c_int32 * 3)(0, 64, 64 + rows_level1)
    sc = (ctypes.c_float * 2)(1.0, 2.0)
    rs = (ctypes.c_int32 * 2)(2, 3)
    return lib.lnerf_grid_encode_forward(P(16), 1.0, P(16), table_dtype, 2, 2, offs, sc, rs, m_host, None, m_host, P(16),
                                         B.BF16, 0, None)


def test_forward_refuses_what_32_bit_offsets_cannot_address(built_lib):
    lib = B.get_lib()
    assert _call(lib, 2 ** 31, 64, B.BF16) == -1 and b"m_host must be < 2^31" in lib.lnerf_last_error()
    assert _call(lib, 8, 2 ** 30 + 8, B.BF16) == -1 and b"level 1 is larger than 4 GiB" in lib.lnerf_last_error()
    assert _call(lib, 8, 2 ** 29 + 8, B.F32) == -1 and b"level 1 is larger than 4 GiB" in lib.lnerf_last_error()
    # nothing to do: OK without touching a pointer, whatever the table
    offs = (ctypes.c_int32 * 3)(0, 64, 128)
    sc = (ctypes.c_float * 2)(1.0, 2.0)
    rs = (ctypes.c_int32 * 2)(2, 3)
    assert lib.lnerf_grid_encode_forward(None, 1.0, None, B.BF16, 2, 2, offs, sc, rs, 0, None, 0, None, B.BF16, 0, None) == 0
