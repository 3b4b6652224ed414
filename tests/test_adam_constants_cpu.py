"""The constants record's entry points (include/lnerf_hip.h, lnerf_adam_constants_*), as far as they go without a GPU:
exported, argument checks, the registry, the form switch.  No kernel is launched: every pointer here is made up."""
import ctypes

from src.latent_nerf.raymarching import backend as B

P = ctypes.c_void_p


def test_bind_and_unbind_check_their_arguments(built_lib):
    lib = B.get_lib()
    key, rec = P(1 << 20), P(4096)
    assert lib.lnerf_adam_constants_bind(None, 0.9, 0.99, rec) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert lib.lnerf_adam_constants_bind(key, 0.9, 0.99, None) == -1 and b"null pointer" in lib.lnerf_last_error()
    assert lib.lnerf_adam_constants_bind(key, 1.0, 0.99, rec) == -1 and b"betas must be in [0,1)" in lib.lnerf_last_error()
    assert lib.lnerf_adam_constants_bind(key, 0.9, -0.1, rec) == -1 and b"betas must be in [0,1)" in lib.lnerf_last_error()
    assert lib.lnerf_adam_constants_bind(key, 0.9, 0.99, P(4096 + 8)) == -1 and b"16-byte aligned" in lib.lnerf_last_error()
    assert lib.lnerf_adam_constants_unbind(None) == -1 and b"null counter" in lib.lnerf_last_error()
    try:
        assert lib.lnerf_adam_constants_bind(key, 0.9, 0.99, rec) == 0
        assert lib.lnerf_adam_constants_bind(key, 0.8, 0.9, rec) == 0       # binding again replaces
    finally:
        assert lib.lnerf_adam_constants_unbind(key) == 0
    assert lib.lnerf_adam_constants_unbind(key) == 0                        # ... and unbinding twice is fine


def test_the_record_size_and_the_switch_are_in_the_header(built_lib):
    lib = B.get_lib()
    header = open(B.HEADER_PATH).read()
    assert "#define LNERF_ADAM_CONSTANTS_BYTES %d" % B.ADAM_CONSTANTS_BYTES in header
    assert '"adam_consts"' in header
    try:
        assert lib.lnerf_set_tuning(b"adam_consts", 0) == 0
        assert lib.lnerf_set_tuning(b"adam_consts", 7) == 0                 # any value is taken as on / off
    finally:
        assert lib.lnerf_set_tuning(b"adam_consts", 1) == 0
