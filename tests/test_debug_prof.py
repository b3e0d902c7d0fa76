"""CPU-side check of the tuning-aid export: the default build instruments no kernel family, says so, and no longer carries
the per-family exports that mel_debug_prof_read replaced."""
import ctypes as C

from melissa_amd import _lib

FAMILIES = range(8)             # KprofFamily, csrc/kprof.hpp
REMOVED = ["mel_debug_world_prof", "mel_debug_env_prof", "mel_debug_gemm_prof", "mel_debug_split_prof", "mel_debug_ring_prof",
           "mel_debug_table_prof", "mel_debug_att_prof", "mel_debug_fin_prof"]


def test_default_build_has_no_profiler_family():
    lib = _lib.load()
    fn = lib.mel_debug_prof_read
    fn.argtypes, fn.restype = [C.c_int32, C.POINTER(C.c_ulonglong), C.c_int32], C.c_int32
    sentinel = 0xA5A5A5A5A5A5A5A5
    for family in FAMILIES:
        out = (C.c_ulonglong * 16)(*([sentinel] * 16))
        assert fn(family, out, 16) == 0, family
        assert list(out) == [sentinel] * 16, family
    out = (C.c_ulonglong * 16)(*([sentinel] * 16))
    assert fn(99, out, 16) == -1
    assert list(out) == [sentinel] * 16
    for name in REMOVED:
        assert not hasattr(lib, name), name
