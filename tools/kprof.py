"""Read (and zero) the in-kernel cycle counters of one profiler family (csrc/kprof.hpp) through mel_debug_prof_read."""
import ctypes as C, sys
from melissa_amd import _lib

FAMILIES = {"world": (0, "-DMEL_ENV_PROF"), "env": (1, "-DMEL_ENV_PROF"), "gemm": (2, "-DMEL_GEMM_PROF=<tag>"),
            "split": (3, "-DMEL_GEMM_PROF=99 -DMEL_SPLIT_PROF"), "ring": (4, "-DMEL_RING_PROF=<tag>"),
            "table": (5, "-DMEL_TABLE_PROF"), "att": (6, "-DMEL_ATT_PROF=<mode>"), "fin": (7, "-DMEL_FIN_PROF")}


def read(family: str) -> list[int]:
    index, flags = FAMILIES[family]
    fn = _lib.load().mel_debug_prof_read
    fn.argtypes, fn.restype = [C.c_int32, C.c_void_p, C.c_int32], C.c_int32
    buf = (C.c_ulonglong * 16)()
    n = fn(index, buf, len(buf))
    if n <= 0:
        sys.exit(f'this build does not contain {family}: rebuild with MEL_HIPCC_FLAGS="{flags}"')
    return list(buf)[:n]
