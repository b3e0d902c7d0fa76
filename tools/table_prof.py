"""Tuning aid: in-kernel cycle breakdown of the node-feature table's work items inside the plan launch (csrc/gemm_table.hpp).
Build with MEL_HIPCC_FLAGS="-DMEL_TABLE_PROF"."""
import ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from melissa_amd import _lib
net, venv, loop = bench.build_workload(torch.device("cuda", 0), 0, 1024, 50, "l_dgn", "round", False, 1)
lib = _lib.load()
fn = lib.mel_debug_table_prof
fn.argtypes = [C.c_void_p]
buf = (C.c_ulonglong * 8)()
loop.run(20)
fn(buf)
N = 20
loop.run(N)
fn(buf)
v = list(buf)
items = max(v[6], 1)
print("work items counted", v[6], "per step", v[6] / N)
names = ["start .. layer-0 block in LDS", "layer 1 products", "layer 1 rows to LDS / t_h0", "conv1 products", "conv1 epilogue", "whole work item"]
for i, name in enumerate(names):
    print(f"{name:32s} {v[i] / items:10.0f} cycles per work item  ({100.0 * v[i] / max(v[5], 1):5.1f} %)")
