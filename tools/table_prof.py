"""Tuning aid: in-kernel cycle breakdown of the node-feature table's work items inside the plan launch (csrc/gemm_table.hpp).
Build with MEL_HIPCC_FLAGS="-DMEL_TABLE_PROF"."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import kprof
net, venv, loop = bench.build_workload(torch.device("cuda", 0), 0, 1024, 50, "l_dgn", "round", False, 1)
loop.run(20)
kprof.read("table")
N = 20
loop.run(N)
v = kprof.read("table")
items = max(v[6], 1)
print("work items counted", v[6], "per step", v[6] / N)
names = ["start .. layer-0 block in LDS", "layer 1 products", "layer 1 rows to LDS / t_h0", "conv1 products", "conv1 epilogue", "whole work item"]
for i, name in enumerate(names):
    print(f"{name:32s} {v[i] / items:10.0f} cycles per work item  ({100.0 * v[i] / max(v[5], 1):5.1f} %)")
