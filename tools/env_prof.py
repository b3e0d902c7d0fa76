"""Tuning aid: in-kernel cycle breakdown of env_round_kernel over a few round steps of the bench workload.
Build with MEL_HIPCC_FLAGS="-DMEL_ENV_PROF"."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
import kprof
net, venv, loop = bench.build_workload(torch.device("cuda", 0), 0, 1024, 50, "l_dgn", "round", False, 1)
loop.run(20)
kprof.read("env")
loop.run(40)
v = kprof.read("env")
w = max(v[7], 1)
print("wavefronts sampled", v[7], "loop iterations per env round", v[8] / w)
names = ["state load", "round loop", "  env_step with the world step", "  other env_step calls", "  env_observe", "  episode end (log + reset)", "state store"]
for i, name in enumerate(names):
    print(f"{name:34s} {v[i] / w:9.0f} cycles per env round")
kprof.read("world")
loop.run(20)
wb = kprof.read("world")
c = max(wb[3], 1)
print(f"world step (sample of {wb[3]} calls): relay + scripted {wb[0] / c:.0f}, move + all-pairs edges {wb[1] / c:.0f}, two-hop masks {wb[2] / c:.0f} cycles")
