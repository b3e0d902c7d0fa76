"""Cost of the per-step logger_stats pool in the mel_env_round launch.

Two identical L-DGN round loops (same seeds, same trajectory, eager launches) that differ only in
mel_env_batch.step_stats run in alternating blocks of rounds; the library's stage timer (mel_prof_*: HIP events on the
dispatches themselves) books every env-round launch of a block.  Reported: microseconds per launch, per block and over all
blocks, pool off and on.

    python tools/step_stats_time.py [--envs 1024] [--nodes 50] [--rounds 50] [--blocks 4]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from melissa_amd import _lib  # noqa: E402
from melissa_amd.collect import RoundLoop  # noqa: E402
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool  # noqa: E402
from melissa_amd.networks import LDGNNetwork  # noqa: E402
from melissa_amd.policy import DQNPolicy  # noqa: E402


def block_us(lib, loop, rounds):
    """`rounds` eager rounds under the stage timer -> (mean us of the env-round launch, launches)"""
    torch.cuda.synchronize()
    prof = lib.mel_prof_create(rounds * 24)
    lib.mel_prof_attach(prof)
    with torch.no_grad():
        loop.run(rounds)
    lib.mel_prof_attach(None)
    torch.cuda.synchronize()
    ms = (C.c_double * _lib.N_STAGES)()
    cnt = (C.c_int64 * _lib.N_STAGES)()
    lib.mel_prof_read(prof, ms, cnt)
    lib.mel_prof_destroy(prof)
    k = _lib.STAGE_NAMES.index("env_step")
    return ms[k] / cnt[k] * 1e3, int(cnt[k])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=50, help="rounds per block")
    ap.add_argument("--blocks", type=int, default=4)
    a = ap.parse_args()
    lib = _lib.load()
    n, B = a.nodes, a.envs
    graphs = synthetic_graph_pool(n, 16, first_seed=0)
    torch.manual_seed(0)
    net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]}),
                      device="cuda", backend="hip")
    loops = {}
    for name in ("off", "on"):
        venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=48,
                                 construct_like_reference=False)
        if name == "on":
            venv.enable_step_stats()
        loops[name] = RoundLoop(venv, DQNPolicy(net), seed=1, eps=0.0, use_graph=False)
        with torch.no_grad():
            loops[name].run(30)                 # past the first episodes: rounds of every kind in the timed blocks
    blocks = {name: [] for name in loops}
    for _ in range(a.blocks):
        for name, loop in loops.items():
            blocks[name].append(block_us(lib, loop, a.rounds)[0])
    out = dict(envs=B, nodes=n, rounds_per_block=a.rounds)
    for name, loop in loops.items():
        c = loop.counters()
        out[f"env_round_us_{name}"] = dict(blocks=[round(x, 2) for x in blocks[name]],
                                           mean=round(sum(blocks[name]) / len(blocks[name]), 2))
        out[f"decisions_{name}"], out[f"errors_{name}"] = c["decisions"], c["errors"]
    out["pool_rows"] = loops["on"].venv.read_step_stats()[0]
    out["pool_cost_us"] = round(out["env_round_us_on"]["mean"] - out["env_round_us_off"]["mean"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
