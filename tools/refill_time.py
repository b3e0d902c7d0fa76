"""A round loop on the device episode stream, to be traced for the cost of a refill (episode_draw / fill / publish kernels):

    rocprofv3 --kernel-trace --stats -d OUT -o t --output-format csv -- python tools/refill_time.py [--ratio 0.5 --heuristic mpr]

1024 envs x 50 nodes, ring 16 (a refill every 7 rounds on the side stream), L-DGN, eps 0.1, rounds replayed from HIP graphs.
With ``--ratio`` > 0 the env generator also draws the scripted set of every episode (one thread per env, ~2 k bounded draws per
episode).  Prints one JSON line: decisions, episodes, error flags, refills."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from melissa_amd.collect import RoundLoop  # noqa: E402
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool  # noqa: E402
from melissa_amd.networks import LDGNNetwork  # noqa: E402
from melissa_amd.policy import DQNPolicy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--ring", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=700)
    ap.add_argument("--ratio", type=float, default=0.0)
    ap.add_argument("--heuristic", default=None)
    a = ap.parse_args()
    kw = dict(scripted_agents_ratio=a.ratio, heuristic=a.heuristic) if a.ratio > 0 else {}
    venv = HipGraphVectorEnv(a.envs, a.nodes, graph_pool=synthetic_graph_pool(a.nodes, 16, first_seed=0), dynamic_graph=True,
                             device="cuda", max_moves=48, construct_like_reference=False, **kw)
    torch.manual_seed(1)
    net = LDGNNetwork(5, 128, 2, 4, a.nodes, dueling_param=({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]}),
                      device="cuda", backend="hip")
    loop = RoundLoop(venv, DQNPolicy(net), seed=1, eps=0.1, ring=a.ring, use_graph=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    loop.run(64)
    e0.record()
    loop.run(a.rounds)
    e1.record()
    torch.cuda.synchronize()
    c = loop.counters()
    print(json.dumps(dict(nodes=a.nodes, envs=a.envs, ring=a.ring, ratio=a.ratio, heuristic=a.heuristic, rounds=a.rounds,
                          ms_per_round=round(e0.elapsed_time(e1) / a.rounds, 4), decisions=c["decisions"],
                          episodes=c["episodes"], errors=c["errors"], supply=loop.supply.describe())))


if __name__ == "__main__":
    main()
