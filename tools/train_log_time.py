"""Cost of the training log (melissa_amd/train_log.py): the launch behind every env round and the launches in front of Adam.

An L-DGN round loop (replayed from HIP graphs of --graph-rounds rounds) is built with and without ``train_log`` in alternation,
anew for every block - same seeds, same trajectory, the same rounds timed - and a block is timed on the host between two
synchronisations.  Then the captured l_dgn update (batch 32) with and without the update launch, the same way.  Reported per
variant: the median of the blocks with their minimum and maximum, in microseconds per round / per update, and the difference of
the medians.

    python tools/train_log_time.py [--envs 1024] [--nodes 50] [--rounds 200] [--updates 100] [--blocks 5] [--out FILE]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from melissa_amd.collect import RoundLoop  # noqa: E402
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool  # noqa: E402
from melissa_amd.policy import DQNPolicy  # noqa: E402
from melissa_amd.replay import DQNLearner, RoundReplay  # noqa: E402
from melissa_amd.train import build_network  # noqa: E402
from melissa_amd.train_log import TrainLog  # noqa: E402


def timed(fn, count):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(count)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / count * 1e6


def summary(blocks):
    return dict(median=round(statistics.median(blocks), 2), min=round(min(blocks), 2), max=round(max(blocks), 2),
                blocks=[round(x, 2) for x in blocks])


def make(n, B, log, graph_rounds, learner=False):
    torch.manual_seed(0)
    net = build_network("l_dgn", n, torch.device("cuda"))
    venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 16, first_seed=0), dynamic_graph=True, device="cuda",
                             max_moves=48, construct_like_reference=False)
    tl = None
    if log:
        tl = TrainLog(venv, interval=1000, capacity=128)
        tl.arm(0)
        tl.drained_upto.fill_(2 ** 62)          # (nothing is drained here: a wrapping ring is then no loss)
    replay = RoundReplay(B, n, 16, "cuda") if learner else None
    policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3)) if learner else DQNPolicy(net)
    loop = RoundLoop(venv, policy, seed=1, eps=0.05, use_graph=True, graph_rounds=graph_rounds, replay=replay, train_log=tl)
    with torch.no_grad():
        loop.run(2 + 8 * graph_rounds)           # warm-up, both captures, past the first episodes
    if not learner:
        return loop, None, tl
    L = DQNLearner(policy, replay, batch_size=32, n_step=4, gamma=0.99, seed=0, fused_td=True, train_log=tl)
    L.capture()
    return loop, L, tl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=200, help="rounds per block")
    ap.add_argument("--updates", type=int, default=100, help="updates per block (0: skip the update half)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--graph-rounds", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = dict(envs=a.envs, nodes=a.nodes, rounds_per_block=a.rounds, updates_per_block=a.updates, graph_rounds=a.graph_rounds)

    def rounds_of(loop):
        def run(count):
            with torch.no_grad():
                loop.run(count)
        return run

    # one loop alive at a time, built anew for every block: both variants then time the SAME rounds of the same trajectory (two
    # loops alive side by side do not walk the trajectory either walks alone, log or no log)
    blocks, decisions = {"off": [], "on": []}, {"off": [], "on": []}
    for _ in range(a.blocks):
        for name in ("off", "on"):
            loop, _, tl = make(a.nodes, a.envs, name == "on", a.graph_rounds)
            blocks[name].append(timed(rounds_of(loop), a.rounds))
            c = loop.counters()
            decisions[name].append(c["decisions"])
            out[f"errors_{name}"] = c["errors"]
            if tl is not None:
                out["log_counters"] = tl.read_counters()
                out["log_slots_used"] = int((tl.interval_id >= 0).sum().item())
            del loop, tl
            gc.collect()
    for name in blocks:
        out[f"round_us_{name}"] = summary(blocks[name])
    out["decisions_per_block"], out["same_trajectory"] = decisions["off"][0], decisions["off"] == decisions["on"]
    out["round_cost_us"] = round(out["round_us_on"]["median"] - out["round_us_off"]["median"], 2)
    out["round_spread_us"] = round(max(out[f"round_us_{k}"]["max"] - out[f"round_us_{k}"]["min"] for k in ("off", "on")), 2)
    if a.updates > 0:
        # the update at the small size whatever --envs is: its cost does not depend on the env batch
        ublocks = {"off": [], "on": []}
        for _ in range(a.blocks):
            for name in ("off", "on"):
                loop, L, tl = make(20, 40, name == "on", a.graph_rounds, learner=True)
                ublocks[name].append(timed(lambda count: [L.step() for _ in range(count)], a.updates))
                del loop, L, tl
                gc.collect()
        for name in ublocks:
            out[f"update_us_{name}"] = summary(ublocks[name])
        out["update_cost_us"] = round(out["update_us_on"]["median"] - out["update_us_off"]["median"], 2)
        out["update_spread_us"] = round(max(out[f"update_us_{k}"]["max"] - out[f"update_us_{k}"]["min"] for k in ("off", "on")), 2)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
