"""Cost of the "mpr" scripted-agent heuristic in the env round (mel_env_round) and of mel_mpr_sets.

For N = 50 and 100 with 1024 envs, an L-DGN round loop (eager launches, greedy random-weight policy) runs in four
settings - no scripted agents; simple_broadcast at ratio 0.5; mpr at ratio 0.5; mpr at ratio 1.0 in testing mode - and
the library's stage timer (mel_prof_*: events on the dispatches themselves) books every env-round launch: mean
microseconds per round.  Then mel_mpr_sets on 1024 connected 50-node random geometric graphs (torch events, mean of 50).

    python tools/mpr_env_time.py [--rounds 60]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from melissa_amd import _lib  # noqa: E402
from melissa_amd.collect import RoundLoop, sample_episode_table  # noqa: E402
from melissa_amd.env import HipGraphVectorEnv, mpr_sets, synthetic_graph_pool  # noqa: E402
from melissa_amd.networks import LDGNNetwork  # noqa: E402
from melissa_amd.policy import DQNPolicy  # noqa: E402

SETTINGS = [("none", {}), ("simple_broadcast 0.5", dict(scripted_agents_ratio=0.5, heuristic="simple_broadcast")),
            ("mpr 0.5", dict(scripted_agents_ratio=0.5, heuristic="mpr")),
            ("mpr 1.0 testing", dict(scripted_agents_ratio=1.0, heuristic="mpr", is_testing=True, num_test_episodes=64))]


def env_round_us(n, B, kw, rounds, graphs):
    lib = _lib.load()
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=40,
                             construct_like_reference=False, **kw)
    net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]}),
                      device="cuda", backend="hip")
    episodes = max(8, rounds // 5)          # host-drawn table (one supply for all four settings: the device stream does not cover testing mode)
    loop = RoundLoop(venv, DQNPolicy(net), seed=1, eps=0.1, episodes=sample_episode_table(venv, episodes, 1))
    loop.run(10)
    torch.cuda.synchronize()
    prof = lib.mel_prof_create(rounds * 24)
    lib.mel_prof_attach(prof)
    loop.run(rounds)
    lib.mel_prof_attach(None)
    torch.cuda.synchronize()
    ms = (C.c_double * _lib.N_STAGES)()
    cnt = (C.c_int64 * _lib.N_STAGES)()
    lib.mel_prof_read(prof, ms, cnt)
    lib.mel_prof_destroy(prof)
    k = _lib.STAGE_NAMES.index("env_step")
    c = loop.counters()
    return dict(env_round_us=round(ms[k] / cnt[k] * 1e3, 2), launches=int(cnt[k]), decisions=c["decisions"],
                episodes=c["episodes"], errors=c["errors"])


def mpr_sets_us(n=50, G=1024, reps=50):
    hop = torch.stack([torch.from_numpy(g.one_hop.astype("uint64").view("int64")) for g in
                       synthetic_graph_pool(n, G, first_seed=0)]).cuda()
    for _ in range(5):
        mpr_sets(hop)
    lib = _lib.load()
    out = torch.empty_like(hop)
    stream = _lib.current_stream_ptr(hop.device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):                    # the launch alone (mpr_sets() also validates the adjacency on the device)
        _lib.check(lib.mel_mpr_sets(hop.data_ptr(), G, n, out.data_ptr(), stream))
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / reps * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--envs", type=int, default=1024)
    a = ap.parse_args()
    res = {}
    for n in (50, 100):
        graphs = synthetic_graph_pool(n, 16, first_seed=0)
        for name, kw in SETTINGS:
            res[f"n{n} {name}"] = env_round_us(n, a.envs, kw, a.rounds, graphs)
            print(f"n{n} {name}: {res[f'n{n} {name}']}", flush=True)
    res["mel_mpr_sets 1024 x 50 nodes us"] = mpr_sets_us()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
