"""env_round_kernel with the replay's neighbour masks off and on (mel_round_replay.active_nb), in one process, alternated in
blocks of rounds - 1024 envs x 50 nodes, L-DGN forward, eager launches:

    rocprofv3 --kernel-trace --stats -d OUT -o t --output-format csv -- python tools/env_nb_prof.py
    python tools/env_nb_prof.py --parse OUT        # per-variant average of the env_round_kernel dispatches

Block i of BLOCK rounds runs with the masks off when i is even, on when i is odd (after WARM untraced-for-the-average rounds)."""
import glob
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, ENVS, WARM, BLOCK, BLOCKS = 50, 1024, 30, 20, 10


def run():
    import torch
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.replay import RoundReplay
    from melissa_amd.train import build_network
    torch.manual_seed(9)
    net = build_network("l_dgn", N, "cuda")
    venv = HipGraphVectorEnv(ENVS, N, graph_pool=synthetic_graph_pool(N, 64, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5000, construct_like_reference=False)
    replay = RoundReplay(ENVS, N, 64, "cuda", neighbours=True)
    loop = RoundLoop(venv, DQNPolicy(net), seed=5000, eps=0.1, replay=replay)
    on = replay.struct.active_nb
    with torch.no_grad():
        loop.run(WARM)
        for blk in range(BLOCKS):
            replay.struct.active_nb = on if blk % 2 else None
            loop.run(BLOCK)
    torch.cuda.synchronize()
    print({"errors": loop.counters()["errors"], "rounds": WARM + BLOCK * BLOCKS})


def parse(out_dir):
    import csv
    paths = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert paths, f"no kernel trace under {out_dir}"
    rows = []
    for p in paths:
        with open(p) as f:
            rows += [r for r in csv.DictReader(f) if "env_round_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) >= WARM + BLOCK * BLOCKS, len(rows)
    us = {0: [], 1: []}
    for i, r in enumerate(rows[-BLOCK * BLOCKS:]):             # the timed blocks are the last launches
        us[(i // BLOCK) % 2].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k, name in ((0, "active_nb off"), (1, "active_nb on")):
        v = sorted(us[k])
        print(f"{name}: {len(v)} launches, mean {sum(v) / len(v):.2f} us, median {v[len(v) // 2]:.2f} us")


if __name__ == "__main__":
    if "--parse" in sys.argv:
        parse(sys.argv[sys.argv.index("--parse") + 1])
    else:
        run()
