"""Captured (HIP-graph) update time at the learner leg's size - 50 nodes, 512 envs, batch 32: n_dgn_r against dgn_r (DGN-R network,
both with the sibling sum in its dense form) and hl_n_dgn_r against hl_dgn (HL-DGN network, DQN loss), alternated
(python tools/n_dgn_update_time.py)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from melissa_amd.collect import RoundLoop
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
from melissa_amd.replay import RoundReplay
from melissa_amd.train import build_network, policy_and_learner

N, ENVS, BATCH, REPS = 50, 512, 32, 50


def update_ms(model):
    torch.manual_seed(9)
    net = build_network(model, N, "cuda")
    policy_cls, learner_cls, neighbours = policy_and_learner(model)
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=500)
    venv = HipGraphVectorEnv(ENVS, N, graph_pool=synthetic_graph_pool(N, 64, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5000, construct_like_reference=False)
    replay = RoundReplay(ENVS, N, 32, "cuda", neighbours=neighbours)
    loop = RoundLoop(venv, policy, seed=5000, eps=0.1, replay=replay)
    learner = learner_cls(policy, replay, batch_size=BATCH, n_step=4, gamma=0.99, seed=0)
    with torch.no_grad():
        loop.run(40)
    learner.capture()
    for _ in range(5):
        learner.step()
    times = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = learner.step()["loss"]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(loss).all()
    times.sort()
    return times[len(times) // 2], times[len(times) // 10], times[-len(times) // 10 - 1]


if __name__ == "__main__":
    pairs = [("dgn_r", "n_dgn_r"), ("hl_dgn", "hl_n_dgn_r")]
    for rnd in range(2):                                   # alternated, twice
        for a, b in pairs:
            for m in (a, b):
                med, lo, hi = update_ms(m)
                print(f"round {rnd} {m}: captured update {med:.3f} ms (p10 {lo:.3f}, p90 {hi:.3f}) at batch {BATCH}", flush=True)
