"""Captured (HIP-graph) update time with the uniform and the prioritized replay at the learner leg's size - 50 nodes, 512 envs,
K = 32, batch 32 - for hl_dgn (DQN loss) and dgn_r (summed sibling Q), alternated twice (python tools/prio_update_time.py).
``--trace MODEL``: only a short prioritized run of MODEL, to be started under ``rocprofv3 --kernel-trace --stats`` for the three new
launches' own kernel time (replay_prio_refresh_kernel, replay_sample_prio_kernel, replay_prio_update_kernel)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from melissa_amd.collect import RoundLoop
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
from melissa_amd.replay import PrioritizedRoundReplay, RoundReplay
from melissa_amd.train import build_network, policy_and_learner

N, ENVS, K, BATCH, REPS = 50, 512, 32, 32, 50


def update_ms(model, prio, reps=REPS):
    torch.manual_seed(9)
    net = build_network(model, N, "cuda")
    policy_cls, learner_cls, neighbours = policy_and_learner(model)
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=500)
    venv = HipGraphVectorEnv(ENVS, N, graph_pool=synthetic_graph_pool(N, 64, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5000, construct_like_reference=False)
    replay = (PrioritizedRoundReplay if prio else RoundReplay)(ENVS, N, K, "cuda", neighbours=neighbours)
    loop = RoundLoop(venv, policy, seed=5000, eps=0.1, replay=replay)
    learner = learner_cls(policy, replay, batch_size=BATCH, n_step=4, gamma=0.99, seed=0)
    with torch.no_grad():
        loop.run(40)
    learner.capture()
    for _ in range(5):
        learner.step()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loss = learner.step()["loss"]
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    assert torch.isfinite(loss).all()
    times.sort()
    return times[len(times) // 2], times[len(times) // 10], times[-len(times) // 10 - 1]


if __name__ == "__main__":
    if "--trace" in sys.argv:
        update_ms(sys.argv[sys.argv.index("--trace") + 1], True, reps=20)
        sys.exit(0)
    for rnd in range(2):                                   # alternated, twice
        for model in ("hl_dgn", "dgn_r"):
            for prio in (False, True):
                med, lo, hi = update_ms(model, prio)
                print(f"round {rnd} {model} {'prioritized' if prio else 'uniform'}: captured update {med:.3f} ms "
                      f"(p10 {lo:.3f}, p90 {hi:.3f}) at batch {BATCH}", flush=True)
