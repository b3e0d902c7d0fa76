"""Captured (HIP-graph) update time with the TD target and the TD loss as torch expressions (``fused_td`` off: the path every
fixed-updates run takes) and as one HIP launch each (on: mel_td_target / mel_td_loss) - 50 nodes, 512 envs, K = 32: l_dgn and
dgn_r at batch 32, l_dgn at batch 1024.  Both learners of a case are built once and timed in alternating blocks of back-to-back
replays (python tools/fused_td_time.py).
``--trace MODEL off|on UPDATES``: only UPDATES captured updates of MODEL at batch 32, to be started under ``rocprofv3 --kernel-trace
--stats``; the launches of one update are the difference of the call counts of two such runs divided by the difference of UPDATES."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from melissa_amd.collect import RoundLoop
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
from melissa_amd.replay import RoundReplay
from melissa_amd.train import build_network, policy_and_learner

N, ENVS, K, BLOCK, BLOCKS = 50, 512, 32, 100, 5


def captured_learner(model, batch, fused):
    torch.manual_seed(9)
    net = build_network(model, N, "cuda")
    policy_cls, learner_cls, neighbours = policy_and_learner(model)
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=500)
    venv = HipGraphVectorEnv(ENVS, N, graph_pool=synthetic_graph_pool(N, 64, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5000, construct_like_reference=False)
    replay = RoundReplay(ENVS, N, K, "cuda", neighbours=neighbours)
    loop = RoundLoop(venv, policy, seed=5000, eps=0.1, replay=replay)
    learner = learner_cls(policy, replay, batch_size=batch, n_step=4, gamma=0.99, seed=0, fused_td=fused)
    with torch.no_grad():
        loop.run(40)
    learner.capture()
    for _ in range(10):
        learner.step()
    torch.cuda.synchronize()
    return learner


def block_ms(learner, reps=BLOCK):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        loss = learner.step()["loss"]
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps * 1e3
    assert torch.isfinite(loss).all()
    return dt


if __name__ == "__main__":
    if "--trace" in sys.argv:
        model, switch, updates = sys.argv[sys.argv.index("--trace") + 1:][:3]
        learner = captured_learner(model, 32, switch == "on")
        block_ms(learner, int(updates))
        sys.exit(0)
    for model, batch in (("l_dgn", 32), ("dgn_r", 32), ("l_dgn", 1024)):
        sides = {False: captured_learner(model, batch, False), True: captured_learner(model, batch, True)}
        ms = {False: [], True: []}
        for _ in range(BLOCKS):                                # alternated: off, on, off, on, ...
            for fused in (False, True):
                ms[fused].append(block_ms(sides[fused]))
        for fused in (False, True):
            t = sorted(ms[fused])
            print(f"{model} batch {batch} fused_td {'on ' if fused else 'off'}: captured update {t[len(t) // 2]:.4f} ms median of {BLOCKS} blocks "
                  f"of {BLOCK} (min {t[0]:.4f}, max {t[-1]:.4f})", flush=True)
        off, on = sorted(ms[False])[BLOCKS // 2], sorted(ms[True])[BLOCKS // 2]
        spread = max(max(ms[s]) - min(ms[s]) for s in (False, True))
        print(f"{model} batch {batch}: on - off = {on - off:+.4f} ms ({(on - off) / off * 100:+.1f} %), largest spread of a side {spread:.4f} ms",
              flush=True)
        del sides
