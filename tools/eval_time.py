"""Wall time of ONE evaluation of ``test_num = 100`` episodes as ``train --epoch`` runs it (``melissa_amd.train._evaluate`` /
``_evaluate_spread``: env construction, episode supply, the rounds, the read of the episode log - a host clock around work that
ends in a synchronising read), l_dgn at 20 and at 50 nodes, three paths alternated in one process:

    test_envs = 1      one env, a host-drawn episode table, eager rounds (the path as it was)
    test_envs = 10     ten envs share the list, drawn on the device, rounds replayed from a HIP graph
    test_envs = 100    one episode per env

One untimed repeat per path, then five timed ones each; median and min - max per path, and each difference next to the largest
spread of a side.  Then the set-up share of the new path, phase by phase (python tools/eval_time.py).
``--trace N ENVS``: one spread evaluation only, to be started under ``rocprofv3 --kernel-trace --stats`` (the refill's kernels are
episode_draw_kernel / episode_fill_kernel / episode_publish_kernel)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from melissa_amd.collect import Collector
from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
from melissa_amd.policy import DQNPolicy
from melissa_amd.train import _evaluate, _evaluate_spread, build_network

TEST_NUM, EPS_TEST, SEED, REPEATS = 100, 0.001, 9, 5
PATHS = (1, 10, 100)


def make_policy(n):
    torch.manual_seed(SEED)
    return DQNPolicy(build_network("l_dgn", n, "cuda"), target_update_freq=1)


def one_evaluation(policy, n, envs):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if envs == 1:
        out = _evaluate(policy, n, TEST_NUM, EPS_TEST, SEED, torch.device("cuda"), None, 0.0)
    else:
        out = _evaluate_spread(policy, n, TEST_NUM, envs, EPS_TEST, SEED, torch.device("cuda"), None, 0.0)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def setup_share(policy, n, envs):
    """The new path's set-up, phase by phase (ms): the envs, the stream (seed list, ring, first refill, the loop's reset), the
    eager warm-up round + the capture of the round graph, the capture of the four-round graph + its first replay."""
    marks = [time.perf_counter()]

    def mark():
        torch.cuda.synchronize()
        marks.append(time.perf_counter())

    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 16, first_seed=0), dynamic_graph=True, device="cuda",
                             max_moves=64, seed=SEED, construct_like_reference=False, is_testing=True,
                             num_test_episodes=TEST_NUM, spread_test_episodes=True)
    mark()
    col = Collector(policy, venv, seed=SEED, eps=EPS_TEST, use_graph=True, episode_stream="test")
    mark()
    with torch.no_grad():
        col.loop.run(2)
        mark()
        col.loop.run(4)
        mark()
    col.loop.supply.side.synchronize()
    return [(b - a) * 1e3 for a, b in zip(marks, marks[1:])]


def main():
    if "--trace" in sys.argv:
        n, envs = (int(x) for x in sys.argv[sys.argv.index("--trace") + 1:][:2])
        ms, out = one_evaluation(make_policy(n), n, envs)
        print(f"N={n} test_envs={envs}: {ms:.1f} ms, rew {out['rew']:.4f}", flush=True)
        return
    for n in (20, 50):
        policy = make_policy(n)
        policy.model.eval()
        ms = {e: [] for e in PATHS}
        for rep in range(REPEATS + 1):                         # alternated: 1, 10, 100, 1, 10, 100, ...
            for e in PATHS:
                dt, out = one_evaluation(policy, n, e)
                if rep:                                        # (the first repeat of every path is not timed)
                    ms[e].append(dt)
        med = {e: sorted(ms[e])[REPEATS // 2] for e in PATHS}
        for e in PATHS:
            print(f"l_dgn N={n} test_envs={e:3d}: one evaluation of {TEST_NUM} episodes {med[e]:9.1f} ms median of {REPEATS} "
                  f"(min {min(ms[e]):.1f}, max {max(ms[e]):.1f})", flush=True)
        for e in PATHS[1:]:
            spread = max(max(ms[s]) - min(ms[s]) for s in (1, e))
            print(f"l_dgn N={n}: test_envs {e} - test_envs 1 = {med[e] - med[1]:+.1f} ms ({(med[e] - med[1]) / med[1] * 100:+.1f} %), "
                  f"largest spread of a side {spread:.1f} ms", flush=True)
        for e in PATHS[1:]:
            setup_share(policy, n, e)                          # untimed once
            parts = setup_share(policy, n, e)
            print(f"l_dgn N={n} test_envs={e:3d} set-up: envs {parts[0]:.1f} ms, stream + first refill + reset {parts[1]:.1f} ms, "
                  f"warm-up round + round-graph capture {parts[2]:.1f} ms, four-round graph capture + first replay {parts[3]:.1f} ms "
                  f"= {sum(parts):.1f} ms", flush=True)


if __name__ == "__main__":
    main()
