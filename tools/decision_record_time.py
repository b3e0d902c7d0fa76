"""Cost of the decision recorder (melissa_amd/decision_record.py): one more launch between every round's forward and env launch.

The per-round time of the graph-replayed L-DGN round loop, three ways on this tree - recorder off, on with the tables only, on
with four traced envs - and, with ``--parent-tree DIR`` (a checkout of the parent commit with its library built), the same loop
on the parent's code.  Every figure comes from a loop built anew (same seeds, same trajectory, the same rounds timed), a block is
timed on the host between two synchronisations, and the variants ALTERNATE: block k of every variant runs before block k + 1 of
any, each tree in a fresh child process.  Reported per variant: the median of the blocks with their minimum and maximum in
microseconds per round, the spread (largest max - min of a variant), and the differences of the medians.

    python tools/decision_record_time.py [--envs 1024] [--nodes 50] [--rounds 400] [--blocks 3] [--parent-tree DIR] [--out FILE]
"""
import argparse
import gc
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("off", "tables", "trace4")


def child(a):
    """One block of every variant the tree offers, on the tree ``a.tree``; prints {variant: us per round, ...}."""
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network
    try:
        from melissa_amd.decision_record import DecisionRecorder
    except ImportError:
        DecisionRecorder = None                   # the parent commit: the loop as it was
    out = {}
    for variant in (VARIANTS if DecisionRecorder is not None else ("parent",)):
        torch.manual_seed(0)
        net = build_network("l_dgn", a.nodes, torch.device("cuda"))
        venv = HipGraphVectorEnv(a.envs, a.nodes, graph_pool=synthetic_graph_pool(a.nodes, 16, first_seed=0), dynamic_graph=True,
                                 device="cuda", max_moves=48, construct_like_reference=False)
        kw = {}
        if variant in ("tables", "trace4"):
            kw["decisions"] = DecisionRecorder(venv, trace_envs=range(4) if variant == "trace4" else (), trace_capacity=64)
        loop = RoundLoop(venv, DQNPolicy(net), seed=1, eps=0.05, use_graph=True, graph_rounds=a.graph_rounds, **kw)
        with torch.no_grad():
            loop.run(2 + 8 * a.graph_rounds)       # warm-up, both captures, past the first episodes
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loop.run(a.rounds)
            torch.cuda.synchronize()
            out[variant] = (time.perf_counter() - t0) / a.rounds * 1e6
        c = loop.counters()
        out[variant + "_decisions"], out[variant + "_errors"] = c["decisions"], c["errors"]
        if "decisions" in kw:
            by_round, by_degree, counters = kw["decisions"].tables()
            out[variant + "_counters"] = dict(counters, booked=float(by_degree[:, 0].sum()))
        del loop, venv, net, kw
        gc.collect()
    print("RESULT " + json.dumps(out))


def run_child(a, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--envs", str(a.envs), "--nodes", str(a.nodes),
           "--rounds", str(a.rounds), "--graph-rounds", str(a.graph_rounds)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=a.child_timeout)
    lines = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
    if res.returncode != 0 or not lines:
        raise RuntimeError(f"child on {tree} failed ({res.returncode}):\n{res.stdout[-2000:]}\n{res.stderr[-2000:]}")
    return json.loads(lines[-1][len("RESULT "):])


def summary(blocks):
    return dict(median=round(statistics.median(blocks), 2), min=round(min(blocks), 2), max=round(max(blocks), 2),
                blocks=[round(x, 2) for x in blocks])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=400, help="rounds per block")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--graph-rounds", type=int, default=4)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit, its library built")
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=os.path.dirname(HERE), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    blocks, extra = {}, {}
    for _ in range(a.blocks):
        for tree in ([a.parent_tree] if a.parent_tree else []) + [os.path.dirname(HERE)]:
            for k, v in run_child(a, tree).items():
                if k in VARIANTS or k == "parent":
                    blocks.setdefault(k, []).append(v)
                else:
                    extra.setdefault(k, []).append(v)
    out = dict(envs=a.envs, nodes=a.nodes, rounds_per_block=a.rounds, graph_rounds=a.graph_rounds, blocks=a.blocks)
    for name, values in blocks.items():
        out[f"round_us_{name}"] = summary(values)
    out["spread_us"] = round(max(s["max"] - s["min"] for k, s in out.items() if k.startswith("round_us_")), 2)
    med = lambda name: out[f"round_us_{name}"]["median"]
    if "parent" in blocks:
        out["off_minus_parent_us"] = round(med("off") - med("parent"), 2)
        out["off_equals_parent_within_spread"] = abs(out["off_minus_parent_us"]) <= out["spread_us"]
    out["tables_cost_us"], out["trace4_cost_us"] = round(med("tables") - med("off"), 2), round(med("trace4") - med("off"), 2)
    decisions = {k[:-len("_decisions")]: v for k, v in extra.items() if k.endswith("_decisions")}
    out["same_trajectory"] = len({tuple(v) for v in decisions.values()}) == 1
    out["errors"] = max(max(v) for k, v in extra.items() if k.endswith("_errors"))
    out["recorder_counters"] = {k[:-len("_counters")]: v[-1] for k, v in extra.items() if k.endswith("_counters")}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
