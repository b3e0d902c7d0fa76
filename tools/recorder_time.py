"""Cost of a device recorder - the per-round recorder (melissa_amd/round_record.py: one more launch behind every env round), the
decision recorder (melissa_amd/decision_record.py: one more launch between every round's forward and env launch) or the
attention recorder (melissa_amd/attention_record.py: two more launches in the same place).

The per-round time of the graph-replayed L-DGN round loop, three ways - recorder off, on without traces, on with four traced
envs - on this tree and, with ``--parent-tree DIR`` (a checkout of the parent commit with its library built), on the parent's:
every variant a tree offers is run on it and labelled ``<tree>_<variant>``.  Every figure comes from a loop built anew (same
seeds, same trajectory, the same rounds timed), a block is timed on the host between two synchronisations, and the variants
ALTERNATE: block k of every variant runs before block k + 1 of any, each tree in a fresh child process.  Reported per variant:
the median of the blocks with their minimum and maximum in microseconds per round, the spread (largest max - min of a variant),
the recorder's cost on each tree and, per variant, this tree's median minus the parent's.

    python tools/recorder_time.py --recorder round|decisions|attention [--envs 1024] [--nodes 50] [--rounds 400] [--blocks 3]
                                  [--parent-tree DIR] [--out FILE]
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
VARIANTS = ("off", "on", "trace4")
# --recorder -> (module, class, the RoundLoop argument)
RECORDERS = {"round": ("round_record", "RoundRecorder", "recorder"), "decisions": ("decision_record", "DecisionRecorder", "decisions"),
             "attention": ("attention_record", "AttentionRecorder", "attention")}


def child(a):
    """One block of every variant the tree offers, on the tree ``a.tree``; prints {variant: us per round, ...}."""
    sys.path.insert(0, os.path.abspath(a.tree))
    import importlib
    import torch
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network
    module, cls, arg = RECORDERS[a.recorder]
    try:
        Recorder = getattr(importlib.import_module("melissa_amd." + module), cls)
    except ImportError:
        Recorder = None                           # a tree from before the recorder: the loop as it was
    out = {}
    for variant in (VARIANTS if Recorder is not None else VARIANTS[:1]):
        torch.manual_seed(0)
        net = build_network("l_dgn", a.nodes, torch.device("cuda"))
        venv = HipGraphVectorEnv(a.envs, a.nodes, graph_pool=synthetic_graph_pool(a.nodes, 16, first_seed=0), dynamic_graph=True,
                                 device="cuda", max_moves=48, construct_like_reference=False)
        kw = {}
        if variant != "off":
            own = (venv, net) if a.recorder == "attention" else (venv,)      # (the attention recorder reads the network's head count)
            kw[arg] = Recorder(*own, trace_envs=range(4) if variant == "trace4" else (), trace_capacity=64)
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
        if a.recorder == "round" and kw:
            out[variant + "_counters"] = kw[arg].curves()[2]
        elif kw:
            _by_round, by_degree, *_by_head, counters = kw[arg].tables()
            out[variant + "_counters"] = dict(counters, booked=float(by_degree[:, 0].sum()))
        del loop, venv, net, kw
        gc.collect()
    print("RESULT " + json.dumps(out))


def run_child(a, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--recorder", a.recorder, "--envs", str(a.envs),
           "--nodes", str(a.nodes), "--rounds", str(a.rounds), "--graph-rounds", str(a.graph_rounds)]
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
    ap.add_argument("--recorder", choices=sorted(RECORDERS), required=True)
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
    trees = ([("parent", a.parent_tree)] if a.parent_tree else []) + [("this", os.path.dirname(HERE))]
    blocks, extra = {}, {}
    for _ in range(a.blocks):
        for label, tree in trees:
            for k, v in run_child(a, tree).items():
                (blocks if k in VARIANTS else extra).setdefault(f"{label}_{k}", []).append(v)
    out = dict(recorder=a.recorder, envs=a.envs, nodes=a.nodes, rounds_per_block=a.rounds, graph_rounds=a.graph_rounds, blocks=a.blocks)
    for name, values in blocks.items():
        out[f"round_us_{name}"] = summary(values)
    out["spread_us"] = round(max(s["max"] - s["min"] for k, s in out.items() if k.startswith("round_us_")), 2)
    med = lambda name: out[f"round_us_{name}"]["median"]
    for label, _ in trees:
        for variant in VARIANTS[1:]:
            if f"{label}_{variant}" in blocks:
                out[f"{label}_{variant}_cost_us"] = round(med(f"{label}_{variant}") - med(f"{label}_off"), 2)
    if a.parent_tree:
        out["this_minus_parent_us"] = {v: round(med(f"this_{v}") - med(f"parent_{v}"), 2) for v in VARIANTS if f"parent_{v}" in blocks}
        out["equals_parent_within_spread"] = all(abs(d) <= out["spread_us"] for d in out["this_minus_parent_us"].values())
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
