"""Evaluation run, the counterpart of the reference's ``--watch`` mode (l_dgn.py:315-319 -> ``watch``: load a policy,
run test episodes on evaluation envs, report the episodes' statistics).

    python -m melissa_amd.watch --model l_dgn --nodes 20 --envs 1 --episodes 10 [--load policy.pth]
                                [--heuristic mpr --scripted-agents-ratio 0.5] [--envs 16 --spread]

``--envs E`` alone makes every env walk the list of test seeds from the top (the reference's order, core.py:351-352): the
``--episodes`` episodes reported are the first ``ceil(episodes / E)`` list positions, ``E`` times over.  ``--spread`` shares
the list out instead - env b plays positions ``b, b + E, ...``, each of the ``--episodes`` positions exactly once - drawn on
the device and replayed from a HIP graph (:func:`melissa_amd.collect.evaluate_spread`).

``--attention-out FILE [--attention-rounds K]`` also plays ``K`` greedy rounds on a small env batch of its own and writes what
the policy saw, what it did and the convolutions' attention weights - which neighbours each node listened to - into an
``.npz`` (:func:`record_attention`); the evaluation and its printed result are the same with and without it.

``--curves-out FILE``, ``--trace-out FILE [--trace-envs K]`` and ``--render-out DIR`` (all with ``--spread``) record the
evaluation round by round on the device (:class:`melissa_amd.round_record.RoundRecorder`): the dissemination curves - coverage
and messages against the round, delivery delay - as JSON, the per-node state of envs ``0 .. K-1`` after every round as an
``.npz``, and one SVG per round and episode coloured by the reference's ``draw_graph`` rule (:mod:`melissa_amd.render`).  The
printed result is the same with and without them.

``--decisions-out FILE`` and ``--decision-trace-out FILE [--trace-envs K]`` (with ``--spread``) record the policy's decisions
between every round's forward and env launch (:class:`melissa_amd.decision_record.DecisionRecorder`): relay rate, Q gap,
non-greedy and first-decision shares against the round index and against the node's degree as JSON, and per round of envs
``0 .. K-1`` who decided, who relayed and with which Q values as an ``.npz`` that joins ``--trace-out`` on
(env, episode ordinal, round).

Graphs: connected random geometric graphs (the reference reads graph_topologies/testing_N/*; pass your own pool through
``watch(graph_pool=...)``).  ``--load`` takes a state_dict saved by ``python -m melissa_amd.train --epoch ...``
(``<logdir>/<model>/weights/<model_name>_best.pth`` / ``_last.pth``) or by the reference's trainer (keys ``model.*`` /
``model_old.*``, l_dgn.py:311), loaded with ``weights_only=True``.  ``--heuristic`` / ``--scripted-agents-ratio`` are the
reference's flags (common.py:67,69): that fraction of the nodes runs the heuristic instead of the policy (in the evaluation
schedule the policy still decides for them, graph.py:244,340; the heuristic overrides it inside the world step).
"""
from __future__ import annotations

import argparse
import json

import torch

from .collect import Collector, RoundLoop, evaluate_spread
from .env import HipGraphVectorEnv, connected_graph_pool, load_graph_pool
from .policy import DQNPolicy
from .attention_record import check_attention_args
from .decision_record import check_decision_args
from .round_record import check_record_args
from .train import AGGREGATORS, N_DGN_NETWORK, build_network, check_network_args, load_policy_weights


def record_attention(policy, venv, rounds: int, seed: int = 0) -> dict:
    """Play ``rounds`` greedy rounds on ``venv`` with the eager round loop (:class:`melissa_amd.collect.RoundLoop`, one launch
    sequence per round, no HIP graph) and keep, per round and env, what the policy saw and which neighbours it listened to:

    ``obs`` fp32 [K, E, 8N]  the observation matrix the round's forward read;  ``acted`` bool [K, E, N]  the round's active
    agents;  ``action`` int32 [K, E, N]  their actions (-1 for a node that did not act);  ``alpha_conv1`` (``alpha_conv2`` for
    the two-convolution models) fp32 [K, E, N, N, H]  ``policy.model.attention_weights`` of ``obs``: target i, source j."""
    net, n, E, dev = policy.model, venv.n, venv.env_num, venv.device
    loop = RoundLoop(venv, policy, episodes_per_env=int(rounds) + 2, seed=seed, eps=0.0, use_graph=False)   # an episode per round at most
    node = torch.arange(n, device=dev)
    rec: dict = {"obs": [], "acted": [], "action": []}
    with torch.no_grad():
        for _ in range(int(rounds)):
            obs = loop._obs_matrix[:, :8 * n].clone()
            acted = ((loop.live.reshape(E, -1)[:, node // 64] >> (node % 64)) & 1).bool()          # [E, N]
            loop.step()
            action = torch.full((E, n), -1, dtype=torch.int32, device=dev)
            if loop.per_env_logits:                        # dense layout: act[b * n + i]
                action[acted] = loop.act.view(E, n)[acted]
            else:                                          # rows by env, then by agent id: the order of the set bits
                action[acted] = loop.act[:int(acted.sum())]
            alphas = net.attention_weights(torch.cat([obs, obs.new_zeros(E, 1)], dim=1))
            rec["obs"].append(obs), rec["acted"].append(acted), rec["action"].append(action)
            for k, a in enumerate(alphas):
                rec.setdefault(f"alpha_conv{k + 1}", []).append(a)
    errors = loop.counters()["errors"]
    if errors:
        raise RuntimeError(f"env error flags {errors:#x} while recording attention weights")
    return {k: torch.stack(v).cpu().numpy() for k, v in rec.items()}


def watch(model="l_dgn", n_nodes=20, envs=1, episodes=10, load=None, graph_pool=None, seed=9, device="cuda:0",
          dynamic_graph=True, feature_dtype="f32", heuristic=None, scripted_agents_ratio=0.0, spread=False, collect_stats="episodes",
          graphs=16, hidden_emb=128, num_heads=4, dueling_q_hidden_sizes=(128, 128), dueling_v_hidden_sizes=(128, 128),
          aggregator_function="max", attention_out=None, attention_rounds=8, curves_out=None, trace_out=None, trace_envs=1,
          render_out=None, decisions_out=None, decision_trace_out=None, attention_curves_out=None, attention_trace_out=None):
    """``graph_pool``: a list of graphs or the path of a packed ``.npz`` (``save_graph_pool``); None draws ``graphs`` connected
    random geometric graphs with the device generator (the graphs of ``synthetic_graph_pool(n_nodes, graphs)``).
    ``collect_stats``: "steps" reports the mean of every ``logger_stats`` key over every env step played (the reference's
    statistic, pooled on the device; ``n_info_rows`` steps) instead of over the episodes' final rows.  Not with ``spread``:
    the envs that finish their share early keep playing, and those surplus episodes would enter the pool.
    ``hidden_emb`` ... ``aggregator_function``: the network flags of :func:`melissa_amd.train.train`; ``load`` of a checkpoint
    trained at another shape is a ValueError naming the mismatching key and both shapes.
    ``attention_out``: path of an ``.npz`` that receives :func:`record_attention` of ``attention_rounds`` greedy rounds on a
    separate batch of ``min(envs, 4)`` envs (every env walks the test list from the top, ``spread`` or not), played after the
    evaluation: the returned dict is the same with and without it.
    ``curves_out`` (a JSON file: :func:`melissa_amd.round_record.summarise` of the evaluation's episodes plus the raw ``running``
    / ``ended`` sums and the recorder's counters), ``trace_out`` (an ``.npz``: the per-node state of envs ``0 .. trace_envs - 1``
    after every round of their episodes) and ``render_out`` (a directory: one SVG per round of those episodes) need ``spread``:
    the recorder rides behind the spread evaluation's rounds and leaves the returned dict as it is.
    ``decisions_out`` (a JSON file: :func:`melissa_amd.decision_record.summarise_decisions` of the evaluation's decisions plus the
    raw ``by_round`` / ``by_degree`` sums and the counters) and ``decision_trace_out`` (an ``.npz``: per round of envs
    ``0 .. trace_envs - 1`` the deciding and relaying sets and the Q values, keyed like ``trace_out``) need ``spread`` too.
    ``attention_curves_out`` (a JSON file: :func:`melissa_amd.attention_record.summarise_attention` of conv2's coefficients of
    the evaluation's own inference launches - the attention the informed and the waiting neighbours of every deciding node got,
    by round index, node degree and head - plus the raw sums and the counters) and ``attention_trace_out`` (an ``.npz``: per
    round of envs ``0 .. trace_envs - 1`` the deciding set and every deciding node's head-mean fields) need ``spread`` as well,
    and a two-convolution model on an fp32 feature path."""
    check_record_args(spread, curves_out, trace_out, render_out, trace_envs)
    check_decision_args(spread, decisions_out, decision_trace_out, trace_envs)
    check_attention_args(spread, attention_curves_out, attention_trace_out, trace_envs, model=model, feature_dtype=feature_dtype)
    check_network_args(model, hidden_emb, num_heads, dueling_q_hidden_sizes, dueling_v_hidden_sizes, aggregator_function,
                       feature_dtype=feature_dtype)
    if spread and collect_stats != "episodes":
        raise ValueError("collect_stats='steps' is not offered with spread: surplus episodes would enter the pool")
    if attention_out is not None and int(attention_rounds) < 1:
        raise ValueError(f"attention_rounds={attention_rounds}: at least one round")
    torch.manual_seed(seed)
    net = build_network(model, n_nodes, device, hidden=hidden_emb, heads=num_heads, dueling_q_hidden_sizes=dueling_q_hidden_sizes,
                        dueling_v_hidden_sizes=dueling_v_hidden_sizes, aggregator=aggregator_function)
    policy = DQNPolicy(net, target_update_freq=1)
    if load:
        load_policy_weights(policy, load, device)
    net.eval()
    net.set_feature_dtype(feature_dtype)
    if isinstance(graph_pool, str):
        graph_pool = load_graph_pool(graph_pool)
    pool = graph_pool if graph_pool is not None else connected_graph_pool(n_nodes, graphs, first_seed=0, device=device)
    if spread:
        envs = min(envs, episodes)
    venv = HipGraphVectorEnv(envs, n_nodes, graph_pool=pool, dynamic_graph=dynamic_graph, device=device, max_moves=64,
                             seed=seed, construct_like_reference=False, is_testing=True, num_test_episodes=episodes,
                             scripted_agents_ratio=scripted_agents_ratio, heuristic=heuristic, spread_test_episodes=spread)
    recorder = None
    if curves_out is not None or trace_out is not None or render_out is not None:
        from .round_record import RoundRecorder
        traced = range(min(int(trace_envs), envs)) if (trace_out is not None or render_out is not None) else ()
        recorder = RoundRecorder(venv, trace_envs=traced, trace_capacity=64)
    decisions = None
    if decisions_out is not None or decision_trace_out is not None:
        from .decision_record import DecisionRecorder
        traced = range(min(int(trace_envs), envs)) if decision_trace_out is not None else ()
        decisions = DecisionRecorder(venv, trace_envs=traced, trace_capacity=64)
    attention = None
    if attention_curves_out is not None or attention_trace_out is not None:
        from .attention_record import AttentionRecorder
        traced = range(min(int(trace_envs), envs)) if attention_trace_out is not None else ()
        attention = AttentionRecorder(venv, net, trace_envs=traced, trace_capacity=64)
    if spread:
        out, _positions = evaluate_spread(policy, venv, episodes, eps=0.0, seed=seed, recorder=recorder, decisions=decisions,
                                          attention=attention)
    else:
        per_env = -(-episodes // envs) + 2
        col = Collector(policy, venv, episodes_per_env=per_env, seed=seed, eps=0.0, chunk=4, use_graph=envs >= 64,
                        stats=collect_stats)
        out = col.collect(n_episode=episodes)
    if recorder is not None:
        write_record(recorder, n_nodes, curves_out, trace_out, render_out)
    if decisions is not None:
        write_decisions(decisions, decisions_out, decision_trace_out)
    if attention is not None:
        write_attention(attention, attention_curves_out, attention_trace_out)
    if attention_out is not None:
        # AFTER the evaluation and on an env batch of its own (built like the evaluation's: same pool, seed and flags), so the
        # result below is what it is without the flag
        import numpy as np
        side = HipGraphVectorEnv(min(envs, 4), n_nodes, graph_pool=pool, dynamic_graph=dynamic_graph, device=device, max_moves=64,
                                 seed=seed, construct_like_reference=False, is_testing=True, num_test_episodes=episodes,
                                 scripted_agents_ratio=scripted_agents_ratio, heuristic=heuristic)
        with open(attention_out, "wb") as f:
            np.savez(f, **record_attention(policy, side, attention_rounds, seed=seed))
    # the scalars of the collect result (counts, speed, mean return / length, mean of every logger_stats key) as a plain dict
    keys = ["n/ep", "n/st", "collect_time", "collect_speed"] + (["rew", "len"] if out.returns_stat is not None else []) \
        + list(out.info.stats) + (["n_info_rows"] if collect_stats == "steps" else [])
    return {k: out[k] for k in keys}


def as_json(v):
    """A summary for ``json.dump``: arrays as lists, NaN (a ratio over nothing) as null, dict keys (the ``delay`` quantiles) as strings."""
    if isinstance(v, dict):
        return {str(k): as_json(x) for k, x in v.items()}
    v = v.tolist() if hasattr(v, "tolist") else v
    if isinstance(v, list):
        return [as_json(x) for x in v]
    return None if isinstance(v, float) and v != v else v


def write_record(recorder, n_nodes: int, curves_out=None, trace_out=None, render_out=None) -> None:
    """What the recorder holds after an evaluation, into the files the caller asked for."""
    from .render import write_svg_frames
    from .round_record import save_traces, summarise
    running, ended, counters = recorder.curves()
    traces, lost = recorder.drain_traces()
    if curves_out is not None:
        doc = as_json(summarise(running, ended, n_nodes=n_nodes))
        doc.update(running_sums=running.tolist(), ended_sums=ended.tolist(), counters=dict(counters, lost_trace_records=int(lost)))
        with open(curves_out, "w") as f:
            json.dump(doc, f)
    if trace_out is not None:
        save_traces(trace_out, traces)
    if render_out is not None:
        for episodes in traces.values():
            for ep in episodes:
                write_svg_frames(ep, render_out)


def write_decisions(decisions, decisions_out=None, decision_trace_out=None) -> None:
    """What the decision recorder holds after an evaluation, into the files the caller asked for."""
    from .decision_record import save_decision_traces, summarise_decisions
    by_round, by_degree, counters = decisions.tables()
    traces, lost = decisions.drain_traces()
    if decisions_out is not None:
        doc = as_json(summarise_decisions(by_round, by_degree))
        doc.update(by_round_sums=by_round.tolist(), by_degree_sums=by_degree.tolist(),
                   counters=dict(counters, lost_trace_records=int(lost)))
        with open(decisions_out, "w") as f:
            json.dump(doc, f)
    if decision_trace_out is not None:
        save_decision_traces(decision_trace_out, traces)


def write_attention(attention, attention_curves_out=None, attention_trace_out=None) -> None:
    """What the attention recorder holds after an evaluation, into the files the caller asked for."""
    from .attention_record import save_attention_traces, summarise_attention
    by_round, by_degree, by_head, counters = attention.tables()
    traces, lost = attention.drain_traces()
    if attention_curves_out is not None:
        doc = as_json(summarise_attention(by_round, by_degree, by_head))
        doc.update(by_round_sums=by_round.tolist(), by_degree_sums=by_degree.tolist(), by_head_sums=by_head.tolist(),
                   counters=dict(counters, lost_trace_records=int(lost)))
        with open(attention_curves_out, "w") as f:
            json.dump(doc, f)
    if attention_trace_out is not None:
        save_attention_traces(attention_trace_out, traces)


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    # (the three N-DGN scripts train these networks under their own names: a checkpoint of theirs loads into the same classes)
    ap.add_argument("--model", default="l_dgn", choices=["l_dgn", "hl_dgn", "dgn_r", *N_DGN_NETWORK])
    ap.add_argument("--nodes", type=int, default=20)
    ap.add_argument("--envs", type=int, default=1)
    ap.add_argument("--episodes", type=int, default=10)
    ap.add_argument("--load", default=None)
    ap.add_argument("--graphs", type=int, default=16, help="evaluation-graph pool size")
    ap.add_argument("--graph-pool", default=None, metavar="FILE",
                    help="packed graph dataset (.npz of python -m melissa_amd.env.episodes) used instead of --graphs")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16", "f32s", "f32a"])
    ap.add_argument("--heuristic", default=None, choices=["simple_broadcast", "broadcast_if_any_interested", "silent", "mpr"],
                    help="heuristic the scripted agents run (common.py:67)")
    ap.add_argument("--scripted-agents-ratio", type=float, default=0.0,
                    help="fraction of the nodes that are scripted agents (common.py:69)")
    ap.add_argument("--spread", action="store_true", default=False,
                    help="share the --episodes test seeds out over the --envs envs (each played once) instead of every env "
                         "walking the list from the top")
    ap.add_argument("--collect-stats", choices=["episodes", "steps"], default="episodes",
                    help="steps: the logger_stats means are taken over every env step played (the reference's statistic), not "
                         "over the episodes' final rows; not with --spread")
    # the reference's network flags, names and defaults (common.py:29-30,41-43): those of the run that trained --load
    ap.add_argument("--hidden-emb", type=int, default=128, help="encoder width and channels per attention head")
    ap.add_argument("--num-heads", type=int, default=4, help="attention heads (a power of two, or 6)")
    ap.add_argument("--dueling-q-hidden-sizes", type=int, nargs="*", default=[128, 128])
    ap.add_argument("--dueling-v-hidden-sizes", type=int, nargs="*", default=[128, 128])
    ap.add_argument("--aggregator-function", type=str, default="max", choices=list(AGGREGATORS),
                    help="graph pool of the HL-DGN models")
    ap.add_argument("--attention-out", default=None, metavar="FILE",
                    help=".npz that receives obs, acted, action and the convolutions' attention weights (alpha_conv1, "
                         "alpha_conv2: [rounds, envs, N target, N source, heads]) of --attention-rounds greedy rounds on "
                         "min(--envs, 4) envs of their own; the evaluation is unaffected")
    ap.add_argument("--attention-rounds", type=int, default=8, help="rounds recorded into --attention-out")
    # (absent from the namespace unless given: callers that compare the namespace of a plain call see what they saw)
    ap.add_argument("--curves-out", default=argparse.SUPPRESS, metavar="FILE",
                    help="JSON file that receives the evaluation's per-round curves (coverage, messages, delivery delay); "
                         "needs --spread")
    ap.add_argument("--trace-out", default=argparse.SUPPRESS, metavar="FILE",
                    help=".npz that receives the per-node state of the traced envs after every round; needs --spread")
    ap.add_argument("--trace-envs", type=int, default=argparse.SUPPRESS,
                    help="envs 0 .. K-1 are traced for --trace-out / --render-out (default 1)")
    ap.add_argument("--render-out", default=argparse.SUPPRESS, metavar="DIR",
                    help="directory that receives one SVG per round of the traced envs' episodes; needs --spread")
    ap.add_argument("--decisions-out", default=argparse.SUPPRESS, metavar="FILE",
                    help="JSON file that receives the policy's decisions per round index and per node degree (relay rate, Q gap, "
                         "non-greedy and first-decision shares); needs --spread")
    ap.add_argument("--decision-trace-out", default=argparse.SUPPRESS, metavar="FILE",
                    help=".npz that receives, per round of the traced envs (--trace-envs), who decided, who relayed and the Q "
                         "values; needs --spread")
    ap.add_argument("--attention-curves-out", default=argparse.SUPPRESS, metavar="FILE",
                    help="JSON file that receives whom the deciding agents attended to in the evaluation's own inference launches "
                         "(conv2: attention on informed / waiting neighbours, lifts, effective neighbours) per round index, node "
                         "degree and head; needs --spread and a two-convolution model at an fp32 --dtype")
    ap.add_argument("--attention-trace-out", default=argparse.SUPPRESS, metavar="FILE",
                    help=".npz that receives, per round of the traced envs (--trace-envs), the deciding set and every deciding "
                         "node's head-mean attention fields; needs --spread")
    return ap


def record_args(a: argparse.Namespace) -> tuple:
    """(curves_out, trace_out, render_out, trace_envs) of a parsed command line, with their defaults where not given."""
    return (getattr(a, "curves_out", None), getattr(a, "trace_out", None), getattr(a, "render_out", None),
            int(getattr(a, "trace_envs", 1)))


def decision_args(a: argparse.Namespace) -> tuple:
    """(decisions_out, decision_trace_out) of a parsed command line, None where not given."""
    return getattr(a, "decisions_out", None), getattr(a, "decision_trace_out", None)


def attention_args(a: argparse.Namespace) -> tuple:
    """(attention_curves_out, attention_trace_out) of a parsed command line, None where not given."""
    return getattr(a, "attention_curves_out", None), getattr(a, "attention_trace_out", None)


def parse_args(argv=None) -> argparse.Namespace:
    ap = arg_parser()
    a = ap.parse_args(argv)
    try:
        check_network_args(a.model, a.hidden_emb, a.num_heads, a.dueling_q_hidden_sizes, a.dueling_v_hidden_sizes,
                           a.aggregator_function, feature_dtype=a.dtype)
    except ValueError as e:
        ap.error(str(e))
    if a.spread and a.collect_stats != "episodes":
        ap.error("--collect-stats steps is not offered with --spread (surplus episodes would enter the pool)")
    if a.attention_rounds < 1:
        ap.error("--attention-rounds: at least one round")
    try:
        check_record_args(a.spread, *record_args(a))
        check_decision_args(a.spread, *decision_args(a), trace_envs=record_args(a)[3])
        check_attention_args(a.spread, *attention_args(a), trace_envs=record_args(a)[3], model=a.model, feature_dtype=a.dtype)
    except ValueError as e:
        ap.error(str(e))
    return a


def main(argv=None):
    a = parse_args(argv)
    import sys
    given = sys.argv[1:] if argv is None else argv
    if a.graph_pool is not None and any(x == "--graphs" or x.startswith("--graphs=") for x in given):
        print(f"--graph-pool {a.graph_pool} is the graph pool: --graphs {a.graphs} is ignored", file=sys.stderr)
    print(json.dumps(watch(a.model, a.nodes, a.envs, a.episodes, a.load, feature_dtype=a.dtype, heuristic=a.heuristic,
                           scripted_agents_ratio=a.scripted_agents_ratio, spread=a.spread, collect_stats=a.collect_stats,
                           graph_pool=a.graph_pool, graphs=a.graphs, hidden_emb=a.hidden_emb, num_heads=a.num_heads,
                           dueling_q_hidden_sizes=list(a.dueling_q_hidden_sizes),
                           dueling_v_hidden_sizes=list(a.dueling_v_hidden_sizes), aggregator_function=a.aggregator_function,
                           attention_out=a.attention_out, attention_rounds=a.attention_rounds,
                           **dict(zip(("curves_out", "trace_out", "render_out", "trace_envs"), record_args(a))),
                           **dict(zip(("decisions_out", "decision_trace_out"), decision_args(a))),
                           **dict(zip(("attention_curves_out", "attention_trace_out"), attention_args(a))))))


if __name__ == "__main__":
    main()
