"""Generate the golden data of the "mpr" scripted-agent heuristic from the REAL reference (build container only).

Run:  python tests/golden/make_mpr_golden.py
Needs /root/reference (read-only), imported through tests/golden/ref_standins.py, and reuses the helpers of
make_env_golden.py.  ``mpr_heuristic`` (heuristics/mpr.py:7-72) returns a bare array where ``World.step`` reads a
``HeuristicResult`` (core.py:227-234); this script installs the one-line reading
``HeuristicResult(relay_mask=mpr, action=None)`` in the heuristic registry, then records DATA only:

* ``mpr_sets_*.npz``: adjacency node sets ``adj`` and the reference's MPR set ``mpr`` of every node (uint64 [G, N], or
  [G, N, W] beyond 64 nodes), ``names`` of the graphs;
* ``mpr_trace_*.npz``: GraphEnv traces in the format of make_env_golden.py (replayed by tests/trace_replay.py), plus
  ``received_from`` (State.received_from of every node after each row, as node sets), ``relay_checks`` (how often the
  relays_for rule, core.py:236-243, examined a scripted node that holds the message) and ``forwards`` (transmissions of
  scripted non-source nodes that the rule allowed).  They are not named env_trace_*: the env oracle in oracle/ does not
  run this heuristic.

A scripted node forwards only after receiving the message from a scripted node that named it, and in training mode
scripted nodes have no action of their own and the source is never scripted (ratio < 1, core.py:212-214): there the
chain cannot start, the rule only silences.  The traces in testing mode (policy actions for scripted nodes without
relay duties, or ratio 1.0 with a scripted source) are the ones where it forwards.
"""
import os
import sys
import tempfile
import types

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_env_golden as meg  # noqa: E402
import ref_standins  # noqa: E402

FORWARDS = [0, 0]       # forwards, relay checks


def install_mpr():
    """HEURISTIC_REGISTRY["mpr"] -> HeuristicResult(relay_mask=mpr_heuristic(agent), action=None), plus a counter of the
    forwards the relays_for rule allows (World.relay_message of a scripted non-source node that some agent relays
    through)."""
    ref_graph, ref_core = ref_standins.import_reference()
    import graph_env.env.utils.heuristics as heur
    from graph_env.env.utils.heuristics.mpr import mpr_heuristic

    def mpr_as_result(agent):
        return heur.HeuristicResult(relay_mask=mpr_heuristic(agent), action=None)

    heur.HEURISTIC_REGISTRY["mpr"] = mpr_as_result
    ref_core.HEURISTIC_REGISTRY["mpr"] = mpr_as_result
    if not getattr(ref_core.World, "_mpr_counting", False):
        relay = ref_core.World.relay_message

        def counting(self, agent):
            if agent.is_scripted and agent.id != self.origin_agent and np.any(agent.state.relays_for):
                FORWARDS[0] += 1
            return relay(self, agent)

        ref_core.World.relay_message = counting
        ref_core.World._mpr_counting = True
        check = ref_core.Agent.has_received_from_relayed_node

        def counting_check(self):
            FORWARDS[1] += 1
            return check(self)

        ref_core.Agent.has_received_from_relayed_node = counting_check
    return ref_graph, ref_core, mpr_heuristic


def reference_mpr_sets(g, n):
    """The reference's MPR set of every node of g, with every agent set up like World.reset does (one-hop attributes,
    labels, two-hop sets, local views: core.py:398-425, 259-262)."""
    _, ref_core, mpr_heuristic = install_mpr()
    g = g.copy()
    g.add_nodes_from(range(n))
    agents = [ref_core.Agent(i, None) for i in range(n)]
    world = types.SimpleNamespace(num_agents=n, graph=g, agents=agents)
    for a in agents:
        a.state.reset(n)
        ref_core.World.update_one_hop_neighbors_info(world, a)
        g.nodes[a.id]["label"] = a.id
    for a in agents:
        ref_core.World.update_two_hop_neighbors_info(world, a)
    for a in agents:
        ref_core.World.update_local_graph(world, a)
    return [meg.mask_of(np.where(mpr_heuristic(agent=a))[0]) for a in agents]


def adjacency(g, n):
    adj = [0] * n
    for u, v in g.edges():
        adj[u] |= 1 << v
        adj[v] |= 1 << u
    return adj


def write_sets(name, n, graphs):
    adj, mpr, names = [], [], []
    for label, g in graphs:
        assert sorted(g.nodes) == list(range(n)), label
        adj.append([meg.words(m, n) for m in adjacency(g, n)])
        mpr.append([meg.words(m, n) for m in reference_mpr_sets(g, n)])
        names.append(label)
    path = os.path.join(HERE, f"mpr_sets_{name}.npz")
    np.savez_compressed(path, n=np.int64(n), adj=np.array(adj, dtype=np.uint64), mpr=np.array(mpr, dtype=np.uint64),
                        names=np.array(names))
    print(f"mpr_sets_{name}: {len(graphs)} graphs -> {os.path.getsize(path) / 1024:.0f} KiB")


def shapes(n, side):
    """Hand-made graphs of n nodes: path, star, cycle, clique (empty sets), a side x n/side grid (many ties), two
    connected components, one isolated node."""
    grid = nx.convert_node_labels_to_integers(nx.grid_2d_graph(side, n // side), ordering="sorted")
    half = n // 2
    a = meg.connected_rggs(half, 1, first_seed=5, radius=0.35)[0][1]
    b = meg.connected_rggs(n - half, 1, first_seed=50, radius=0.35)[0][1]
    two = nx.disjoint_union(a, b)
    rest = meg.connected_rggs(n - 1, 1, first_seed=9, radius=0.3 if n < 64 else 0.2)[0][1]
    iso_at = n // 3                                        # the isolated node sits between the others' ids
    lone = nx.relabel_nodes(rest, {i: (i if i < iso_at else i + 1) for i in range(n - 1)})
    lone.add_node(iso_at)
    return [("path", nx.path_graph(n)), ("star", nx.star_graph(n - 1)), ("cycle", nx.cycle_graph(n)),
            ("clique", nx.complete_graph(n)), (f"grid_{side}x{n // side}", grid), ("two_components", two),
            (f"isolated_{iso_at}", lone)]


def run_mpr_trace(name, n, mode, dynamic, steps, env_seed, tape_seed, ratio, n_graphs=4, num_test_episodes=None):
    ref_graph, ref_core, _ = install_mpr()
    ref_standins.DEFAULT_SEED = env_seed
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            kind = "testing" if mode == "testing" else "training"
            os.makedirs(f"graph_topologies/{kind}_{n}")
            graphs = meg.connected_rggs(n, n_graphs, first_seed=(300 if mode == "testing" else 100) * n + 7)
            for s, g in graphs:
                with open(f"graph_topologies/{kind}_{n}/rgg_{s:05d}.gpickle", "wb") as f:
                    import pickle
                    pickle.dump(g, f)     # a file this script wrote, not a reference artefact
            env = ref_graph.GraphEnv(graph=None, number_of_agents=n, radius=0.2, dynamic_graph=dynamic,
                                     is_testing=mode == "testing", num_test_episodes=num_test_episodes or 10,
                                     scripted_agents_ratio=ratio, heuristic="mpr")
            files = env.world.test_graphs if mode == "testing" else env.world.train_graphs
            by_name = {f"rgg_{s:05d}.gpickle": g for s, g in graphs}
            pool = [by_name[os.path.basename(p)] for p in files]
            meta = {"pool_pos": np.array([[gg.nodes[i]["pos"] for i in range(n)] for gg in pool], dtype=np.float64),
                    "pool_adj": np.array([[meg.words(m, n) for m in adjacency(gg, n)] for gg in pool], dtype=np.uint64)}
            pz = meg.RefPettingZoo(env)
            tape = np.random.RandomState(tape_seed).randint(0, 2, size=steps).astype(np.int8)
            rows = {k: [] for k in ("agent_id obs mask rew term trunc env_step environment_step explicit_reset active_nb "
                                    "has_stats stats agents_mask alive_mask terminated_mask has_message_mask "
                                    "interested_mask scripted_mask origin pos one_hop two_hop was_reset "
                                    "received_from").split()}

            def keep(packed, was_reset):
                meg.record(rows, pz, packed, n)
                rows["was_reset"].append(was_reset)
                rows["received_from"].append(np.array(
                    [meg.words(meg.mask_of(np.where(a.state.received_from)[0]), n) for a in env.world.agents], dtype=np.uint64))

            FORWARDS[0] = FORWARDS[1] = 0         # (constructor-time episodes do not count)
            keep(pz.reset(), True)
            done_count = 0
            for t in range(steps):
                packed = pz.step(int(tape[t]))
                keep(packed, False)
                _, term, trunc, info = packed
                if term or trunc:
                    done_count += 1
                    if done_count == n or info.get("explicit_reset", False):
                        keep(pz.reset(), True)
                        done_count = 0
        finally:
            os.chdir(cwd)
    out = {k: np.array(v) for k, v in rows.items()}
    out.update(meta)
    out.update(n=np.int64(n), dynamic=np.bool_(dynamic), env_seed=np.int64(env_seed), tape=tape,
               fixed_graph=np.bool_(False), is_testing=np.bool_(mode == "testing"),
               num_test_episodes=np.int64(num_test_episodes or 0), scripted_agents_ratio=np.float64(ratio),
               heuristic=np.str_("mpr"), local_ratio=np.float64(-1.0), forwards=np.int64(FORWARDS[0]),
               relay_checks=np.int64(FORWARDS[1]))
    assert FORWARDS[1] >= 5, f"{name}: the relays_for rule examined a scripted node only {FORWARDS[1]} times"
    if mode == "testing":
        assert FORWARDS[0] >= 5, f"{name}: the relays_for rule let scripted nodes forward only {FORWARDS[0]} times"
    assert len(out["agent_id"]) >= 300
    path = os.path.join(HERE, f"mpr_trace_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"mpr_trace_{name}: {len(out['agent_id'])} rows, {int(np.sum(out['was_reset']))} resets, "
          f"{FORWARDS[1]} relay checks, {FORWARDS[0]} relay forwards -> {os.path.getsize(path) / 1024:.0f} KiB")


def main(only=None):
    if only == "traces":
        return traces()
    write_sets("n12_fixture", 12, [("test_core_fixture", meg.fixture_graph_12())])
    for n, count in ((20, 40), (50, 30), (100, 16), (128, 10)):
        write_sets(f"rgg_n{n}", n, [(f"rgg_seed{s}", g) for s, g in meg.connected_rggs(n, count, first_seed=1000 + n)])
    write_sets("shapes_n30", 30, shapes(30, 5))
    write_sets("shapes_n100", 100, shapes(100, 10))
    traces()


def traces():
    run_mpr_trace("n20_pool_dynamic", 20, "pool", True, 700, env_seed=31, tape_seed=21, ratio=0.5)
    run_mpr_trace("n50_pool_static", 50, "pool", False, 600, env_seed=32, tape_seed=22, ratio=0.4)
    run_mpr_trace("n20_testing_dynamic", 20, "testing", True, 600, env_seed=33, tape_seed=23, ratio=1.0, num_test_episodes=6)
    run_mpr_trace("n100_pool_dynamic", 100, "pool", True, 400, env_seed=34, tape_seed=24, ratio=0.5, n_graphs=3)
    run_mpr_trace("n100_testing_dynamic", 100, "testing", True, 500, env_seed=35, tape_seed=25, ratio=0.5, n_graphs=3,
                  num_test_episodes=5)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
