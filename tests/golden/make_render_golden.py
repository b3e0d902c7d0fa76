"""Generate the golden of the reference's rendering rule from the REAL reference ``GraphEnv`` (build container only).

Run:  python tests/golden/make_render_golden.py
Needs /root/reference (read-only) - imported through tests/golden/ref_standins.py.  The file written is DATA (the env state
after every world step and the ``node_color`` list the reference hands to ``nx.draw``); no reference source is stored.

``GraphEnv(render_mode="human")`` calls ``draw_graph`` after every world step (graph.py:350-356,466-484).  A stand-in takes the
place of ``matplotlib.pyplot`` (``clf`` / ``pause`` do nothing) and of ``nx.draw`` (it keeps ``node_color`` and the graph's node
order) inside the reference module; every call also records the env state a round recorder would sample at that moment.  Two
traces on the reference's own 12-node test fixture graph, static and moving, two episodes each, driven by an action tape.
``tests/test_round_record_ref.py`` feeds the states through the recorder's NumPy model and ``melissa_amd.render.colour_classes``.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_standins  # noqa: E402
from make_env_golden import RefPettingZoo, fixture_graph_12, mask_of  # noqa: E402

CLASSES = ("green", "blue", "purple", "red", "yellow")
N = 12


class _Pyplot:
    @staticmethod
    def clf():
        pass

    @staticmethod
    def pause(_seconds):
        pass


class _Networkx:
    """networkx as the reference module sees it, with a ``draw`` that keeps what it is given."""

    def __init__(self, real, sink):
        self._real, self._sink = real, sink

    def __getattr__(self, name):
        return getattr(self._real, name)

    def draw(self, graph, node_color=None, **_kw):
        self._sink(list(graph), list(node_color))


def state_row(env, ordinal):
    w = env.world
    return dict(ordinal=ordinal, num_moves=int(env.num_moves), world_msgs=int(w.messages_transmitted), origin=int(w.origin_agent),
                has_message=np.uint64(mask_of(a.name for a in w.agents if a.state.has_message)),
                origin_set=np.uint64(mask_of(a.name for a in w.agents if a.state.message_origin)),
                interested=np.uint64(mask_of(a.name for a in w.agents if a.is_interested)),
                scripted=np.uint64(mask_of(a.name for a in w.agents if a.is_scripted)),
                active=np.uint64(mask_of(env.agents)),
                taken_action=np.uint64(mask_of(a.name for a in w.agents if a.state.has_taken_action)),
                pos=np.array([a.pos for a in w.agents], dtype=np.float64),
                one_hop=np.array([mask_of(np.where(a.one_hop_neighbours_ids)[0]) for a in w.agents], dtype=np.uint64),
                agent_msgs=np.array([a.messages_transmitted for a in w.agents], dtype=np.int32),
                received=np.array([int(np.sum(a.state.received_from)) for a in w.agents], dtype=np.int32))


def run_trace(dynamic, env_seed, tape_seed, episodes=2, max_steps=4000):
    ref_graph, _ = ref_standins.import_reference()
    ref_standins.DEFAULT_SEED = env_seed
    rows, box = [], {}

    def sink(order, node_color):
        colour = np.full(N, -1, dtype=np.int8)
        for node, name in zip(order, node_color):
            colour[int(node)] = CLASSES.index(name)
        row = state_row(box["env"], box["ordinal"])
        row["colour"] = colour
        rows.append(row)

    real_plt, real_nx = ref_graph.plt, ref_graph.nx
    ref_graph.plt, ref_graph.nx = _Pyplot, _Networkx(real_nx, sink)
    try:
        env = ref_graph.GraphEnv(graph=fixture_graph_12(), render_mode="human", number_of_agents=N, radius=0.2,
                                 dynamic_graph=dynamic)
        box.update(env=env, ordinal=0)
        rows.clear()                                # (the constructor's own resets draw nothing, but stay safe)
        pz = RefPettingZoo(env)
        tape = np.random.RandomState(tape_seed).randint(0, 2, size=max_steps)

        def reset_row():
            row = state_row(env, box["ordinal"])
            row["colour"] = np.full(N, -1, dtype=np.int8)           # the reference draws nothing at a reset
            rows.append(row)

        pz.reset()
        reset_row()
        done_count = 0
        for t in range(max_steps):
            _obs, term, trunc, info = pz.step(int(tape[t]))
            if term or trunc:
                done_count += 1
                if done_count == N or info.get("explicit_reset", False):
                    box["ordinal"] += 1
                    if box["ordinal"] == episodes:
                        break
                    pz.reset()
                    reset_row()
                    done_count = 0
        else:
            raise RuntimeError("the tape ended before the episodes did")
    finally:
        ref_graph.plt, ref_graph.nx = real_plt, real_nx
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def main():
    out = {}
    for name, dynamic, env_seed, tape_seed in (("static", False, 31, 21), ("dynamic", True, 32, 22)):
        trace = run_trace(dynamic, env_seed, tape_seed)
        drawn = int((trace["colour"][:, 0] >= 0).sum())
        print(f"{name}: {len(trace['ordinal'])} states, {drawn} drawn, classes used "
              f"{sorted({CLASSES[c] for c in trace['colour'].reshape(-1) if c >= 0})}")
        out.update({f"{name}_{k}": v for k, v in trace.items()})
    path = os.path.join(HERE, "render_trace_n12_fixture.npz")
    np.savez_compressed(path, classes=np.array(CLASSES), **out)
    print(f"-> {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()
