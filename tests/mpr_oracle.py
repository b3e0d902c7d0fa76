"""CPU restatement of the "mpr" scripted-agent heuristic (TEST INFRASTRUCTURE, like oracle/env_oracle.py).

Reference: heuristics/mpr.py:7-72 (OLSR multipoint relays, RFC 3626) read as ``HeuristicResult(relay_mask=mpr,
action=None)`` - ``mpr_heuristic`` returns the bare array where ``World.step`` reads ``result.relay_mask``
(core.py:227-234) - and the relays_for / received_from half of ``World.step`` that only a relay mask reaches
(core.py:229-243,276-278).  Pinned by ``tests/golden/mpr_sets_*.npz`` (the reference's sets on fixed graphs) and
``tests/golden/mpr_trace_*.npz`` (the real GraphEnv run with that reading), both written by
``tests/golden/make_mpr_golden.py``.

Node sets are Python ints (bit i = node i), as in oracle/env_oracle.py.
"""
from __future__ import annotations

import numpy as np

from oracle.env_oracle import OracleGraphEnv, bits, popcount


def mpr_set(adj: list, v: int) -> int:
    """MPR set of node v in the undirected graph ``adj`` (one-hop bit masks).

    N1 = one-hop set, N2 = two-hop set minus N1 and v (mpr.py:18).  (1) Every node of N2 that exactly one neighbour
    reaches makes that neighbour a relay and counts as covered - only those nodes (:43-47).  (2) While N2 has uncovered
    nodes, the neighbour reaching most of them - the largest id among equals (max over the dict keys, :60-66; the d_y
    degrees are never compared) - becomes a relay (possibly again) and what it reaches counts as covered (:52-70)."""
    n1 = adj[v]
    reach = 0
    for u in bits(n1):
        reach |= adj[u]
    n2 = reach & ~n1 & ~(1 << v)
    providers = {x: [u for u in bits(n1) if (adj[u] >> x) & 1] for x in bits(n2)}
    mpr, covered = 0, 0
    for x, cands in providers.items():
        if len(cands) == 1:
            mpr |= 1 << cands[0]
            covered |= 1 << x
    left = n2 & ~covered
    for _ in range(popcount(n2)):
        if not left:
            break
        counts = {u: popcount(adj[u] & left) for u in bits(n1)}
        top = max(counts.values())
        pick = max(u for u, c in counts.items() if c == top)
        mpr |= 1 << pick
        left &= ~adj[pick]
    return mpr


def mpr_sets_batch(adj: np.ndarray) -> np.ndarray:
    """:func:`mpr_set` of every node of a batch of graphs at once, in numpy: ``adj`` bool [G, N, N] (symmetric, no self
    loops) -> bool [G, N, N], row v = the MPR set of v.  Reach counts are matrix products (float32: exact below 2^24)."""
    a = adj.astype(np.float32)
    g, n, _ = adj.shape
    eye = np.eye(n, dtype=bool)[None]
    cnt = a @ a                                                    # [g, v, x]: neighbours of v that reach x
    n2 = (cnt > 0) & ~adj & ~eye
    unique = n2 & (cnt == 1)
    mpr = adj & ((unique.astype(np.float32) @ a) > 0)             # (1) providers of uniquely reached nodes
    left = n2 & ~unique
    ids = np.arange(n)
    for _ in range(n):                                             # (2) one pick per (graph, node) with uncovered nodes
        busy = left.any(axis=2)
        if not busy.any():
            break
        r = np.where(adj, left.astype(np.float32) @ a, -1.0)      # [g, v, u]: uncovered nodes neighbour u reaches
        pick = np.argmax(r * (n + 1) + ids[None, None, :], axis=2)   # most reached, then the largest id
        gi, vi = np.nonzero(busy)
        ui = pick[gi, vi]
        mpr[gi, vi, ui] = True
        left[gi, vi] &= ~adj[gi, ui]
    return mpr


class MprOracleGraphEnv(OracleGraphEnv):
    """``OracleGraphEnv`` with ``heuristic="mpr"``: every scripted agent names its MPR set at every world step; a
    scripted node that some scripted agent named transmits only if it has not transmitted yet, holds the message (or is
    the source) and received it from one of the agents that named it (or is the source), and stays silent otherwise;
    other scripted agents keep the action ``_execute_world_step`` gave them (None in training mode, the policy's in
    testing mode).  ``forwards`` counts the transmissions of scripted non-source nodes that this rule allowed,
    ``relay_duties`` the (world step, scripted node) pairs it applied to."""

    def __init__(self, number_of_agents, *args, scripted_agents_ratio=0.0, heuristic="mpr", **kwargs):
        if heuristic != "mpr":
            raise ValueError(f"MprOracleGraphEnv runs the mpr heuristic, not {heuristic}")
        if not (0.0 <= scripted_agents_ratio <= 1.0):
            raise ValueError("`scripted_agents_ratio` must be in [0.0, 1.0].")
        if scripted_agents_ratio == 0.0:
            raise ValueError("If `scripted_agents_ratio` is 0.0, no heuristic can be set.")
        self.forwards = self.relay_duties = 0
        self.relays_for = None
        # the base class knows only the action heuristics: it runs with none (no scripted action is overwritten by it)
        # and this class adds the relay-mask half of World.step around its world step
        super().__init__(number_of_agents, *args, scripted_agents_ratio=scripted_agents_ratio, heuristic=None, **kwargs)
        self.mpr_heuristic = "mpr"

    def _world_step(self):
        n = self.n
        if self.messages_transmitted == 0:        # the reset's own World.step (core.py:389,437): State.reset (:21-22)
            self.received_from = [0] * n
        # :226-234 relays_for[b] |= {a} for every b in M(a), a scripted (the graph of the previous move)
        self.relays_for = [0] * n
        for a in bits(self.scripted):
            for b in bits(mpr_set(self.adj, a)):
                self.relays_for[b] |= 1 << a
        # :236-243 only scripted nodes that some agent relays through
        for b in bits(self.scripted):
            if self.relays_for[b]:
                self.relay_duties += 1
                origin = (self.message_origin >> b) & 1
                holds = ((self.has_message | self.message_origin) >> b) & 1
                fresh = not (self.has_taken_action >> b) & 1
                self.agent_action[b] = 1 if fresh and holds and ((self.received_from[b] & self.relays_for[b]) or origin) else 0
        super()._world_step()                      # :246-261 source override, relay loop, move, two-hop cover
        for i in bits(self.scripted):              # :263-266
            self.agent_action[i] = 0
        self.relays_for = [0] * n

    def _relay_message(self, i):
        super()._relay_message(i)
        for j in bits(self.adj[i]):                # :276-278 received_from[j][i] += 1
            self.received_from[j] |= 1 << i
        if (self.scripted >> i) & 1 and self.relays_for and self.relays_for[i] and i != self.origin_agent:
            self.forwards += 1
