"""Draw a recorded episode: the reference's ``draw_graph`` (graph.py:466-484) from a trace of
:class:`melissa_amd.round_record.RoundRecorder`, as one hand-written SVG per round (no plotting library).

An episode trace is one dict of :func:`melissa_amd.round_record.group_episodes`: per recorded round the node positions, the
``one_hop`` adjacency node sets, six node sets (``_lib.RR_TRACE_SETS``) and per node the messages transmitted and received.
"""
from __future__ import annotations

import os

import numpy as np

from ._lib import RR_TRACE_SETS

CLASSES = ("green", "blue", "purple", "red", "yellow")
FILL = {"green": "#2ca02c", "blue": "#1f77b4", "purple": "#9467bd", "red": "#d62728", "yellow": "#ffdd33"}


def members(words, n: int) -> np.ndarray:
    """A node set (uint64 words, word k = nodes 64 k .. 64 k + 63) -> bool [n]."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    node = np.arange(n)
    return ((words[node // 64] >> (node % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)


def edges(one_hop, n: int) -> list:
    """``one_hop`` uint64 [N, W] -> the undirected edges (i, j), i < j, in order."""
    rows = np.stack([members(one_hop[i], n) for i in range(n)])
    return [(i, j) for i in range(n) for j in range(i + 1, n) if rows[i, j] or rows[j, i]]


def transmitted_to_somebody(episode_trace) -> np.ndarray:
    """bool [K, N]: ``sum(state.transmitted_to) > 0`` after each recorded round.  Not env state: a relay adds the sender's
    neighbours of the graph BEFORE the round's move (core.py:249-257,269), so a node has transmitted to somebody once its
    ``agent_msgs`` grew in a round whose previous record shows it with a neighbour; at round 0 (the reset's forced first
    transmission, core.py:246,437) it is the origin."""
    msgs, one_hop = np.asarray(episode_trace["agent_msgs"]), np.asarray(episode_trace["one_hop"])
    K, n = msgs.shape
    out = np.zeros((K, n), dtype=bool)
    for k in range(K):
        if k == 0:
            if int(episode_trace["rounds"][0]) == 0:
                out[0, int(episode_trace["origin"])] = msgs[0, int(episode_trace["origin"])] > 0
            continue
        had_neighbour = one_hop[k - 1].reshape(n, -1).any(axis=1)
        out[k] = out[k - 1] | ((msgs[k] > msgs[k - 1]) & had_neighbour)
    return out


def colour_classes(episode_trace) -> list:
    """The reference's colour of every node after each recorded round, by its rule in its order (graph.py:472-481): ``green``
    received something and transmitted to nobody, ``blue`` the origin, ``purple`` more than one transmission, ``red``
    transmitted to somebody, ``yellow`` everything else.  -> K lists of N class names."""
    msgs, received = np.asarray(episode_trace["agent_msgs"]), np.asarray(episode_trace["received"])
    K, n = msgs.shape
    sent = transmitted_to_somebody(episode_trace)
    origin_at = RR_TRACE_SETS.index("origin")
    out = []
    for k in range(K):
        origin = members(episode_trace["sets"][k][origin_at], n)
        row = []
        for i in range(n):
            if received[k, i] > 0 and not sent[k, i]:
                row.append("green")
            elif origin[i]:
                row.append("blue")
            elif msgs[k, i] > 1:
                row.append("purple")
            elif sent[k, i]:
                row.append("red")
            else:
                row.append("yellow")
        out.append(row)
    return out


def svg_frame(pos, one_hop, classes, title: str = "", size: int = 480, margin: int = 24) -> str:
    """One frame: a line per edge, a circle per node filled by its class, the node id as a label."""
    pos = np.asarray(pos, dtype=np.float64)
    n = pos.shape[0]
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    span = float(max((hi - lo).max(), 1e-9))
    xy = margin + (pos - lo) / span * (size - 2 * margin)
    xy[:, 1] = size - xy[:, 1]                     # y upwards, as a plot draws it
    out = [f'<svg xmlns="http://www.w3.org/2000/svg" width="{size}" height="{size}" viewBox="0 0 {size} {size}">',
           f'<title>{title}</title>', f'<rect width="{size}" height="{size}" fill="white"/>']
    for i, j in edges(one_hop, n):
        out.append(f'<line x1="{xy[i, 0]:.2f}" y1="{xy[i, 1]:.2f}" x2="{xy[j, 0]:.2f}" y2="{xy[j, 1]:.2f}" stroke="#444444" '
                   f'stroke-width="1"/>')
    for i in range(n):
        out.append(f'<circle cx="{xy[i, 0]:.2f}" cy="{xy[i, 1]:.2f}" r="10" fill="{FILL[classes[i]]}" stroke="black" '
                   f'class="{classes[i]}"/>')
        out.append(f'<text x="{xy[i, 0]:.2f}" y="{xy[i, 1] + 4:.2f}" font-size="10" text-anchor="middle">{i}</text>')
    out.append("</svg>")
    return "\n".join(out) + "\n"


def write_svg_frames(episode_trace, out_dir: str) -> list:
    """One SVG per recorded round of the episode into ``out_dir`` (created): ``env<E>_ep<ordinal>_round<r>.svg`` -> the paths."""
    os.makedirs(out_dir, exist_ok=True)
    classes = colour_classes(episode_trace)
    paths = []
    for k, r in enumerate(np.asarray(episode_trace["rounds"]).tolist()):
        path = os.path.join(out_dir, f"env{int(episode_trace['env'])}_ep{int(episode_trace['ordinal']):04d}_round{int(r):03d}.svg")
        title = f"env {int(episode_trace['env'])} episode {int(episode_trace['ordinal'])} round {int(r)}: " \
                f"{int(episode_trace['world_msgs'][k])} messages"
        with open(path, "w") as f:
            f.write(svg_frame(episode_trace["pos"][k], episode_trace["one_hop"][k], classes[k], title))
        paths.append(path)
    return paths
