"""References of the inference path's conv2 coefficients (``mel_forward_attention``) and a NumPy model of
``mel_attention_record_round`` (include/melissa_hip.h) - shared by tests/test_attention_record_ref.py (CPU: the references
themselves, the measurement behind every bound, the booking rules on hand examples) and the two GPU test files.

Coefficients.  ``alpha64``: the float64 softmax from given ``x_l2`` / ``x_r2`` / ``att`` rows over given sources.  ``alpha32``: a
float32 restatement in the device's expression order - per lane an even and an odd fused-multiply-add chain over its channels,
their sum, the head's lanes added in a butterfly, ``exp`` as ``exp2(x * log2 e)`` in float32, the sum of the exponentials in
ascending source order, one reciprocal.  ``x3_64`` / ``x3_32``: ``relu(sum_k alpha_k * value_k + bias)``, the x_3 block of the
head input, in float64 and as a float32 fused-multiply-add chain in ascending source order.

Bounds.  ``ALPHA_TOL`` / ``X3_TOL`` are 8 times the largest error of ``alpha32`` / ``x3_32`` against float64 on ``CELLS``, the
cells the GPU tests run (8: the convention of tests/shape_grid_ref.py - the kernels use the hardware exp2 and reciprocal and
another summation order than either CPU evaluation).  tests/test_attention_record_ref.py measures them and holds the constants
to the measurement.

Booking.  ``AttentionRecordModel.launch(state, live, alpha, sources, row_offsets)``: the rules of the header on plain arrays;
``state`` as ``tests.decision_record_ref.state_of`` gives it.  Every field is a fixed sequence of float64 operations.
"""
import functools
import math

import numpy as np
import torch

from melissa_amd.shapes import head_lanes
from oracle import net_oracle as no
from tests.decision_record_ref import S_EPISODE, S_EPISODES_DONE, S_ERROR, S_NUM_MOVES, SET_SCRIPTED, members, pack, state_of  # noqa: F401
from tests.shape_grid_ref import agent_words, weights  # noqa: F401

SET_HAS_MESSAGE, SET_INTERESTED = 0, 2
FIELDS, MAX_SOURCES = 8, 34
LOG2E = np.float32(1.44269504088896341)

# ---- the cells -------------------------------------------------------------------------------------------------------
# (hidden, heads, model, n, bs).  12 nodes x 4 envs: env 0 one agent, node 0, alone in a corner (DGN-R: an agent without a
# source), env 1 every node an agent inside a 0.15 box, env 2 no agent, env 3 a few; 70 x 2 (two set words): env 0 every node
# inside a 0.1 box - every row is cut at the neighbour cap, 34 sources for GATv2 -, env 1 agents 0, 63, 64 and 69.
# (64, 6): 48 live lanes; (64, 16): 4 lanes per head, the most heads; (512, 1): one head on 64 lanes, 8 channels each.
CELLS = ((128, 4, "l_dgn", 12, 4), (128, 4, "l_dgn", 70, 2), (64, 6, "l_dgn", 12, 4), (64, 16, "l_dgn", 12, 4),
         (512, 1, "l_dgn", 12, 4), (128, 4, "dgn_r", 12, 4))
cell_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}-n{c[3]}"
TABLE_CELL = (128, 4, "l_dgn", 7, 48)           # past the 40 envs from which the agents forward takes the node-feature table


@functools.lru_cache(maxsize=None)
def cell_inputs(n, bs):
    """-> (obs [bs, 8 n + 1] float32 with integer features, agent sets bool [bs, n])."""
    rng = np.random.RandomState(4000 + n + bs)
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, 0.45 if n < 64 else 0.3, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, min(n, 9), size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = rng.uniform(size=(bs, n)) >= 0.2
    live = np.zeros((bs, n), dtype=bool)
    if n > 64:
        m[0, :, 0:2] = 0.3 + rng.uniform(0, 0.1, size=(n, 2))
        live[0] = True
        live[1, [0, 63, 64, 69]] = True
    elif bs == 4:
        m[0, :, 0:2] = 0.6 + rng.uniform(0, 0.35, size=(n, 2))
        m[0, 0, 0:2], m[0, 0, 7] = 0.0, 1
        live[0, 0] = True
        m[1, :, 0:2] = 0.3 + rng.uniform(0, 0.15, size=(n, 2))
        live[1] = True
        live[3, rng.choice(n, size=4, replace=False)] = True
    else:
        for b in range(bs):
            live[b, rng.choice(n, size=rng.randint(1, n + 1), replace=False)] = True
    return obs, live


def adjacency(obs, n):
    """bool [bs, n, n], [b, i, j]: edge j -> i - the oracle's radius rule on the float32 positions."""
    bs = obs.shape[0]
    return no.radius_adjacency(torch.from_numpy(obs[:, :-1]).reshape(bs, n, 8)[:, :, :2].float()).numpy()


def source_sets(adj, gat):
    """conv2's source sets: GATv2 the closed neighbourhood, TransformerConv the open one."""
    return adj | np.eye(adj.shape[1], dtype=bool)[None] if gat else adj.copy()


def conv2_rows64(cell):
    """The rows conv2's attention reads, float64, full graphs: (x_l2 [bs, n, hc] (keys), values [bs, n, hc], x_r2 [bs, n, hc],
    att [hc] or None, bias [hc] or None, adjacency)."""
    hidden, heads, model, n, bs = cell
    obs, _live = cell_inputs(n, bs)
    sd = {k: v.double() for k, v in weights(model, hidden, heads).items()}
    torch.set_num_threads(8)
    with torch.no_grad():
        sd, feats, dm, adj, _gi, bs, n = no._inputs(sd, obs, n, torch.float64, None)
        x = torch.relu(no._mlp(sd, "encoder", feats.reshape(bs * n, -1), 2))
        conv1 = no.gatv2_dense if model == "l_dgn" else no.transformer_dense
        h1 = torch.relu(conv1(sd, "conv1", x, adj, heads)) * dm.reshape(bs * n, 1)
        lin = lambda name: (h1 @ sd[f"conv2.{name}.weight"].t() + sd[f"conv2.{name}.bias"]).reshape(bs, n, -1).numpy()
        if model == "l_dgn":
            xl = lin("lin_l")
            return xl, xl, lin("lin_r"), sd["conv2.att"].reshape(-1).numpy(), sd["conv2.bias"].numpy(), adj.numpy()
        return lin("lin_key"), lin("lin_value"), lin("lin_query"), None, None, adj.numpy()


# ---- the coefficients ------------------------------------------------------------------------------------------------
def alpha64(x_l, x_r, att, heads):
    """x_l [c, heads * C] (the sources' rows in ascending node id), x_r [heads * C], att [heads * C] or None (TransformerConv)
    -> alpha float64 [c, heads]; c = 0 gives an empty array."""
    if len(x_l) == 0:
        return np.zeros((0, heads))
    x_l, x_r = np.asarray(x_l, dtype=np.float64).reshape(len(x_l), heads, -1), np.asarray(x_r, dtype=np.float64).reshape(heads, -1)
    if att is not None:
        z = x_l + x_r[None]
        e = (np.where(z > 0, z, 0.2 * z) * np.asarray(att, dtype=np.float64).reshape(1, heads, -1)).sum(-1)
    else:
        e = (x_l * x_r[None]).sum(-1) / math.sqrt(x_l.shape[-1])
    p = np.exp(e - e.max(0, keepdims=True))
    return p / (p.sum(0, keepdims=True) + 1e-16)


def _fma32(a, b, c):
    """float32 fused multiply-add: the product of two floats is exact in float64, the sum is rounded there once and once more
    to float32 (a double rounding that differs from the fused one in about one case of 2^29)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def alpha32(x_l, x_r, att, heads):
    """The same in float32, in the device's expression order -> float32 [c, heads]."""
    c = len(x_l)
    if c == 0:
        return np.zeros((0, heads), dtype=np.float32)
    channels = np.asarray(x_l).shape[-1] // heads
    lanes, _live, vpl, why = head_lanes(heads, channels)
    assert why is None, why
    xl = np.asarray(x_l, dtype=np.float32).reshape(c, heads, lanes, vpl)
    xr = np.asarray(x_r, dtype=np.float32).reshape(1, heads, lanes, vpl)
    if att is not None:
        a = np.asarray(att, dtype=np.float32).reshape(1, heads, lanes, vpl)
        z = xr + xl
        zm = np.maximum(z, z * np.float32(0.2))
        even, odd = np.zeros((c, heads, lanes), dtype=np.float32), np.zeros((c, heads, lanes), dtype=np.float32)
        for i in range(0, vpl, 2):
            even, odd = _fma32(np.broadcast_to(a[..., i], even.shape), zm[..., i], even), \
                _fma32(np.broadcast_to(a[..., i + 1], odd.shape), zm[..., i + 1], odd)
        t = even + odd
    else:
        t = np.zeros((c, heads, lanes), dtype=np.float32)
        for i in range(vpl):
            t = _fma32(np.broadcast_to(xr[..., i], t.shape), xl[..., i], t)
    idx = np.arange(lanes)
    steps = [1 << k for k in range(lanes.bit_length() - 1)]
    for o in (steps if lanes == 16 else steps[::-1]):          # 16 lanes: the DPP moves, nearest first; else shuffles, farthest first
        t = t + t[..., idx ^ o]
    s = t[..., 0]
    if att is None:
        s = s * np.float32(1.0 / np.sqrt(np.float32(channels)))
    m = s.max(0, keepdims=True)
    p = np.exp2((s - m) * LOG2E).astype(np.float32)
    total = np.zeros(heads, dtype=np.float32)
    for k in range(c):
        total = total + p[k]
    return p * (np.float32(1.0) / (total + np.float32(1e-16)))


def x3_64(alpha, values, bias, heads):
    """relu(sum_k alpha[k, h] * values[k, h, :] + bias) -> float64 [heads * C]; no source: relu(bias)."""
    width = np.asarray(values).shape[-1]
    values = np.asarray(values, dtype=np.float64).reshape(len(values), heads, width // heads)
    out = (np.asarray(alpha, dtype=np.float64)[:, :, None] * values).sum(0).reshape(-1)
    return np.maximum(out + (0.0 if bias is None else np.asarray(bias, dtype=np.float64)), 0.0)


def x3_32(alpha, values, bias, heads):
    """The same as a float32 fused-multiply-add chain in ascending source order."""
    width = np.asarray(values).shape[-1]
    values = np.asarray(values, dtype=np.float32).reshape(len(values), heads, width // heads)
    alpha = np.asarray(alpha, dtype=np.float32)
    out = np.zeros(values.shape[1:], dtype=np.float32)
    for k in range(len(values)):
        out = _fma32(np.broadcast_to(alpha[k][:, None], out.shape), values[k], out)
    out = out.reshape(-1)
    if bias is not None:
        out = out + np.asarray(bias, dtype=np.float32)
    return np.maximum(out, np.float32(0))


def agent_rows(live):
    """(env, agent) of every agent row: by env, then agent id."""
    return [(int(b), int(a)) for b, a in zip(*np.nonzero(live))]


def measure(cell):
    """-> (largest |alpha32 - alpha64|, largest |x3_32 - x3_64|) over the cell's agent rows, both sides on the float32 rows."""
    hidden, heads, model, n, bs = cell
    _obs, live = cell_inputs(n, bs)
    keys, values, queries, att, bias, adj = conv2_rows64(cell)
    keys, values, queries = (a.astype(np.float32) for a in (keys, values, queries))
    src = source_sets(adj, model == "l_dgn")
    worst_a = worst_x = 0.0
    for b, i in agent_rows(live):
        js = np.flatnonzero(src[b, i])
        a64, a32 = alpha64(keys[b, js], queries[b, i], att, heads), alpha32(keys[b, js], queries[b, i], att, heads)
        if len(js):
            worst_a = max(worst_a, float(np.abs(a32.astype(np.float64) - a64).max()))
        x64, x32 = x3_64(a64, values[b, js], bias, heads), x3_32(a32, values[b, js], bias, heads)
        worst_x = max(worst_x, float(np.abs(x32.astype(np.float64) - x64).max()))
    return worst_a, worst_x


# ---- the bounds ------------------------------------------------------------------------------------------------------
# 8 x the largest error of the float32 restatements against float64 over CELLS (test_bounds_are_eight_times_the_measured_error)
ALPHA_TOL = 2.7e-7         # measured 3.39e-08 (64 x 16 L-DGN)
X3_TOL = 1.2e-6            # measured 1.53e-07 (512 x 1 L-DGN)


# ---- the booking rules -----------------------------------------------------------------------------------------------
def decision_fields(alpha_row, src_ids, i, has, waiting):
    """The eight fields of ONE head of ONE decision: ``alpha_row`` float32 [c] (the head's coefficients of the sources
    ``src_ids`` in ascending node id), ``i`` the deciding node, ``has`` / ``waiting`` sets of node ids."""
    c = len(src_ids)
    v = np.zeros(FIELDS, dtype=np.float64)
    v[0] = 1.0
    if c == 0:
        return v
    informed = wait = 0
    for k, j in enumerate(src_ids):
        al = np.float64(np.float32(alpha_row[k]))
        if j == i:
            v[1] = al
        elif j in has:
            v[2] = v[2] + al
            informed += 1
        elif j in waiting:
            v[4] = v[4] + al
            wait += 1
        v[6] = v[6] + al * al
        v[7] = al if al > v[7] else v[7]
    v[3], v[5] = np.float64(informed) / np.float64(c), np.float64(wait) / np.float64(c)
    return v


class AttentionRecordModel:
    def __init__(self, n_envs, n_nodes, max_rounds, n_degrees, heads, trace_envs=(), trace_capacity=64, quota=None):
        self.B, self.n, self.R, self.D, self.H = int(n_envs), int(n_nodes), int(max_rounds), int(n_degrees), int(heads)
        self.W = (self.n + 63) // 64
        self.trace_envs, self.cap = [int(t) for t in trace_envs], int(trace_capacity)
        self.quota = None if quota is None else np.asarray(quota, dtype=np.int64)
        self.reset()

    def reset(self):
        B, R, D, H, n, W, T, cap = self.B, self.R, self.D, self.H, self.n, self.W, len(self.trace_envs), self.cap
        self.by_round, self.by_degree, self.by_head = np.zeros((B, R, FIELDS)), np.zeros((B, D, FIELDS)), np.zeros((B, H, FIELDS))
        self.overflow, self.skipped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.cursor = np.zeros(T, dtype=np.int64)
        self.ring = dict(meta=np.zeros((T, cap, 8), dtype=np.int32), sets=np.zeros((T, cap, W), dtype=np.uint64),
                         fields=np.zeros((T, cap, n, FIELDS), dtype=np.float64))
        self.all_records = {t: [] for t in self.trace_envs}
        self.booked = []           # (env, node, source count, informed sources, waiting sources) of every decision booked

    def launch(self, state, live, alpha, sources, row_offsets):
        live = np.asarray(live).view(np.uint64).reshape(self.B, self.W)
        alpha = np.asarray(alpha, dtype=np.float32).reshape(-1, MAX_SOURCES, self.H)
        sources = np.asarray(sources).view(np.uint64).reshape(-1, self.W)
        for b in range(self.B):
            self._env(b, state, live[b], alpha, sources, row_offsets)

    def _env(self, b, st, live, alpha, sources, row_offsets):
        sc = st["scalars"][b]
        if int(sc[S_ERROR]) != 0:
            self.skipped[b] += 1
            return
        ep, mv = int(sc[S_EPISODES_DONE]), int(sc[S_NUM_MOVES])
        if self.quota is not None and ep >= int(self.quota[b]):
            return
        n, H = self.n, self.H
        sets = np.asarray(st["node_sets"][b], dtype=np.uint64).reshape(8, -1)
        scripted, has = set(members(sets[SET_SCRIPTED], n)), set(members(sets[SET_HAS_MESSAGE], n))
        waiting = set(members(sets[SET_INTERESTED], n)) - has
        deciding, empty = [], 0
        fields_of = np.zeros((n, FIELDS), dtype=np.float64)
        for rank, i in enumerate(members(live, n)):
            if i in scripted:
                continue
            row = int(row_offsets[b]) + rank
            src = members(sources[row], n)[:MAX_SOURCES]
            per_head = np.stack([decision_fields(alpha[row, :len(src), h], src, i, has, waiting) for h in range(H)])
            total = np.zeros(FIELDS, dtype=np.float64)
            for h in range(H):                                   # the head mean: ascending heads, one division
                total = total + per_head[h]
                self.by_head[b, h] += per_head[h]
            mean = total / np.float64(H)
            d = min(max(int(np.float32(st["degree"][b][i])), 0), self.D - 1)
            if 0 <= mv < self.R:
                self.by_round[b, mv] += mean
            else:
                self.overflow[b] += 1
            self.by_degree[b, d] += mean
            deciding.append(i)
            fields_of[i] = mean
            empty += not src
            others = [j for j in src if j != i]
            self.booked.append((b, i, len(src), sum(j in has for j in others), sum(j in waiting for j in others)))
        if deciding and b in self.trace_envs:
            t = self.trace_envs.index(b)
            rec = dict(meta=np.array([b, ep, int(sc[S_EPISODE]), mv, len(deciding), empty, 0, 0], dtype=np.int32),
                       sets=pack(deciding, n), fields=fields_of)
            slot = int(self.cursor[t] % self.cap)
            for k, v_ in rec.items():
                self.ring[k][t, slot] = v_
            self.cursor[t] += 1
            self.all_records[b].append(rec)

    def folded(self):
        """The three tables added over the envs in ascending order (what mel_attention_record_read returns), the counters."""
        out = [np.zeros((rows, FIELDS)) for rows in (self.R, self.D, self.H)]
        for b in range(self.B):
            out = [o + t[b] for o, t in zip(out, (self.by_round, self.by_degree, self.by_head))]
        return (*out, dict(overflow=int(self.overflow.sum()), skipped=int(self.skipped.sum())))


def fold_records(records_by_env, B, R, D, H, degree_of):
    """by_round / by_degree per env from trace records alone (``records_by_env[b]``: env b's records in play order, each with
    ``meta`` and ``fields``; ``degree_of(b, record index, node)`` -> the degree row): the sums the device made, in its order."""
    by_round, by_degree = np.zeros((B, R, FIELDS)), np.zeros((B, D, FIELDS))
    for b, records in records_by_env.items():
        for k, rec in enumerate(records):
            mv = int(rec["meta"][3])
            for i in members(rec["sets"], rec["fields"].shape[0]):
                if 0 <= mv < R:
                    by_round[b, mv] += rec["fields"][i]
                by_degree[b, degree_of(b, k, i)] += rec["fields"][i]
    return by_round, by_degree
