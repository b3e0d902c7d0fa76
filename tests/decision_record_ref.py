"""NumPy model of ``mel_decision_record_round`` (include/melissa_hip.h): the booking rules restated on plain arrays, one
``launch(state, live, logits, act, row_offsets)`` per device launch.  ``state``: dict of the env batch's arrays as the launch
finds them -

    scalars int32 [B, 16], node_sets uint64 [B, 8, W], sel_sets uint64 [B, 4, W], degree [B, N] (column 2 of obs_matrix)

``live`` uint64 [B, W]; ``logits`` float32 [rows, 2]; ``act`` int32 [rows] with ``row_offsets`` int32 [B + 1] (the rows of env b
are one per member of live[b], ascending) or, ``row_offsets=None``, the dense [B * N] layout with logits row b for every agent of
env b.  The arithmetic is the device's: ``np.float32`` subtraction for the gap, everything else in float64, the decisions of an
env added one after the other in ascending node id.

The model keeps what the device keeps (``by_round``, ``by_degree``, ``overflow``, ``skipped``, the trace rings and cursors) and,
beside the rings, every trace record ever written (``all_records``) and every row ever added (``addends``: (env, round or None,
degree row, row of 8 doubles)) for tests that bound a re-ordered sum.
"""
import numpy as np

S_NUM_MOVES, S_EPISODE, S_EPISODES_DONE, S_ERROR = 3, 6, 10, 11
SET_SCRIPTED, SEL_TAKEN_ACTION = 3, 3
FIELDS = 8


def members(words, n) -> list:
    """uint64 [W] node set -> ascending member ids below n."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    return [i for i in range(n) if (int(words[i // 64]) >> (i % 64)) & 1]


def pack(ids, n) -> np.ndarray:
    """member ids -> uint64 [W] node set."""
    out = np.zeros((n + 63) // 64, dtype=np.uint64)
    for i in ids:
        out[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return out


def greedy(q) -> int:
    """The fused selection at eps = 0: the first maximum (strict >, from -inf)."""
    best, bv = 0, np.float32(-np.inf)
    for a in range(len(q)):
        if np.float32(q[a]) > bv:
            best, bv = a, np.float32(q[a])
    return best


class DecisionRecordModel:
    def __init__(self, n_envs, n_nodes, max_rounds, n_degrees, trace_envs=(), trace_capacity=64, quota=None):
        self.B, self.n, self.R, self.D = int(n_envs), int(n_nodes), int(max_rounds), int(n_degrees)
        self.W = (self.n + 63) // 64
        self.trace_envs, self.cap = [int(t) for t in trace_envs], int(trace_capacity)
        self.quota = None if quota is None else np.asarray(quota, dtype=np.int64)
        self.reset()

    def reset(self):
        B, R, D, n, W, T, cap = self.B, self.R, self.D, self.n, self.W, len(self.trace_envs), self.cap
        self.by_round, self.by_degree = np.zeros((B, R, FIELDS)), np.zeros((B, D, FIELDS))
        self.overflow, self.skipped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.cursor = np.zeros(T, dtype=np.int64)
        self.ring = dict(meta=np.zeros((T, cap, 8), dtype=np.int32), sets=np.zeros((T, cap, 2, W), dtype=np.uint64),
                         q=np.zeros((T, cap, n, 2), dtype=np.float32))
        self.all_records = {t: [] for t in self.trace_envs}
        self.addends = []

    def launch(self, state, live, logits, act, row_offsets=None):
        live = np.asarray(live).view(np.uint64).reshape(self.B, self.W)
        logits = np.asarray(logits, dtype=np.float32).reshape(-1, 2)
        act = np.asarray(act, dtype=np.int32).reshape(-1)
        for b in range(self.B):
            self._env(b, state, live[b], logits, act, row_offsets)

    def _env(self, b, st, live, logits, act, row_offsets):
        sc = st["scalars"][b]
        if int(sc[S_ERROR]) != 0:
            self.skipped[b] += 1
            return
        ep, mv = int(sc[S_EPISODES_DONE]), int(sc[S_NUM_MOVES])
        if self.quota is not None and ep >= int(self.quota[b]):
            return
        n = self.n
        alive = members(live, n)
        scripted = set(members(np.asarray(st["node_sets"][b], dtype=np.uint64).reshape(8, -1)[SET_SCRIPTED], n))
        taken = set(members(np.asarray(st["sel_sets"][b], dtype=np.uint64).reshape(4, -1)[SEL_TAKEN_ACTION], n))
        deciding, relaying = [], []
        q_of = np.zeros((n, 2), dtype=np.float32)
        for rank, i in enumerate(alive):
            if i in scripted:
                continue
            row = int(row_offsets[b]) + rank if row_offsets is not None else b
            q = logits[row]
            a = int(act[row] if row_offsets is not None else act[b * n + i])
            d = int(np.float32(st["degree"][b][i]))
            d = min(max(d, 0), self.D - 1)
            gap = np.float64(np.float32(q[1]) - np.float32(q[0]))          # one fp32 subtraction, widened
            v = np.array([1.0, 1.0 if a == 1 else 0.0, gap, gap * gap, np.float64(q[1] if a == 1 else q[0]),
                          np.float64(q[1] if q[1] > q[0] else q[0]), 1.0 if a != greedy(q) else 0.0,
                          0.0 if i in taken else 1.0], dtype=np.float64)
            if 0 <= mv < self.R:
                self.by_round[b, mv] += v
            else:
                self.overflow[b] += 1
            self.by_degree[b, d] += v
            self.addends.append((b, mv if 0 <= mv < self.R else None, d, v))
            deciding.append(i)
            q_of[i] = q
            if a == 1:
                relaying.append(i)
        if deciding and b in self.trace_envs:
            t = self.trace_envs.index(b)
            rec = dict(meta=np.array([b, ep, int(sc[S_EPISODE]), mv, len(deciding), len(relaying), 0, 0], dtype=np.int32),
                       sets=np.stack([pack(deciding, n), pack(relaying, n)]), q=q_of)
            slot = int(self.cursor[t] % self.cap)
            for k, v_ in rec.items():
                self.ring[k][t, slot] = v_
            self.cursor[t] += 1
            self.all_records[b].append(rec)

    def folded(self):
        """by_round / by_degree added over the envs in ascending order (what mel_decision_record_read returns), the counters."""
        by_round, by_degree = np.zeros((self.R, FIELDS)), np.zeros((self.D, FIELDS))
        for b in range(self.B):
            by_round, by_degree = by_round + self.by_round[b], by_degree + self.by_degree[b]
        return by_round, by_degree, dict(overflow=int(self.overflow.sum()), skipped=int(self.skipped.sum()))


def state_of(venv) -> dict:
    """The arrays a launch reads, copied from a ``HipGraphVectorEnv`` (synchronises)."""
    import torch
    B, n, W = venv.env_num, venv.n, (venv.n + 63) // 64
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    return dict(scalars=venv.scalars().cpu().numpy().copy(), node_sets=u64(venv.node_sets()).reshape(B, 8, W).copy(),
                sel_sets=u64(venv._field(venv.env.sel_sets, 4 * W, torch.int64)).reshape(B, 4, W).copy(),
                degree=venv.obs_matrix().cpu().numpy().reshape(B, n, 8)[:, :, 2].copy())
