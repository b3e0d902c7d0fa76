"""float64 NumPy restatement of the two training-log launches (``mel_train_log_round`` / ``mel_train_log_update``,
melissa_amd/csrc/train_log.hpp; contract at ``mel_train_log`` in include/melissa_hip.h): the record layout, the slot rule, the
clearing of a slot, the counters, and every sum in the order the kernels add in - so a record of the device equals the model's
bit for bit.  No torch, no GPU."""
import math

import numpy as np

from melissa_amd import _lib as L

DOUBLES, CHUNK, LANES = L.TRAIN_LOG_DOUBLES, L.TRAIN_LOG_GRAD_CHUNK, 256
STAT_MESSAGES, STAT_COVERAGE, STAT_COV_INTERESTED, STAT_REWARD = 0, 1, 6, 9      # columns of a logger_stats row (graph.py:166-178)
INF = float("inf")


def empty_record() -> np.ndarray:
    r = np.zeros(DOUBLES)
    r[L.TL_REW_MIN] = INF
    for f in (L.TL_REW_MAX, L.TL_LOSS_MAX, L.TL_TD_ABS_MEAN_MAX, L.TL_TD_ABS_MAX, L.TL_GRAD_NORM_MAX):
        r[f] = -INF
    r[L.TL_EPS_LAST] = -1.0
    return r


def nan_max(m: float, v: float) -> float:
    """The kernels' compare: a NaN wins and then stays."""
    return v if (v > m or v != v) else m


def nan_min(m: float, v: float) -> float:
    return v if (v < m or v != v) else m


def tree_sum(lanes: np.ndarray) -> float:
    """lane t += lane t + o for o = 128, 64 .. 1 (``lanes``: float64 [256])."""
    a = np.array(lanes, dtype=np.float64)
    o = len(a) // 2
    while o > 0:
        a[:o] = a[:o] + a[o:2 * o]
        o //= 2
    return float(a[0])


def grad_sq_sum(grads) -> float:
    """The squared L2 norm of a gradient table as the device adds it: per MEL_TRAIN_LOG_GRAD_CHUNK elements of one tensor lane t
    adds its elements t, t + 256, ... in order (each widened to double and squared), the lanes meet in the tree; then 64 lanes
    add a run of consecutive chunk sums each and lane 0 adds the lanes in order."""
    partial = []
    for g in grads:
        g = np.asarray(g, dtype=np.float32).reshape(-1).astype(np.float64)
        for lo in range(0, len(g), CHUNK):
            c = g[lo:lo + CHUNK]
            sq = np.zeros(-(-len(c) // LANES) * LANES)
            sq[:len(c)] = c * c
            lanes = np.zeros(LANES)
            for row in sq.reshape(-1, LANES):
                lanes = lanes + row
            partial.append(tree_sum(lanes))
    groups, total = len(partial), 0.0
    per = (groups + 63) // 64
    for lane in range(64):
        s = 0.0
        for k in range(lane * per, min((lane + 1) * per, groups)):
            s += partial[k]
        total += s
    return total


def td_stats(td):
    """(sum_i |td_i|, max_i |td_i|) of a float32 vector as one wavefront computes them: lane l adds i = l, l + 64, ... in double,
    lane 0 adds the lanes in order."""
    a = np.abs(np.asarray(td, dtype=np.float32).astype(np.float64))
    asum, amax = 0.0, -INF
    for lane in range(64):
        s, m = 0.0, -INF
        for v in a[lane::64]:
            s += float(v)
            m = nan_max(m, float(v))
        asum += s
        amax = nan_max(amax, m)
    return asum, amax


class TrainLogModel:
    def __init__(self, capacity: int, interval: int):
        self.capacity, self.interval = int(capacity), int(interval)
        self.records = np.zeros((self.capacity, DOUBLES))
        self.interval_id = np.full(self.capacity, -1, dtype=np.int64)
        self.counters = np.zeros(4, dtype=np.int64)
        self.base = None                       # not armed
        self.drained_upto = 0

    def slot(self, env_step: int):
        """The record of ``env_step``'s interval (cleared and renamed when the slot held another one), or None."""
        if self.base is None or env_step < self.base:
            return None
        k = (env_step - self.base) // self.interval
        s = k % self.capacity
        old = int(self.interval_id[s])
        if old != k:
            if old >= 0 and old >= self.drained_upto:
                self.counters[L.TLC_LOST_RECORDS] += 1
            self.records[s] = empty_record()
            self.interval_id[s] = k
        return self.records[s]

    def round(self, env_step: int, stats, meta, cursor: int, log_capacity: int, n_envs: int, eps=None):
        """``stats`` float64 [rows, 10] / ``meta`` int32 [rows, 3]: the episode log's buffers (at least min(cursor, capacity) rows)."""
        n = min(max(int(cursor), 0), int(log_capacity))
        stats, meta = np.asarray(stats, dtype=np.float64)[:n], np.asarray(meta)[:n]
        acc = np.zeros((LANES, 9))
        acc[:, 3], acc[:, 4] = INF, -INF
        bad = dup = 0
        by_env = {}
        for r in range(n):
            b = int(meta[r, 0])
            if 0 <= b < n_envs:
                by_env.setdefault(b, []).append(r)
            else:
                bad += 1
        for b in sorted(by_env):
            rows = sorted(by_env[b], key=lambda r: (int(meta[r, 1]), r))
            dup += len(rows) - 1
            a = acc[b % LANES]
            for r in rows:
                v = float(stats[r, STAT_REWARD])
                a[0] += 1.0
                a[1] += v
                a[2] += v * v
                a[3], a[4] = nan_min(a[3], v), nan_max(a[4], v)
                a[5] += float(meta[r, 2])
                a[6] += stats[r, STAT_COVERAGE]
                a[7] += stats[r, STAT_COV_INTERESTED]
                a[8] += stats[r, STAT_MESSAGES]
        rec = self.slot(env_step)
        if rec is None:
            return
        self.counters[L.TLC_LOST_EPISODES] += max(int(cursor) - int(log_capacity), 0) + bad
        self.counters[L.TLC_DUPLICATE_ENV_ROWS] += dup
        total = [tree_sum(acc[:, f]) for f in range(9)]
        lo, hi = INF, -INF
        # (a tree of compares: for numbers the minimum / maximum whatever the order)
        for v in acc[:, 3]:
            lo = nan_min(lo, float(v))
        for v in acc[:, 4]:
            hi = nan_max(hi, float(v))
        rec[L.TL_EPISODES] += total[0]
        rec[L.TL_REW_SUM] += total[1]
        rec[L.TL_REW_SQ] += total[2]
        rec[L.TL_REW_MIN] = nan_min(rec[L.TL_REW_MIN], lo)
        rec[L.TL_REW_MAX] = nan_max(rec[L.TL_REW_MAX], hi)
        rec[L.TL_MOVES_SUM] += total[5]
        rec[L.TL_COVERAGE_SUM] += total[6]
        rec[L.TL_COV_INTERESTED_SUM] += total[7]
        rec[L.TL_MESSAGES_SUM] += total[8]
        rec[L.TL_ROUNDS] += 1.0
        rec[L.TL_ENV_STEP_LAST] = float(env_step)
        if eps is not None:
            rec[L.TL_EPS_LAST] = float(np.float32(eps))

    def update(self, env_step: int, loss, td, grads):
        rec = self.slot(env_step)
        if rec is None:
            return
        loss = float(np.float32(loss))
        asum, amax = td_stats(td)
        mean_abs = asum / float(len(np.asarray(td).reshape(-1)))
        sq = grad_sq_sum(grads)
        norm = float("nan") if math.isnan(sq) else math.sqrt(sq)
        rec[L.TL_UPDATES] += 1.0
        rec[L.TL_LOSS_SUM] += loss
        rec[L.TL_LOSS_MAX] = nan_max(rec[L.TL_LOSS_MAX], loss)
        rec[L.TL_LOSS_LAST] = loss
        rec[L.TL_TD_ABS_SUM] += mean_abs
        rec[L.TL_TD_ABS_MEAN_MAX] = nan_max(rec[L.TL_TD_ABS_MEAN_MAX], mean_abs)
        rec[L.TL_TD_ABS_MAX] = nan_max(rec[L.TL_TD_ABS_MAX], amax)
        rec[L.TL_GRAD_NORM_SUM] += norm
        rec[L.TL_GRAD_NORM_MAX] = nan_max(rec[L.TL_GRAD_NORM_MAX], norm)
        rec[L.TL_GRAD_NORM_LAST] = norm
        rec[L.TL_ENV_STEP_LAST] = float(env_step)
