"""NumPy model of ``mel_round_record_round`` (include/melissa_hip.h): the sampling rules restated on plain arrays, one
``launch(state)`` per device launch.  ``state``: dict of the env batch's arrays as the launch finds them -

    scalars int32 [B, 16], node_sets uint64 [B, 8, W], sel_sets uint64 [B, 4, W], pos float64 [B, N, 2],
    one_hop uint64 [B, N, W], agent_msgs int32 [B, N], received int32 [B, N]
    and, optional (absent: an empty log), the env batch's episode log: log_cursor int, log_capacity int,
    log_stats float64 [rows, 10], log_meta int32 [rows, 3]

The model keeps what the device keeps (``running``, ``ended``, ``carry``, ``last``, ``overflow``, ``skipped``, the trace rings and
cursors, ``unlogged``) and, beside the rings, every trace record ever written (``all_records``: nothing is overwritten there).
"""
import numpy as np

S_ORIGIN, S_NUM_MOVES, S_WORLD_MSGS, S_EPISODE, S_EPISODES_DONE, S_ERROR = 0, 3, 4, 6, 10, 11
SET_HAS_MESSAGE, SET_ORIGIN, SET_INTERESTED, SET_SCRIPTED = 0, 1, 2, 3
SEL_ACTIVE, SEL_TAKEN_ACTION = 0, 3
FIELDS = 8


def popcount(words) -> int:
    return sum(bin(int(w)).count("1") for w in np.asarray(words, dtype=np.uint64).reshape(-1))


def pack_set(flags) -> np.ndarray:
    """bool [N] -> uint64 [W] node set."""
    flags = np.asarray(flags, dtype=bool)
    out = np.zeros((len(flags) + 63) // 64, dtype=np.uint64)
    for i in np.flatnonzero(flags):
        out[i // 64] |= np.uint64(1) << np.uint64(i % 64)
    return out


class RoundRecordModel:
    def __init__(self, n_envs, n_nodes, max_rounds, trace_envs=(), trace_capacity=64, quota=None):
        self.B, self.n, self.R, self.W = int(n_envs), int(n_nodes), int(max_rounds), (int(n_nodes) + 63) // 64
        self.trace_envs, self.cap = [int(t) for t in trace_envs], int(trace_capacity)
        self.quota = None if quota is None else np.asarray(quota, dtype=np.int64)
        self.reset()

    def reset(self):
        B, R, n, W, T, cap = self.B, self.R, self.n, self.W, len(self.trace_envs), self.cap
        self.running, self.ended = np.zeros((B, R, FIELDS)), np.zeros((B, R, FIELDS))
        self.carry = np.full((B, 6), -1, dtype=np.int32)
        self.last = np.zeros((B, FIELDS))
        self.overflow, self.skipped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        self.unlogged = np.zeros(B, dtype=np.int64)
        self.cursor = np.zeros(T, dtype=np.int64)
        self.ring = dict(meta=np.zeros((T, cap, 8), dtype=np.int32), pos=np.zeros((T, cap, n, 2)),
                         one_hop=np.zeros((T, cap, n, W), dtype=np.uint64), sets=np.zeros((T, cap, 6, W), dtype=np.uint64),
                         agent_msgs=np.zeros((T, cap, n), dtype=np.int32), received=np.zeros((T, cap, n), dtype=np.int32))
        self.all_records = {t: [] for t in self.trace_envs}

    @property
    def seen(self):
        return self.carry[:, :2]

    def launch(self, state):
        for b in range(self.B):
            self._env(b, state)

    def _env(self, b, st):
        sc = st["scalars"][b]
        ep, mv = int(sc[S_EPISODES_DONE]), int(sc[S_NUM_MOVES])
        seen_ep, seen_mv, last_r, last_full, log_seen, _reserved = (int(x) for x in self.carry[b])
        if (ep, mv) == (seen_ep, seen_mv):
            return
        if int(sc[S_ERROR]) != 0:
            self.skipped[b] += 1
            return
        log_total, log_cap = int(st.get("log_cursor", 0)), int(st.get("log_capacity", 0))
        log_to = max(0, min(log_total, log_cap))
        log_from = 0 if (log_seen < 0 or log_seen > log_to) else log_seen
        if ep != seen_ep:
            if last_r >= 0:
                row = -1
                if log_total <= log_cap:
                    mine = [k for k in range(log_from, log_to) if int(st["log_meta"][k][0]) == b]
                    row = mine[-1] if mine else -1
                final_r = int(st["log_meta"][row][2]) if row >= 0 else last_r
                if row < 0:
                    self.unlogged[b] += 1
                end_v = self.last[b].copy()
                if row >= 0:                             # the row: the logger_stats of the episode's final observation
                    s = np.asarray(st["log_stats"][row], dtype=np.float64)
                    full = int(s[5] > 0.0 and s[7] == s[5])
                    v = np.array([1.0, float(int(s[1] * float(self.n) + 0.5)), s[7], s[5], s[0], 0.0, s[6],
                                  1.0 if (full and not last_full) else 0.0])
                    if final_r != last_r:                # the last world step ran in the launch that ended the episode
                        if 0 <= final_r < self.R:
                            self.running[b, final_r] += v
                        else:
                            self.overflow[b] += 1
                        last_r, end_v = final_r, v
                    else:
                        end_v[[1, 2, 3, 4, 6]] = v[[1, 2, 3, 4, 6]]
                if 0 <= last_r < self.R:
                    self.ended[b, last_r] += end_v
                else:
                    self.overflow[b] += 1
            last_r, last_full = -1, 0
        if self.quota is None or ep < int(self.quota[b]):
            ns, ss = np.asarray(st["node_sets"][b], dtype=np.uint64).reshape(8, -1), np.asarray(st["sel_sets"][b], dtype=np.uint64).reshape(4, -1)
            has, interested = ns[SET_HAS_MESSAGE], ns[SET_INTERESTED]
            n_int, cov_int = popcount(interested), popcount(has & interested)
            frac = float(cov_int) / float(n_int) if n_int > 0 else 0.0
            full = int(n_int > 0 and cov_int == n_int)
            v = np.array([1.0, popcount(has), cov_int, n_int, int(sc[S_WORLD_MSGS]), popcount(ss[SEL_ACTIVE]), frac,
                          1.0 if (full and not last_full) else 0.0])
            if mv < self.R:
                self.running[b, mv] += v
            else:
                self.overflow[b] += 1
            self.last[b] = v
            last_r, last_full = mv, full
            if b in self.trace_envs:
                t = self.trace_envs.index(b)
                rec = dict(meta=np.array([b, ep, int(sc[S_EPISODE]), mv, int(sc[S_ORIGIN]), int(sc[S_WORLD_MSGS]), 0, 0], dtype=np.int32),
                           pos=np.array(st["pos"][b], dtype=np.float64).reshape(self.n, 2),
                           one_hop=np.array(st["one_hop"][b], dtype=np.uint64).reshape(self.n, self.W),
                           sets=np.stack([ns[SET_HAS_MESSAGE], ns[SET_ORIGIN], ns[SET_INTERESTED], ns[SET_SCRIPTED],
                                          ss[SEL_ACTIVE], ss[SEL_TAKEN_ACTION]]),
                           agent_msgs=np.array(st["agent_msgs"][b], dtype=np.int32), received=np.array(st["received"][b], dtype=np.int32))
                slot = int(self.cursor[t] % self.cap)
                for k, v_ in rec.items():
                    self.ring[k][t, slot] = v_
                self.cursor[t] += 1
                self.all_records[b].append(rec)
        self.carry[b] = (ep, mv, last_r, last_full, log_to, -1)

    def folded(self):
        """running / ended added over the envs in ascending order (what mel_round_record_read returns), and the counters."""
        run, end = np.zeros((self.R, FIELDS)), np.zeros((self.R, FIELDS))
        for b in range(self.B):
            run, end = run + self.running[b], end + self.ended[b]
        return run, end, dict(overflow=int(self.overflow.sum()), skipped=int(self.skipped.sum()), unlogged=int(self.unlogged.sum()))


def state_of(venv) -> dict:
    """The arrays a launch reads, copied from a ``HipGraphVectorEnv`` (synchronises)."""
    import torch
    B, n, W = venv.env_num, venv.n, (venv.n + 63) // 64
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    return dict(scalars=venv.scalars().cpu().numpy(), node_sets=u64(venv.node_sets()).reshape(B, 8, W),
                sel_sets=u64(venv._field(venv.env.sel_sets, 4 * W, torch.int64)).reshape(B, 4, W),
                pos=venv.positions().cpu().numpy(), one_hop=u64(venv.one_hop()).reshape(B, n, W),
                agent_msgs=venv._field(venv.env.agent_msgs, n, torch.int32).cpu().numpy(),
                received=venv._field(venv.env.received, n, torch.int32).cpu().numpy(),
                log_cursor=int(venv.log_cursor.item()), log_capacity=int(venv.env.log_capacity),
                log_stats=venv.log_stats.cpu().numpy(), log_meta=venv.log_meta.cpu().numpy())
