"""The policy's decisions per round, recorded on the device (``mel_decision_record``, include/melissa_hip.h).

``watch --curves-out`` tells how coverage and messages grow with the round, ``--trace-out`` what every node's state was; neither
tells which nodes the policy let relay, how sure it was, or how that depends on the round and on the node's degree - the
forwarding ratio per hop and per neighbourhood size, which is also what tells a learned policy from ``simple_broadcast`` or
``mpr`` when their coverage curves look alike.  The data exists between two launches only: the forward writes the round's
logits and actions, ``mel_env_round`` consumes the actions and overwrites ``live``.  :class:`DecisionRecorder` owns the device
buffers of one capturable launch that sits between the two (:class:`melissa_amd.collect.RoundLoop`, ``decisions=``) and books
every decision of the policy by round index and by the deciding node's degree, and for a few chosen envs a ring of per-round
records (who decided, who relayed, with which Q values) that join the round recorder's node traces on
(env, episode ordinal, num_moves).  Opt-in: a loop without it issues no such launch.  It does not touch the episode log, so it
rides with or without a :class:`melissa_amd.round_record.RoundRecorder` or a :class:`melissa_amd.train_log.TrainLog`.

:func:`summarise_decisions` is pure NumPy: it turns the two tables into rates and means.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

FIELDS = ("decisions", "relays", "gap", "gap_sq", "chosen_q", "max_q", "non_greedy", "first_decisions")


def check_decision_args(spread: bool, decisions_out=None, decision_trace_out=None, trace_envs: int = 1) -> None:
    """ValueError for decision-recorder arguments that mean nothing (no torch, nothing built)."""
    wanted = [n for n, v in (("decisions_out", decisions_out), ("decision_trace_out", decision_trace_out)) if v is not None]
    if wanted and not spread:
        raise ValueError(f"{', '.join(wanted)}: the decision recorder runs with the spread evaluation (spread=True / --spread; "
                         f"with one env that is the reference's own walk down the test list)")
    if decision_trace_out is not None and not 1 <= int(trace_envs) <= _lib.DR_MAX_TRACE:
        raise ValueError(f"trace_envs={trace_envs} outside [1, {_lib.DR_MAX_TRACE}]")


def _figures(t: np.ndarray) -> dict:
    """Rows of sums [..., 8] -> the figures of every row; every ratio is NaN where the row holds no decision."""
    cnt = t[..., _lib.DR_DECISIONS]
    with np.errstate(divide="ignore", invalid="ignore"):
        per = lambda f: np.where(cnt > 0, t[..., f] / cnt, np.nan)
        mean_gap = per(_lib.DR_GAP)
        var = per(_lib.DR_GAP_SQ) - mean_gap * mean_gap
        return dict(decisions=cnt.copy(), relay_rate=per(_lib.DR_RELAYS), gap_mean=mean_gap,
                    gap_std=np.sqrt(np.where(var > 0, var, np.where(cnt > 0, 0.0, np.nan))), chosen_q_mean=per(_lib.DR_CHOSEN_Q),
                    max_q_mean=per(_lib.DR_MAX_Q), non_greedy_share=per(_lib.DR_NON_GREEDY), first_decision_share=per(_lib.DR_FIRST))


def summarise_decisions(by_round, by_degree) -> dict:
    """The tables ``by_round`` float64 ``[R, 8]`` and ``by_degree`` float64 ``[D, 8]`` (fields :data:`FIELDS`) as figures.

    -> dict: ``rounds`` [R], ``degrees`` [D] (the last degree row also holds every larger degree), ``by_round`` / ``by_degree``:
    dicts of arrays over the rows - ``decisions``, ``relay_rate``, ``gap_mean`` and ``gap_std`` of q[1] - q[0] (population
    standard deviation), ``chosen_q_mean``, ``max_q_mean``, ``non_greedy_share``, ``first_decision_share``, every ratio NaN where
    no decision was taken - and ``total``: the same figures (floats) over all rows of ``by_degree``, which also holds the
    decisions of rounds past the round table."""
    by_round, by_degree = np.asarray(by_round, dtype=np.float64), np.asarray(by_degree, dtype=np.float64)
    for name, t in (("by_round", by_round), ("by_degree", by_degree)):
        if t.ndim != 2 or t.shape[1] != _lib.DR_FIELDS:
            raise ValueError(f"summarise_decisions: {name} {t.shape} must be [rows, {_lib.DR_FIELDS}]")
    return dict(rounds=np.arange(by_round.shape[0]), degrees=np.arange(by_degree.shape[0]), by_round=_figures(by_round),
                by_degree=_figures(by_degree), total={k: float(v) for k, v in _figures(by_degree.sum(axis=0)).items()})


def group_decision_episodes(records: list) -> list:
    """Decision records of ONE env in play order -> one dict per episode ordinal: ``env``, ``ordinal``, ``pool_episode``,
    ``rounds`` [K] (num_moves of the state the decisions were taken in), ``decisions`` / ``relays`` int32 [K], ``sets`` uint64
    [K, 2, W] (``_lib.DR_TRACE_SETS``), ``q`` float32 [K, N, 2] (0 for nodes that did not decide)."""
    episodes, run = [], []

    def close():
        if run:
            m = np.stack([r["meta"] for r in run])
            episodes.append(dict(env=int(m[0, 0]), ordinal=int(m[0, 1]), pool_episode=int(m[0, 2]), rounds=m[:, 3].copy(),
                                 decisions=m[:, 4].copy(), relays=m[:, 5].copy(),
                                 **{k: np.stack([r[k] for r in run]) for k in ("sets", "q")}))
            run.clear()

    for rec in records:
        if run and int(rec["meta"][1]) != int(run[0]["meta"][1]):
            close()
        run.append(rec)
    close()
    return episodes


def save_decision_traces(path, traces: dict) -> None:
    """``{env: [episode, ...]}`` (:meth:`DecisionRecorder.drain_traces`) as one ``.npz``: key ``e<env>_o<ordinal>_<array>``, as
    :func:`melissa_amd.round_record.save_traces` keys the node traces."""
    flat = {}
    for env, episodes in traces.items():
        for ep in episodes:
            for k, v in ep.items():
                flat[f"e{int(env)}_o{ep['ordinal']}_{k}"] = np.asarray(v)
    with open(path, "wb") as f:
        np.savez(f, **flat)


class DecisionRecorder:
    """Owner of one ``mel_decision_record`` and its device buffers for the envs of ``venv``.  ``max_rounds``: round indices kept
    (default: the env's ``max_moves + 1``); ``n_degrees``: degree rows, the last one also takes every larger degree (default:
    ``min(N, 64)``); ``trace_envs``: up to 16 env ids whose decisions are kept per round, in a ring of ``trace_capacity`` records
    each; ``quota``: per env, how many of its episodes count (None: all).  Give it to :class:`melissa_amd.collect.RoundLoop`
    (``decisions=``) BEFORE the loop captures its rounds: captured launches hold the pointers and the sizes."""

    launches = 0             # calls of :meth:`launch`, over every instance (tests: a loop without a recorder makes none)

    def __init__(self, venv, max_rounds: "int | None" = None, n_degrees: "int | None" = None, trace_envs=(),
                 trace_capacity: int = 64, quota=None, device=None):
        import torch
        B, n = int(venv.env_num), int(venv.n)
        R = int(venv.max_moves) + 1 if max_rounds is None else int(max_rounds)
        D = min(n, 64) if n_degrees is None else int(n_degrees)
        trace_envs = [int(t) for t in trace_envs]
        if not 1 <= R <= _lib.DR_MAX_ROUNDS:
            raise ValueError(f"DecisionRecorder: max_rounds={R} outside [1, {_lib.DR_MAX_ROUNDS}]")
        if not 1 <= D <= _lib.DR_MAX_DEGREES:
            raise ValueError(f"DecisionRecorder: n_degrees={D} outside [1, {_lib.DR_MAX_DEGREES}]")
        if len(trace_envs) > _lib.DR_MAX_TRACE or len(set(trace_envs)) != len(trace_envs) or any(not 0 <= t < B for t in trace_envs):
            raise ValueError(f"DecisionRecorder: trace_envs={trace_envs}: at most {_lib.DR_MAX_TRACE} distinct envs of [0, {B})")
        if trace_envs and int(trace_capacity) < 1:
            raise ValueError(f"DecisionRecorder: trace_capacity={trace_capacity} must be >= 1")
        self.venv, self.max_rounds, self.n_degrees = venv, R, D
        self.trace_envs, self.trace_capacity = trace_envs, int(trace_capacity)
        self.device = dev = torch.device(device) if device is not None else venv.device
        T, cap, W = len(trace_envs), int(trace_capacity), _lib.set_words(n)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        self.by_round = torch.zeros(B, R, _lib.DR_FIELDS, dtype=f64, device=dev)
        self.by_degree = torch.zeros(B, D, _lib.DR_FIELDS, dtype=f64, device=dev)
        self.overflow = torch.zeros(B, dtype=i64, device=dev)
        self.skipped = torch.zeros(B, dtype=i64, device=dev)
        self.quota = torch.zeros(B, dtype=i32, device=dev)
        self._out_round = torch.zeros(R, _lib.DR_FIELDS, dtype=f64, device=dev)
        self._out_degree = torch.zeros(D, _lib.DR_FIELDS, dtype=f64, device=dev)
        self._counters = torch.zeros(4, dtype=i64, device=dev)
        self.c = c = _lib.MelDecisionRecord()
        c.by_round, c.by_degree = self.by_round.data_ptr(), self.by_degree.data_ptr()
        c.overflow, c.skipped = self.overflow.data_ptr(), self.skipped.data_ptr()
        c.n_envs, c.n_nodes, c.max_rounds, c.n_degrees, c.n_trace, c.trace_capacity = B, n, R, D, T, cap if T else 0
        if T:
            self.trace_cursor = torch.zeros(T, dtype=i64, device=dev)
            self.trace_meta = torch.zeros(T, cap, 8, dtype=i32, device=dev)
            self.trace_sets = torch.zeros(T, cap, 2, W, dtype=i64, device=dev)
            self.trace_q = torch.zeros(T, cap, n, 2, dtype=torch.float32, device=dev)
            for name in ("trace_cursor", "trace_meta", "trace_sets", "trace_q"):
                setattr(c, name, getattr(self, name).data_ptr())
            for k, t in enumerate(trace_envs):
                c.trace_env[k] = t
        self._drained = [0] * T
        self.records = {t: [] for t in trace_envs}           # every record drained since reset(), per traced env
        self.lost = 0                                        # records overwritten before they were read, since reset()
        self.set_quota(quota)

    # ------------------------------------------------------------------ launch (capturable: no host read, no allocation)
    def launch(self, logits, act, row_offsets, live) -> None:
        """Between the round's forward and its ``mel_env_round``: ``logits`` fp32 [rows, 2] and ``act`` int32 as the forward
        wrote them, ``row_offsets`` int32 [B + 1] (None: one logits row per env and the dense [B, N] action layout), ``live``
        the round's active sets."""
        DecisionRecorder.launches += 1
        _lib.check(_lib.load().mel_decision_record_round(
            C.byref(self.c), C.byref(self.venv.env), logits.data_ptr(), act.data_ptr(),
            row_offsets.data_ptr() if row_offsets is not None else None, live.data_ptr(), int(logits.shape[-1]),
            _lib.current_stream_ptr(self.device)), "mel_decision_record_round")

    # ------------------------------------------------------------------ host side
    def set_quota(self, quota) -> None:
        """Per env, how many of its episodes count (decisions of later ones are not booked); None: no limit.  The VALUES live
        on the device, but whether there is a quota at all is fixed into a captured launch: set it before the loop is built."""
        import torch
        if quota is None:
            self.c.quota = None
            return
        q = torch.as_tensor(np.asarray(quota, dtype=np.int32))
        if q.shape != (self.venv.env_num,):
            raise ValueError(f"DecisionRecorder: quota has shape {tuple(q.shape)}, one value per env ({self.venv.env_num}) is needed")
        self.quota.copy_(q)
        self.c.quota = self.quota.data_ptr()

    def reset(self) -> None:
        """Zero the tables and the counters, forget every trace record."""
        for t in (self.by_round, self.by_degree, self.overflow, self.skipped):
            t.zero_()
        if self.trace_envs:
            self.trace_cursor.zero_()
        self._drained = [0] * len(self.trace_envs)
        self.records = {t: [] for t in self.trace_envs}
        self.lost = 0

    def tables(self):
        """-> (by_round float64 [R, 8], by_degree float64 [D, 8], {"overflow": int, "skipped": int}): the envs' rows added on the
        device in ascending env order; the counters are 0 in a clean run (decisions whose round index was past ``max_rounds``,
        launches that found an env in error).  Synchronises."""
        import torch
        _lib.check(_lib.load().mel_decision_record_read(C.byref(self.c), self._out_round.data_ptr(), self._out_degree.data_ptr(),
                                                        self._counters.data_ptr(), _lib.current_stream_ptr(self.device)),
                   "mel_decision_record_read")
        torch.cuda.synchronize(self.device)
        counters = self._counters.cpu().tolist()
        return (self._out_round.cpu().numpy(), self._out_degree.cpu().numpy(),
                dict(overflow=int(counters[_lib.DRC_OVERFLOW]), skipped=int(counters[_lib.DRC_SKIPPED])))

    def drain_traces(self):
        """Read the records written since the last drain (synchronises) -> (``{env: [episode, ...]}`` of EVERY record drained
        since :meth:`reset`, in play order and grouped by episode ordinal (:func:`group_decision_episodes`), records overwritten
        before they were read since :meth:`reset`)."""
        import torch
        if self.trace_envs:
            torch.cuda.synchronize(self.device)
            cursors = self.trace_cursor.cpu().tolist()
            host = {k: getattr(self, "trace_" + k).cpu().numpy() for k in ("meta", "sets", "q")}
            host["sets"] = host["sets"].view(np.uint64)
            cap = self.trace_capacity
            for t, env in enumerate(self.trace_envs):
                cur, first = int(cursors[t]), self._drained[t]
                if cur - first > cap:
                    self.lost += cur - cap - first
                    first = cur - cap
                for j in range(first, cur):
                    self.records[env].append({k: v[t, j % cap].copy() for k, v in host.items()})
                self._drained[t] = cur
        return {env: group_decision_episodes(recs) for env, recs in self.records.items()}, self.lost
