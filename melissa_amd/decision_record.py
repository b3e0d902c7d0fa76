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
from .record_common import TraceRecorder, check_out_args, group_by_ordinal, save_traces

FIELDS = ("decisions", "relays", "gap", "gap_sq", "chosen_q", "max_q", "non_greedy", "first_decisions")


def check_decision_args(spread: bool, decisions_out=None, decision_trace_out=None, trace_envs: int = 1) -> None:
    """ValueError for decision-recorder arguments that mean nothing (no torch, nothing built)."""
    check_out_args("decision recorder", spread, dict(decisions_out=decisions_out, decision_trace_out=decision_trace_out),
                   decision_trace_out is not None, trace_envs)


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
    return group_by_ordinal(records, scalars={}, series=dict(decisions=4, relays=5), arrays=("sets", "q"))


save_decision_traces = save_traces       # keyed as :func:`melissa_amd.round_record.save_traces` keys the node traces


class DecisionRecorder(TraceRecorder):
    """Owner of one ``mel_decision_record`` and its device buffers for the envs of ``venv``.  ``max_rounds``: round indices kept
    (default: the env's ``max_moves + 1``); ``n_degrees``: degree rows, the last one also takes every larger degree (default:
    ``min(N, 64)``); ``trace_envs``: up to 16 env ids whose decisions are kept per round, in a ring of ``trace_capacity`` records
    each; ``quota``: per env, how many of its episodes count (None: all).  Give it to :class:`melissa_amd.collect.RoundLoop`
    (``decisions=``) BEFORE the loop captures its rounds: captured launches hold the pointers and the sizes."""

    group = staticmethod(group_decision_episodes)

    @staticmethod
    def trace_spec(n: int, W: int) -> dict:
        return dict(sets=((2, W), "int64"), q=((n, 2), "float32"))

    launches = 0             # calls of :meth:`launch`, over every instance (tests: a loop without a recorder makes none)

    def __init__(self, venv, max_rounds: "int | None" = None, n_degrees: "int | None" = None, trace_envs=(),
                 trace_capacity: int = 64, quota=None, device=None):
        import torch
        D = min(int(venv.n), 64) if n_degrees is None else int(n_degrees)
        if not 1 <= D <= _lib.DR_MAX_DEGREES:
            raise ValueError(f"DecisionRecorder: n_degrees={D} outside [1, {_lib.DR_MAX_DEGREES}]")
        B, n, R, dev = self._setup(venv, max_rounds, trace_envs, trace_capacity, device)
        self.n_degrees = D
        f64, i64 = torch.float64, torch.int64
        self.by_round = torch.zeros(B, R, _lib.DR_FIELDS, dtype=f64, device=dev)
        self.by_degree = torch.zeros(B, D, _lib.DR_FIELDS, dtype=f64, device=dev)
        self.overflow = torch.zeros(B, dtype=i64, device=dev)
        self.skipped = torch.zeros(B, dtype=i64, device=dev)
        self._out_round = torch.zeros(R, _lib.DR_FIELDS, dtype=f64, device=dev)
        self._out_degree = torch.zeros(D, _lib.DR_FIELDS, dtype=f64, device=dev)
        self._counters = torch.zeros(4, dtype=i64, device=dev)
        self.c = c = _lib.MelDecisionRecord()
        c.by_round, c.by_degree = self.by_round.data_ptr(), self.by_degree.data_ptr()
        c.overflow, c.skipped = self.overflow.data_ptr(), self.skipped.data_ptr()
        c.n_degrees = D
        self._bind_ring(quota)

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
    def reset(self) -> None:
        """Zero the tables and the counters, forget every trace record."""
        for t in (self.by_round, self.by_degree, self.overflow, self.skipped):
            t.zero_()
        self._reset_ring()

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
