"""Per-round dissemination curves and node traces of an evaluation, recorded on the device (``mel_round_record``,
include/melissa_hip.h).

The reference lets a user SEE an evaluation: ``render_mode="human"`` draws the graph after every world step (graph.py:350-356,
``draw_graph`` :466-484).  Here the rounds replay from HIP graphs and nothing reads the device between them, so
:class:`RoundRecorder` owns the device buffers of one capturable launch that runs behind every ``mel_env_round`` and samples the
state the round left: per round index the sums behind the usual dissemination figures (coverage and messages against round,
delivery delay), and for a few chosen envs a ring of per-node records that can be drawn (:mod:`melissa_amd.render`).  The host
reads where the run synchronises anyway.  Opt-in: a loop without a recorder issues none of the launches.

The launch sees the state a round LEFT.  An episode whose last world step also ends it (the observation right after the step
raises ``explicit_reset``, graph.py:205-211) is reset inside that round's launch; its final figures are taken from the env
batch's episode log instead, so the recorder needs the log: it switches one on where the env batch has none, and it cannot
share a loop with a :class:`melissa_amd.train_log.TrainLog`, which empties the log every round.

:func:`summarise` is pure NumPy: it turns the two accumulators into per-round curves.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .record_common import TraceRecorder, check_out_args, group_by_ordinal, save_traces  # noqa: F401  (save_traces: this module's too)

FIELDS = ("count", "has_message", "interested_with_message", "interested", "messages", "active_agents",
          "coverage_interested_fraction", "newly_covered")
QUANTILES = (0.5, 0.9, 1.0)


def check_record_args(spread: bool, curves_out=None, trace_out=None, render_out=None, trace_envs: int = 1) -> None:
    """ValueError for recorder arguments that mean nothing (no torch, nothing built)."""
    check_out_args("per-round recorder", spread, dict(curves_out=curves_out, trace_out=trace_out, render_out=render_out),
                   trace_out is not None or render_out is not None, trace_envs)


def summarise(running, ended, n_nodes: "int | None" = None, quantiles=QUANTILES) -> dict:
    """The accumulators ``running`` / ``ended`` (float64 ``[R, 8]``, fields :data:`FIELDS`) of COMPLETE episodes as curves over the
    round index.  An episode that has ended keeps its final value: the carried-forward sum of field f at round r is
    ``running[r, f] + sum(ended[e, f] for e < r)``, divided by the episode count.

    -> dict: ``episodes`` (int: the samples at round 0), ``rounds`` [R], ``running`` [R] episodes still running at round r,
    ``carried_count`` [R] running plus ended-before (the episode count at every r when every episode is complete),
    ``coverage`` [R] mean share of nodes with the message (mean node COUNT without ``n_nodes``),
    ``coverage_interested_fraction`` [R], ``messages`` [R] mean messages transmitted so far, ``covered_share`` [R] cumulative
    share of episodes in which every interested node has the message, ``delay`` {q: first round at which ``covered_share >= q``,
    None where it never is}."""
    running, ended = np.asarray(running, dtype=np.float64), np.asarray(ended, dtype=np.float64)
    if running.ndim != 2 or running.shape[1] != _lib.RR_FIELDS or running.shape != ended.shape:
        raise ValueError(f"summarise: running {running.shape} and ended {ended.shape} must both be [R, {_lib.RR_FIELDS}]")
    R = running.shape[0]
    episodes = float(running[0, _lib.RR_COUNT])
    before = np.concatenate([np.zeros((1, _lib.RR_FIELDS)), np.cumsum(ended, axis=0)[:-1]])      # sum over e < r
    carried = running + before
    div = episodes if episodes > 0 else 1.0
    covered = np.cumsum(running[:, _lib.RR_NEWLY_COVERED]) / div
    delay = {}
    for q in quantiles:
        hit = np.flatnonzero(covered >= float(q)) if episodes > 0 else []
        delay[float(q)] = int(hit[0]) if len(hit) else None
    return dict(episodes=int(episodes), rounds=np.arange(R), running=running[:, _lib.RR_COUNT].copy(),
                carried_count=carried[:, _lib.RR_COUNT].copy(),
                coverage=carried[:, _lib.RR_HAS_MESSAGE] / div / (float(n_nodes) if n_nodes else 1.0),
                coverage_interested_fraction=carried[:, _lib.RR_COVERAGE_FRACTION] / div,
                messages=carried[:, _lib.RR_MESSAGES] / div, covered_share=covered, delay=delay)


def group_episodes(records: list) -> list:
    """Trace records of ONE env in play order -> one dict per episode ordinal: ``env``, ``ordinal``, ``pool_episode``, ``origin``,
    ``rounds`` [K], ``world_msgs`` [K], ``pos`` [K, N, 2], ``one_hop`` uint64 [K, N, W], ``sets`` uint64 [K, 6, W]
    (``_lib.RR_TRACE_SETS``), ``agent_msgs`` / ``received`` int32 [K, N]."""
    return group_by_ordinal(records, scalars=dict(origin=4), series=dict(world_msgs=5),
                            arrays=("pos", "one_hop", "sets", "agent_msgs", "received"))


class RoundRecorder(TraceRecorder):
    """Owner of one ``mel_round_record`` and its device buffers for the envs of ``venv``.  ``max_rounds``: round indices kept
    (default: the env's ``max_moves + 1``); ``trace_envs``: up to 16 env ids whose per-node state is kept after every round, in
    a ring of ``trace_capacity`` records each; ``quota``: per env, how many of its episodes count (None: all).  Give it to
    :class:`melissa_amd.collect.RoundLoop` (``recorder=``) BEFORE the loop captures its rounds: captured launches hold the pointers
    and the sizes."""

    group = staticmethod(group_episodes)

    @staticmethod
    def trace_spec(n: int, W: int) -> dict:
        return dict(pos=((n, 2), "float64"), one_hop=((n, W), "int64"), sets=((6, W), "int64"), agent_msgs=((n,), "int32"),
                    received=((n,), "int32"))

    def __init__(self, venv, max_rounds: "int | None" = None, trace_envs=(), trace_capacity: int = 64, quota=None, device=None,
                 log_capacity: int = 65536):
        import torch
        if int(venv.env.log_capacity) < 1:
            venv.enable_episode_log(int(log_capacity))       # (a Collector built afterwards replaces it with its own)
        B, n, R, dev = self._setup(venv, max_rounds, trace_envs, trace_capacity, device)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        self.running = torch.zeros(B, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.ended = torch.zeros(B, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.carry = torch.full((B, _lib.RR_CARRY), -1, dtype=i32, device=dev)
        self.last = torch.zeros(B, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.overflow = torch.zeros(B, dtype=i64, device=dev)
        self.skipped = torch.zeros(B, dtype=i64, device=dev)
        self.unlogged = torch.zeros(B, dtype=i64, device=dev)
        self._out = torch.zeros(2, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self._counters = torch.zeros(4, dtype=i64, device=dev)
        self.c = c = _lib.MelRoundRecord()
        c.running, c.ended, c.seen, c.last = self.running.data_ptr(), self.ended.data_ptr(), self.carry.data_ptr(), self.last.data_ptr()
        c.overflow, c.skipped, c.unlogged = self.overflow.data_ptr(), self.skipped.data_ptr(), self.unlogged.data_ptr()
        self._bind_ring(quota)

    # ------------------------------------------------------------------ launch (capturable: no host read, no allocation)
    def launch(self) -> None:
        """Behind a ``mel_env_round``: one sample per env whose state moved since the last launch."""
        _lib.check(_lib.load().mel_round_record_round(C.byref(self.c), C.byref(self.venv.env), _lib.current_stream_ptr(self.device)),
                   "mel_round_record_round")

    # ------------------------------------------------------------------ host side
    def reset(self) -> None:
        """Zero the accumulators and the counters, forget the carry (``seen`` = -1) and every trace record."""
        for t in (self.running, self.ended, self.last, self.overflow, self.skipped, self.unlogged):
            t.zero_()
        self.carry.fill_(-1)
        self._reset_ring()

    @property
    def seen(self):
        """int32 [B, 2] (device): (episodes_done, num_moves) of the state each env sampled last, -1 before the first."""
        return self.carry[:, :2]

    def curves(self):
        """-> (running float64 [R, 8], ended float64 [R, 8], {"overflow": int, "skipped": int, "unlogged": int}): the envs' rows
        added on the device in ascending env order; the counters are 0 in a clean run (rows past ``max_rounds``, launches that
        found an env in error, ended episodes missing from a full episode log).  Synchronises."""
        import torch
        _lib.check(_lib.load().mel_round_record_read(C.byref(self.c), self._out[0].data_ptr(), self._out[1].data_ptr(),
                                                     self._counters.data_ptr(), _lib.current_stream_ptr(self.device)),
                   "mel_round_record_read")
        torch.cuda.synchronize(self.device)
        out, counters = self._out.cpu().numpy(), self._counters.cpu().tolist()
        return out[0], out[1], dict(overflow=int(counters[_lib.RRC_OVERFLOW]), skipped=int(counters[_lib.RRC_SKIPPED]),
                                    unlogged=int(counters[_lib.RRC_UNLOGGED]))
