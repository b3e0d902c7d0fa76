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

FIELDS = ("count", "has_message", "interested_with_message", "interested", "messages", "active_agents",
          "coverage_interested_fraction", "newly_covered")
QUANTILES = (0.5, 0.9, 1.0)


def check_record_args(spread: bool, curves_out=None, trace_out=None, render_out=None, trace_envs: int = 1) -> None:
    """ValueError for recorder arguments that mean nothing (no torch, nothing built)."""
    wanted = [n for n, v in (("curves_out", curves_out), ("trace_out", trace_out), ("render_out", render_out)) if v is not None]
    if wanted and not spread:
        raise ValueError(f"{', '.join(wanted)}: the per-round recorder runs with the spread evaluation (spread=True / --spread; "
                         f"with one env that is the reference's own walk down the test list)")
    if (trace_out is not None or render_out is not None) and not 1 <= int(trace_envs) <= _lib.RR_MAX_TRACE:
        raise ValueError(f"trace_envs={trace_envs} outside [1, {_lib.RR_MAX_TRACE}]")


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
    episodes, run = [], []

    def close():
        if run:
            m = np.stack([r["meta"] for r in run])
            episodes.append(dict(env=int(m[0, 0]), ordinal=int(m[0, 1]), pool_episode=int(m[0, 2]), origin=int(m[0, 4]),
                                 rounds=m[:, 3].copy(), world_msgs=m[:, 5].copy(),
                                 **{k: np.stack([r[k] for r in run]) for k in ("pos", "one_hop", "sets", "agent_msgs", "received")}))
            run.clear()

    for rec in records:
        if run and int(rec["meta"][1]) != int(run[0]["meta"][1]):
            close()
        run.append(rec)
    close()
    return episodes


def save_traces(path, traces: dict) -> None:
    """``{env: [episode, ...]}`` (:meth:`RoundRecorder.drain_traces`) as one ``.npz``: key ``e<env>_o<ordinal>_<array>``."""
    flat = {}
    for env, episodes in traces.items():
        for ep in episodes:
            for k, v in ep.items():
                flat[f"e{int(env)}_o{ep['ordinal']}_{k}"] = np.asarray(v)
    with open(path, "wb") as f:
        np.savez(f, **flat)


class RoundRecorder:
    """Owner of one ``mel_round_record`` and its device buffers for the envs of ``venv``.  ``max_rounds``: round indices kept
    (default: the env's ``max_moves + 1``); ``trace_envs``: up to 16 env ids whose per-node state is kept after every round, in
    a ring of ``trace_capacity`` records each; ``quota``: per env, how many of its episodes count (None: all).  Give it to
    :class:`melissa_amd.collect.RoundLoop` (``recorder=``) BEFORE the loop captures its rounds: captured launches hold the pointers
    and the sizes."""

    def __init__(self, venv, max_rounds: "int | None" = None, trace_envs=(), trace_capacity: int = 64, quota=None, device=None,
                 log_capacity: int = 65536):
        import torch
        if int(venv.env.log_capacity) < 1:
            venv.enable_episode_log(int(log_capacity))       # (a Collector built afterwards replaces it with its own)
        B, n = int(venv.env_num), int(venv.n)
        R = int(venv.max_moves) + 1 if max_rounds is None else int(max_rounds)
        trace_envs = [int(t) for t in trace_envs]
        if not 1 <= R <= _lib.RR_MAX_ROUNDS:
            raise ValueError(f"RoundRecorder: max_rounds={R} outside [1, {_lib.RR_MAX_ROUNDS}]")
        if len(trace_envs) > _lib.RR_MAX_TRACE or len(set(trace_envs)) != len(trace_envs) or any(not 0 <= t < B for t in trace_envs):
            raise ValueError(f"RoundRecorder: trace_envs={trace_envs}: at most {_lib.RR_MAX_TRACE} distinct envs of [0, {B})")
        if trace_envs and int(trace_capacity) < 1:
            raise ValueError(f"RoundRecorder: trace_capacity={trace_capacity} must be >= 1")
        self.venv, self.max_rounds, self.trace_envs, self.trace_capacity = venv, R, trace_envs, int(trace_capacity)
        self.device = dev = torch.device(device) if device is not None else venv.device
        T, cap, W = len(trace_envs), int(trace_capacity), _lib.set_words(n)
        f64, i32, i64 = torch.float64, torch.int32, torch.int64
        self.running = torch.zeros(B, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.ended = torch.zeros(B, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.carry = torch.full((B, _lib.RR_CARRY), -1, dtype=i32, device=dev)
        self.last = torch.zeros(B, _lib.RR_FIELDS, dtype=f64, device=dev)
        self.overflow = torch.zeros(B, dtype=i64, device=dev)
        self.skipped = torch.zeros(B, dtype=i64, device=dev)
        self.unlogged = torch.zeros(B, dtype=i64, device=dev)
        self.quota = torch.zeros(B, dtype=i32, device=dev)
        self._out = torch.zeros(2, R, _lib.RR_FIELDS, dtype=f64, device=dev)
        self._counters = torch.zeros(4, dtype=i64, device=dev)
        self.c = c = _lib.MelRoundRecord()
        c.running, c.ended, c.seen, c.last = self.running.data_ptr(), self.ended.data_ptr(), self.carry.data_ptr(), self.last.data_ptr()
        c.overflow, c.skipped, c.unlogged = self.overflow.data_ptr(), self.skipped.data_ptr(), self.unlogged.data_ptr()
        c.n_envs, c.n_nodes, c.max_rounds, c.n_trace, c.trace_capacity = B, n, R, T, cap if T else 0
        if T:
            self.trace_cursor = torch.zeros(T, dtype=i64, device=dev)
            self.trace_meta = torch.zeros(T, cap, 8, dtype=i32, device=dev)
            self.trace_pos = torch.zeros(T, cap, n, 2, dtype=f64, device=dev)
            self.trace_one_hop = torch.zeros(T, cap, n, W, dtype=i64, device=dev)
            self.trace_sets = torch.zeros(T, cap, 6, W, dtype=i64, device=dev)
            self.trace_agent_msgs = torch.zeros(T, cap, n, dtype=i32, device=dev)
            self.trace_received = torch.zeros(T, cap, n, dtype=i32, device=dev)
            for name in ("trace_cursor", "trace_meta", "trace_pos", "trace_one_hop", "trace_sets", "trace_agent_msgs", "trace_received"):
                setattr(c, name, getattr(self, name).data_ptr())
            for k, t in enumerate(trace_envs):
                c.trace_env[k] = t
        self._drained = [0] * T
        self.records = {t: [] for t in trace_envs}           # every record drained since reset(), per traced env
        self.lost = 0                                        # records overwritten before they were read, since reset()
        self.set_quota(quota)

    # ------------------------------------------------------------------ launch (capturable: no host read, no allocation)
    def launch(self) -> None:
        """Behind a ``mel_env_round``: one sample per env whose state moved since the last launch."""
        _lib.check(_lib.load().mel_round_record_round(C.byref(self.c), C.byref(self.venv.env), _lib.current_stream_ptr(self.device)),
                   "mel_round_record_round")

    # ------------------------------------------------------------------ host side
    def set_quota(self, quota) -> None:
        """Per env, how many of its episodes count (samples of later ones are not taken); None: no limit.  The VALUES live on
        the device, but whether there is a quota at all is fixed into a captured launch: set it before the loop is built."""
        import torch
        if quota is None:
            self.c.quota = None
            return
        q = torch.as_tensor(np.asarray(quota, dtype=np.int32))
        if q.shape != (self.venv.env_num,):
            raise ValueError(f"RoundRecorder: quota has shape {tuple(q.shape)}, one value per env ({self.venv.env_num}) is needed")
        self.quota.copy_(q)
        self.c.quota = self.quota.data_ptr()

    def reset(self) -> None:
        """Zero the accumulators and the counters, forget the carry (``seen`` = -1) and every trace record."""
        for t in (self.running, self.ended, self.last, self.overflow, self.skipped, self.unlogged):
            t.zero_()
        self.carry.fill_(-1)
        if self.trace_envs:
            self.trace_cursor.zero_()
        self._drained = [0] * len(self.trace_envs)
        self.records = {t: [] for t in self.trace_envs}
        self.lost = 0

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

    def drain_traces(self):
        """Read the records written since the last drain (synchronises) -> (``{env: [episode, ...]}`` of EVERY record drained
        since :meth:`reset`, in play order and grouped by episode ordinal (:func:`group_episodes`), records overwritten before
        they were read since :meth:`reset`)."""
        import torch
        if self.trace_envs:
            torch.cuda.synchronize(self.device)
            cursors = self.trace_cursor.cpu().tolist()
            host = {k: getattr(self, "trace_" + k).cpu().numpy() for k in ("meta", "pos", "one_hop", "sets", "agent_msgs", "received")}
            host["one_hop"], host["sets"] = host["one_hop"].view(np.uint64), host["sets"].view(np.uint64)
            cap = self.trace_capacity
            for t, env in enumerate(self.trace_envs):
                cur, first = int(cursors[t]), self._drained[t]
                if cur - first > cap:
                    self.lost += cur - cap - first
                    first = cur - cap
                for j in range(first, cur):
                    self.records[env].append({k: v[t, j % cap].copy() for k, v in host.items()})
                self._drained[t] = cur
        return {env: group_episodes(recs) for env, recs in self.records.items()}, self.lost
