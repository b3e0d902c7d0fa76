"""The host half of what :class:`melissa_amd.round_record.RoundRecorder` and :class:`melissa_amd.decision_record.DecisionRecorder`
share (the device half is csrc/record_common.hpp): the per-env quota and the trace sink - for each of up to 16 listed envs a
ring of ``trace_capacity`` records, an eight-int header ``trace_meta`` (env, episode ordinal, pool episode, num_moves, two ints of
the recorder's own, 0, 0) plus the recorder's payload arrays, written by the device behind a cursor that only grows and drained
here where the run synchronises anyway.  A recorder names its payload in ``trace_spec``; everything else about the ring is here.
"""
from __future__ import annotations

import itertools

import numpy as np

from . import _lib


def check_out_args(what: str, spread: bool, outs: dict, traced: bool, trace_envs: int) -> None:
    """ValueError for output arguments ``{name: value}`` of the recorder ``what`` that mean nothing; ``traced``: one of them
    asks for trace records."""
    wanted = [n for n, v in outs.items() if v is not None]
    if wanted and not spread:
        raise ValueError(f"{', '.join(wanted)}: the {what} runs with the spread evaluation (spread=True / --spread; "
                         f"with one env that is the reference's own walk down the test list)")
    if traced and not 1 <= int(trace_envs) <= _lib.RR_MAX_TRACE:
        raise ValueError(f"trace_envs={trace_envs} outside [1, {_lib.RR_MAX_TRACE}]")


def check_rides(who: str, name: str, rec, venv, chunk: "int | None" = None) -> None:
    """ValueError unless the recorder ``rec`` (argument ``name`` of ``who``; None passes) was built on ``venv`` and, where
    ``chunk`` rounds are played between two drains, its rings hold twice as many records."""
    if rec is None:
        return
    if rec.venv is not venv:
        raise ValueError(f"{who}: {name} was built on another env batch")
    if chunk is not None and rec.trace_envs and rec.trace_capacity < 2 * int(chunk):
        raise ValueError(f"{who}: trace_capacity={rec.trace_capacity} is below twice the {int(chunk)} rounds "
                         f"played between two drains of the traces")


def drain_ring(cursors, host: dict, drained, capacity: int):
    """The records written since the last drain, by arithmetic alone.  ``cursors[t]``: records ever written to slot t's ring;
    ``host``: ``{name: array [T, capacity, ...]}`` as read with the cursors; ``drained[t]``: the cursor at the last drain.
    Record j lies in ring slot ``j % capacity``, so of more than ``capacity`` new records the oldest were overwritten.
    -> (per slot the new records in play order, each ``{name: copy of its row}``; the new ``drained``; records lost)."""
    out, lost = [], 0
    for t, (cur, first) in enumerate(zip(cursors, drained)):
        if cur - first > capacity:
            lost += cur - capacity - first
            first = cur - capacity
        out.append([{k: v[t, j % capacity].copy() for k, v in host.items()} for j in range(first, cur)])
    return out, [int(c) for c in cursors], lost


def group_by_ordinal(records: list, scalars: dict, series: dict, arrays: tuple) -> list:
    """Trace records of ONE env in play order -> one dict per run of equal episode ordinal: ``env``, ``ordinal``,
    ``pool_episode``, the header columns ``scalars`` ``{name: column}`` of its first record as ints, ``rounds`` [K] (num_moves),
    the header columns ``series`` as int32 [K], and every payload array of ``arrays`` stacked to [K, ...]."""
    episodes = []
    for _, run in itertools.groupby(records, key=lambda r: int(r["meta"][1])):
        run = list(run)
        m = np.stack([r["meta"] for r in run])
        episodes.append(dict(env=int(m[0, 0]), ordinal=int(m[0, 1]), pool_episode=int(m[0, 2]),
                             **{k: int(m[0, col]) for k, col in scalars.items()}, rounds=m[:, 3].copy(),
                             **{k: m[:, col].copy() for k, col in series.items()},
                             **{k: np.stack([r[k] for r in run]) for k in arrays}))
    return episodes


def save_traces(path, traces: dict) -> None:
    """``{env: [episode, ...]}`` (a recorder's ``drain_traces``) as one ``.npz``: key ``e<env>_o<ordinal>_<array>``."""
    flat = {}
    for env, episodes in traces.items():
        for ep in episodes:
            for k, v in ep.items():
                flat[f"e{int(env)}_o{ep['ordinal']}_{k}"] = np.asarray(v)
    with open(path, "wb") as f:
        np.savez(f, **flat)


class TraceRecorder:
    """Base of the two recorders: ``venv``, ``max_rounds``, ``device``, the quota and the trace sink.  A subclass gives
    ``trace_spec(n, W)`` -> ``{payload array: (tail shape, dtype name)}`` (an int64 payload holds node sets: it is drained as
    uint64) and ``group`` (its ``group_*episodes``), calls :meth:`_setup` first, builds ``self.c`` and its own buffers, then
    :meth:`_bind_ring`.  Every buffer is a plain attribute, looked up whenever it is used."""

    def _setup(self, venv, max_rounds, trace_envs, trace_capacity, device):
        """Validate and keep the common arguments -> (B, n, R, device)."""
        import torch
        who, B = type(self).__name__, int(venv.env_num)
        R = int(venv.max_moves) + 1 if max_rounds is None else int(max_rounds)
        trace_envs = [int(t) for t in trace_envs]
        if not 1 <= R <= _lib.RR_MAX_ROUNDS:
            raise ValueError(f"{who}: max_rounds={R} outside [1, {_lib.RR_MAX_ROUNDS}]")
        if len(trace_envs) > _lib.RR_MAX_TRACE or len(set(trace_envs)) != len(trace_envs) or any(not 0 <= t < B for t in trace_envs):
            raise ValueError(f"{who}: trace_envs={trace_envs}: at most {_lib.RR_MAX_TRACE} distinct envs of [0, {B})")
        if trace_envs and int(trace_capacity) < 1:
            raise ValueError(f"{who}: trace_capacity={trace_capacity} must be >= 1")
        self.venv, self.max_rounds, self.trace_envs, self.trace_capacity = venv, R, trace_envs, int(trace_capacity)
        self.device = torch.device(device) if device is not None else venv.device
        return B, int(venv.n), R, self.device

    def _bind_ring(self, quota) -> None:
        """Allocate the quota and the rings and bind them, with the sizes, into ``self.c``."""
        import torch
        c, B, n, T, cap = self.c, int(self.venv.env_num), int(self.venv.n), len(self.trace_envs), self.trace_capacity
        c.n_envs, c.n_nodes, c.max_rounds, c.n_trace, c.trace_capacity = B, n, self.max_rounds, T, cap if T else 0
        self.quota = torch.zeros(B, dtype=torch.int32, device=self.device)
        if T:
            spec = dict(cursor=(None, "int64"), meta=((8,), "int32"), **self._payload_spec())
            for k, (tail, dtype) in spec.items():
                t = torch.zeros((T,) if tail is None else (T, cap, *tail), dtype=getattr(torch, dtype), device=self.device)
                setattr(self, "trace_" + k, t)
                setattr(c, "trace_" + k, t.data_ptr())
            for k, t in enumerate(self.trace_envs):
                c.trace_env[k] = t
        self._reset_ring()
        self.set_quota(quota)

    def set_quota(self, quota) -> None:
        """Per env, how many of its episodes count (nothing is recorded of later ones); None: no limit.  The VALUES live on the
        device, but whether there is a quota at all is fixed into a captured launch: set it before the loop is built."""
        import torch
        if quota is None:
            self.c.quota = None
            return
        q = torch.as_tensor(np.asarray(quota, dtype=np.int32))
        if q.shape != (self.venv.env_num,):
            raise ValueError(f"{type(self).__name__}: quota has shape {tuple(q.shape)}, one value per env ({self.venv.env_num}) is needed")
        self.quota.copy_(q)
        self.c.quota = self.quota.data_ptr()

    def _payload_spec(self) -> dict:
        return self.trace_spec(int(self.venv.n), _lib.set_words(int(self.venv.n)))

    def _reset_ring(self) -> None:
        """Forget every trace record, on the device (the cursors) and here."""
        if self.trace_envs:
            self.trace_cursor.zero_()
        self._drained = [0] * len(self.trace_envs)
        self.records = {t: [] for t in self.trace_envs}      # every record drained since reset(), per traced env
        self.lost = 0                                        # records overwritten before they were read, since reset()

    def drain_traces(self):
        """Read the records written since the last drain (synchronises) -> (``{env: [episode, ...]}`` of EVERY record drained
        since ``reset``, in play order and grouped by episode ordinal (the recorder's ``group``), records overwritten before
        they were read since ``reset``)."""
        import torch
        if self.trace_envs:
            torch.cuda.synchronize(self.device)
            cursors = self.trace_cursor.cpu().tolist()
            host = {k: getattr(self, "trace_" + k).cpu().numpy() for k in ("meta", *self._payload_spec())}
            host = {k: v.view(np.uint64) if v.dtype == np.int64 else v for k, v in host.items()}
            new, self._drained, lost = drain_ring(cursors, host, self._drained, self.trace_capacity)
            self.lost += lost
            for env, records in zip(self.trace_envs, new):
                self.records[env].extend(records)
        return {env: type(self).group(recs) for env, recs in self.records.items()}, self.lost
