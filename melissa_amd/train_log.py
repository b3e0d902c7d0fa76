"""Training curves of an epoch-mode run, accumulated on the device (``mel_train_log``, include/melissa_hip.h).

The reference's ``train_agent`` wires a logger (l_dgn.py:203-213,237-238,260) and [3P] tianshou writes ``train/reward``,
``train/length``, ``train/episode``, ``train/eps``, ``update/loss`` and ``test/reward`` about every 1000 env steps.  Here rounds and
updates replay from HIP graphs and nothing in the loop reads the device, so the curve is summed per interval of env steps by two
capturable launches - :meth:`TrainLog.launch_round` behind every env round, :meth:`TrainLog.launch_update` in front of every Adam
step - into a ring of records on the device, and :meth:`TrainLog.drain` reads the ring where the run synchronises anyway (after an
epoch's evaluation).  Rows are plain dicts with tianshou's logger keys where one exists; :func:`append_rows` writes them as JSON
lines.  Opt-in: a run without a log issues none of the launches and allocates none of the buffers.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os

from . import _lib

COUNTER_NAMES = ("lost_records", "lost_episodes", "duplicate_env_rows")


def check_log_args(epoch=None, log_interval=None, log_file=None) -> None:
    """ValueError for log arguments that mean nothing (no torch, nothing built)."""
    if log_interval is None:
        if log_file is not None:
            raise ValueError("log_file names the file of the training log: it needs log_interval")
        return
    if epoch is None:
        raise ValueError("log_interval logs the training curve of an epoch-mode run: it needs epoch")
    if int(log_interval) < 1:
        raise ValueError(f"log_interval={log_interval} must be >= 1 env step")


def ring_capacity(step_per_epoch: int, interval: int, overshoot: int = 0) -> int:
    """Records the ring must hold between two drains: the intervals of one epoch, of the env steps the loop may run past its
    target (``overshoot``, a bound), and four to spare."""
    return -(-int(step_per_epoch) // int(interval)) + 4 + -(-max(0, int(overshoot)) // int(interval))


def default_log_file(logdir: str, model: str, model_name: str) -> str:
    return os.path.join(logdir, model, f"{model_name}_progress.jsonl")


def row_from_record(rec, k: int, base: int, interval: int) -> dict:
    """One record of the device's ring (``MEL_TRAIN_LOG_DOUBLES`` float64) as a row: ``env_step`` is the interval's nominal end;
    a key whose count is 0 is absent."""
    L = _lib
    row = {"env_step": int(base) + (int(k) + 1) * int(interval)}
    n = float(rec[L.TL_EPISODES])
    if n > 0:
        mean = float(rec[L.TL_REW_SUM]) / n
        row.update({"train/episode": int(n), "train/reward": mean,
                    "train/reward_std": math.sqrt(max(float(rec[L.TL_REW_SQ]) / n - mean * mean, 0.0)),
                    "train/reward_min": float(rec[L.TL_REW_MIN]), "train/reward_max": float(rec[L.TL_REW_MAX]),
                    "train/length": float(rec[L.TL_MOVES_SUM]) / n, "train/coverage": float(rec[L.TL_COVERAGE_SUM]) / n,
                    "train/coverage_interested": float(rec[L.TL_COV_INTERESTED_SUM]) / n,
                    "train/messages": float(rec[L.TL_MESSAGES_SUM]) / n})
    if float(rec[L.TL_ROUNDS]) > 0 and float(rec[L.TL_EPS_LAST]) >= 0.0:
        row["train/eps"] = float(rec[L.TL_EPS_LAST])
    u = float(rec[L.TL_UPDATES])
    if u > 0:
        row.update({"update/n": int(u), "update/loss": float(rec[L.TL_LOSS_SUM]) / u, "update/loss_max": float(rec[L.TL_LOSS_MAX]),
                    "update/loss_last": float(rec[L.TL_LOSS_LAST]), "update/td_abs": float(rec[L.TL_TD_ABS_SUM]) / u,
                    "update/td_abs_max": float(rec[L.TL_TD_ABS_MAX]), "update/grad_norm": float(rec[L.TL_GRAD_NORM_SUM]) / u,
                    "update/grad_norm_max": float(rec[L.TL_GRAD_NORM_MAX])})
    return row


def append_rows(path: str, rows) -> int:
    """Append ``rows`` to ``path``, one JSON object per line (a resumed run goes on in the file it finds); -> rows written."""
    rows = list(rows)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return len(rows)


class TrainLog:
    """Owner of one ``mel_train_log`` and its device buffers for the envs of ``venv``.  It switches the env batch's episode log
    on (at least a row per env: an env ends at most one episode per round and every round is followed by a drain of the log),
    so it must exist BEFORE the :class:`melissa_amd.collect.RoundLoop` that takes it (``enable_step_stats`` has the same rule:
    captured rounds hold the pointers).  ``interval``: env steps per record, ``capacity``: records in the ring
    (:func:`ring_capacity`), ``scale``: env steps per decision of this loop (the world size)."""

    def __init__(self, venv, interval: int, capacity: int, scale: int = 1, device=None):
        import torch
        if int(interval) < 1 or int(capacity) < 1 or int(scale) < 1:
            raise ValueError(f"TrainLog: interval={interval}, capacity={capacity} and scale={scale} must all be >= 1")
        self.venv, self.interval, self.capacity, self.scale = venv, int(interval), int(capacity), int(scale)
        self.device = dev = torch.device(device) if device is not None else venv.device
        venv.enable_episode_log(max(int(venv.env_num), 64))
        self.records = torch.zeros(self.capacity, _lib.TRAIN_LOG_DOUBLES, dtype=torch.float64, device=dev)
        self.interval_id = torch.full((self.capacity,), -1, dtype=torch.int64, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.base = torch.full((1,), -1, dtype=torch.int64, device=dev)          # (the bits of UINT64_MAX: not armed)
        self.drained_upto = torch.zeros(1, dtype=torch.int64, device=dev)
        self._scalars = venv.scalars()
        self.c = _lib.MelTrainLog()
        self.c.records, self.c.interval_id, self.c.counters = self.records.data_ptr(), self.interval_id.data_ptr(), self.counters.data_ptr()
        self.c.base, self.c.drained_upto = self.base.data_ptr(), self.drained_upto.data_ptr()
        self.c.decisions, self.c.stride = self._scalars.data_ptr() + 4 * _lib.S_DECISIONS, _lib.ENV_SCALARS
        self.c.interval, self.c.capacity, self.c.n_envs, self.c.scale = self.interval, self.capacity, int(venv.env_num), self.scale
        self._scratch = None
        self._seen = [0, 0, 0]                      # the counters as the last drain found them
        self._base = None

    # ------------------------------------------------------------------ launches (capturable: no host read, no allocation)
    def launch_round(self, eps_dev=None) -> None:
        """Behind a ``mel_env_round``: fold the episode log's rows into the open record and empty the log."""
        _lib.check(_lib.load().mel_train_log_round(C.byref(self.c), C.byref(self.venv.env),
                                                   eps_dev.data_ptr() if eps_dev is not None else None,
                                                   _lib.current_stream_ptr(self.device)), "mel_train_log_round")

    def grad_table(self, optim) -> "_lib.MelAdamTensors":
        """The gradients the optimizer is about to apply, as ``adam_step`` lists them."""
        grads = [p.grad for group in optim.param_groups for p in group["params"] if p.grad is not None]
        if not 1 <= len(grads) <= _lib.ADAM_MAX_TENSORS:
            raise ValueError(f"TrainLog: {len(grads)} gradient tensors, the update launch takes 1 .. {_lib.ADAM_MAX_TENSORS}")
        import torch
        t = _lib.MelAdamTensors()
        t.count = len(grads)
        for i, g in enumerate(grads):
            if g.dtype != torch.float32 or not g.is_contiguous() or g.is_sparse:
                raise ValueError("TrainLog: the update launch reads dense contiguous fp32 gradients")
            t.grad[i], t.numel[i] = g.data_ptr(), g.numel()
        return t

    def launch_update(self, loss, td, optim) -> None:
        """In front of the Adam step: loss [1], td [batch] (device fp32), the optimizer's gradients."""
        import torch
        t = self.grad_table(optim)
        lib = _lib.load()
        need = int(lib.mel_train_log_scratch_bytes(C.byref(t)))
        if self._scratch is None or self._scratch.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TrainLog: the update launch's scratch must exist before a capture (run a warm-up update)")
            self._scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
        if loss.dtype != torch.float32 or td.dtype != torch.float32 or not td.is_contiguous():
            raise ValueError("TrainLog: loss and td must be contiguous fp32 device tensors")
        _lib.check(lib.mel_train_log_update(C.byref(self.c), loss.data_ptr(), td.data_ptr(), int(td.numel()), C.byref(t),
                                            self._scratch.data_ptr(), self._scratch.numel(), _lib.current_stream_ptr(self.device)),
                   "mel_train_log_update")

    # ------------------------------------------------------------------ host side (synchronises)
    def arm(self, base: int) -> None:
        """Intervals count from env step ``base`` on; launches already captured follow (the value lives on the device)."""
        self._base = int(base)
        self.base.fill_(self._base)

    def read_counters(self) -> dict:
        c = self.counters.cpu().tolist()
        return dict(zip(COUNTER_NAMES, (int(x) for x in c[:3])))

    def drain(self, final: bool = False) -> list:
        """The rows of every interval completed since the last drain, in order (an interval nothing fell into is a row with
        ``env_step`` alone); ``final``: the open interval too.  Advances ``drained_upto``.  RuntimeError when a counter of the
        log moved: a record was overwritten before it was read, the env's episode log overflowed, or an env had two rows in it."""
        import torch
        torch.cuda.synchronize(self.device)
        counters = self.counters.cpu().tolist()[:3]
        if counters != self._seen:
            moved = {n: int(c) for n, c, s in zip(COUNTER_NAMES, counters, self._seen) if c != s}
            self._seen = [int(c) for c in counters]
            raise RuntimeError(f"the training log lost data since the last drain: {moved} (a larger ring / a longer interval; "
                               f"the episode log holds {int(self.venv.env.log_capacity)} rows per round)")
        if self._base is None:
            return []
        env_step = self.scale * int(self._scalars[:, _lib.S_DECISIONS].to(torch.int64).sum().item())
        if env_step < self._base:
            return []
        k_now = (env_step - self._base) // self.interval
        ids, recs = self.interval_id.cpu().tolist(), self.records.cpu().numpy()
        first, end = int(self.drained_upto.item()), k_now + (1 if final else 0)
        rows = []
        for k in range(first, end):
            slot = k % self.capacity
            if ids[slot] == k:
                row = row_from_record(recs[slot], k, self._base, self.interval)
            elif k == k_now:
                continue                           # the open interval, and nothing has fallen into it yet
            else:
                row = {"env_step": self._base + (k + 1) * self.interval}
            if k == k_now:
                row["partial"] = True
            rows.append(row)
        if end > first:
            self.drained_upto.fill_(end)
        return rows

    def state(self) -> dict:
        """Host copy of the ring and the drain position (for the training state file)."""
        return dict(records=self.records.cpu(), interval_id=self.interval_id.cpu(), counters=self.counters.cpu(),
                    base=self.base.cpu(), drained_upto=self.drained_upto.cpu(), seen=[int(x) for x in self._seen],
                    interval=self.interval, capacity=self.capacity)

    def load_state(self, state: dict) -> None:
        if int(state["interval"]) != self.interval or int(state["capacity"]) != self.capacity:
            raise ValueError(f"state file: the training log has interval={state['interval']} capacity={state['capacity']}, the one "
                             f"built here interval={self.interval} capacity={self.capacity}")
        for name in ("records", "interval_id", "counters", "base", "drained_upto"):
            getattr(self, name).copy_(state[name])
        self._seen = [int(x) for x in state["seen"]]
        b = int(state["base"][0])
        self._base = None if b == -1 else b
