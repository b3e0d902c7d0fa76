"""The trace ring's host arithmetic (melissa_amd/record_common.py), without a GPU: what a drain yields, in which order and with
how many records lost, when the device has overrun the ring - on the payload arrays of both recorders."""
import types

import numpy as np
import pytest
import torch

from melissa_amd import _lib as L
from melissa_amd.decision_record import DecisionRecorder
from melissa_amd.record_common import drain_ring
from melissa_amd.round_record import RoundRecorder

CAP, N, ENV = 4, 70, 5
READS = [(3, list(range(0, 3)), 0), (7, list(range(3, 7)), 0), (13, list(range(9, 13)), 2)]      # cursor, records drained, lost


def write_record(arrays: dict, t: int, j: int) -> None:
    """What the device does for record j of slot t: header and payload into ring slot j % CAP, every payload element = j."""
    for a in arrays.values():
        a[t, j % CAP] = j
    arrays["meta"][t, j % CAP] = [ENV, j // 5, 0, j % 5, j, j, 0, 0]      # (ordinal j // 5, num_moves j % 5)


@pytest.mark.parametrize("cls", [RoundRecorder, DecisionRecorder])
def test_drain_ring_yields_the_new_records_in_play_order_and_counts_the_overwritten(cls):
    spec = dict(meta=((8,), "int32"), **cls.trace_spec(N, L.set_words(N)))
    host = {k: np.zeros((2, CAP, *tail), dtype=dtype) for k, (tail, dtype) in spec.items()}
    drained, written = [0, 0], 0
    for cursor, want, want_lost in READS:
        for j in range(written, cursor):
            write_record(host, 1, j)                     # slot 1 is the ring under test; slot 0 never gets a record
        written = cursor
        new, drained, lost = drain_ring([0, cursor], host, drained, CAP)
        assert new[0] == [] and drained == [0, cursor] and lost == want_lost
        assert [int(r["meta"][4]) for r in new[1]] == want
        for j, r in zip(want, new[1]):
            assert sorted(r) == sorted(spec)
            for k, (tail, dtype) in spec.items():
                assert r[k].shape == tail and r[k].dtype == np.dtype(dtype)
                if k != "meta":
                    assert (r[k] == j).all(), (k, j)     # the payload of slot j % CAP as it stood at the drain
        host["meta"][1] = -1                             # the records are copies: the ring may be overwritten afterwards
        assert [int(r["meta"][4]) for r in new[1]] == want
    assert drain_ring([0, 13], host, drained, CAP) == ([[], []], [0, 13], 0)       # nothing new: nothing read


@pytest.mark.parametrize("cls", [RoundRecorder, DecisionRecorder])
def test_a_recorder_drains_accumulates_and_resets(cls, monkeypatch):
    """The recorder's own ``drain_traces`` and ``reset`` on host tensors (the device's writes done by hand)."""
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: None)
    venv = types.SimpleNamespace(env_num=8, n=N, max_moves=10, device=torch.device("cpu"), env=types.SimpleNamespace(log_capacity=1))
    rec = cls(venv, trace_envs=(ENV,), trace_capacity=CAP)
    payload = list(cls.trace_spec(N, L.set_words(N)))
    arrays = lambda: {k: getattr(rec, "trace_" + k).numpy() for k in ["meta"] + payload}      # (views of the host tensors)
    written, seen, total_lost = 0, [], 0
    for cursor, want, want_lost in READS:
        for j in range(written, cursor):
            write_record(arrays(), 0, j)
        written = cursor
        rec.trace_cursor[0] = cursor
        if cursor == 7:                                  # a buffer that moved since construction is read where it is now
            rec.trace_meta = rec.trace_meta.clone()
        traces, lost = rec.drain_traces()
        seen, total_lost = seen + want, total_lost + want_lost
        assert lost == rec.lost == total_lost and list(traces) == [ENV]
        assert [int(r["meta"][4]) for r in rec.records[ENV]] == seen
        # grouped by ordinal j // 5, rounds j % 5, in play order
        assert [(ep["ordinal"], ep["rounds"].tolist()) for ep in traces[ENV]] == \
            [(o, [j % 5 for j in seen if j // 5 == o]) for o in sorted({j // 5 for j in seen})]
        for ep in traces[ENV]:
            for k in payload:
                want_dtype = np.uint64 if getattr(rec, "trace_" + k).dtype == torch.int64 else None
                assert want_dtype is None or ep[k].dtype == want_dtype
                assert ep[k].reshape(len(ep["rounds"]), -1)[:, 0].tolist() == [j for j in seen if j // 5 == ep["ordinal"]]
    rec.reset()
    assert rec.trace_cursor.tolist() == [0] and rec._drained == [0] and rec.records == {ENV: []} and rec.lost == 0
    assert rec.drain_traces() == ({ENV: []}, 0)
    write_record(arrays(), 0, 0)
    rec.trace_cursor[0] = 1
    traces, lost = rec.drain_traces()
    assert lost == 0 and [(ep["ordinal"], ep["rounds"].tolist()) for ep in traces[ENV]] == [(0, [0])]
