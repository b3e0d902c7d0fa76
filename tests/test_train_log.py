"""The training log's host side without a GPU: the command line and keyword checks, the ring's size, the JSONL writer, the rows a
record becomes, the ctypes mirror of ``mel_train_log``, the state header's optional key, and the float64 host model of the two
launches (tests/train_log_ref.py) against records computed by hand."""
import ctypes as C
import json
import math

import numpy as np
import pytest

from melissa_amd import _lib, train_log, train_state
from melissa_amd.train import parse_args, train, train_kwargs
from tests.train_log_ref import TrainLogModel, empty_record, grad_sq_sum, td_stats


def test_the_parsers_take_the_flags():
    a = parse_args(["--epoch", "2", "--log-interval", "1000", "--log-file", "curve.jsonl"])
    kw = train_kwargs(a)
    assert kw["log_interval"] == 1000 and kw["log_file"] == "curve.jsonl"
    kw = train_kwargs(parse_args(["--epoch", "2"]))
    assert kw["log_interval"] is None and kw["log_file"] is None


def test_log_interval_needs_epoch(capsys):
    with pytest.raises(SystemExit):
        parse_args(["--log-interval", "1000"])
    assert "needs epoch" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        parse_args(["--epoch", "2", "--log-file", "x.jsonl"])
    with pytest.raises(ValueError, match="needs epoch"):
        train(log_interval=1000)
    with pytest.raises(ValueError, match="needs log_interval"):
        train(epoch=2, log_file="x.jsonl")
    with pytest.raises(ValueError, match=">= 1"):
        train(epoch=2, log_interval=0)


def test_ring_capacity():
    assert train_log.ring_capacity(100000, 1000) == 104
    assert train_log.ring_capacity(300, 100) == 7
    assert train_log.ring_capacity(301, 100) == 8                     # a started interval is an interval
    assert train_log.ring_capacity(300, 100, overshoot=250) == 10     # ... of the overshoot too
    assert train_log.ring_capacity(10, 1000) == 5
    assert train_log.default_log_file("log", "l_dgn", "run").replace("\\", "/") == "log/l_dgn/run_progress.jsonl"


def test_the_writer_appends(tmp_path):
    path = str(tmp_path / "deep" / "er" / "p.jsonl")
    assert train_log.append_rows(path, [{"env_step": 100, "train/episode": 2}, {"env_step": 200}]) == 2
    assert train_log.append_rows(path, []) == 0
    assert train_log.append_rows(path, [{"env_step": 300, "epoch": 1, "test/reward": -1.5}]) == 1      # (a resumed run)
    rows = [json.loads(line) for line in open(path)]
    assert [r["env_step"] for r in rows] == [100, 200, 300] and rows[2]["test/reward"] == -1.5


def test_keys_whose_count_is_zero_are_absent():
    rec = empty_record()
    assert train_log.row_from_record(rec, 3, 1000, 100) == {"env_step": 1400}
    rec[_lib.TL_ROUNDS], rec[_lib.TL_EPS_LAST] = 4.0, 0.25
    assert train_log.row_from_record(rec, 0, 0, 100) == {"env_step": 100, "train/eps": 0.25}
    rec[_lib.TL_EPISODES], rec[_lib.TL_REW_SUM], rec[_lib.TL_REW_SQ] = 2.0, -6.0, 20.0
    rec[_lib.TL_REW_MIN], rec[_lib.TL_REW_MAX], rec[_lib.TL_MOVES_SUM] = -4.0, -2.0, 30.0
    row = train_log.row_from_record(rec, 0, 0, 100)
    assert row["train/episode"] == 2 and row["train/reward"] == -3.0 and row["train/reward_std"] == 1.0
    assert row["train/length"] == 15.0 and row["train/reward_min"] == -4.0 and not any(k.startswith("update/") for k in row)
    rec[_lib.TL_UPDATES], rec[_lib.TL_LOSS_SUM], rec[_lib.TL_LOSS_LAST], rec[_lib.TL_GRAD_NORM_SUM] = 4.0, 2.0, 0.125, 8.0
    row = train_log.row_from_record(rec, 0, 0, 100)
    assert row["update/n"] == 4 and row["update/loss"] == 0.5 and row["update/loss_last"] == 0.125 and row["update/grad_norm"] == 2.0
    assert set(k for k in row if k.startswith("train/")) == {
        "train/episode", "train/reward", "train/reward_std", "train/reward_min", "train/reward_max", "train/length", "train/eps",
        "train/coverage", "train/coverage_interested", "train/messages"}
    assert set(k for k in row if k.startswith("update/")) == {
        "update/loss", "update/n", "update/loss_max", "update/loss_last", "update/td_abs", "update/td_abs_max", "update/grad_norm",
        "update/grad_norm_max"}


def test_ctypes_mirror_of_the_struct():
    lib = _lib.load()
    assert C.sizeof(_lib.MelTrainLog) == lib.mel_abi_sizeof(14) == 72
    for name in ("mel_train_log_round", "mel_train_log_update", "mel_train_log_scratch_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    t = _lib.MelAdamTensors()
    t.count = 3
    for i, n in enumerate((1, 4096, 4097)):
        t.grad[i], t.numel[i] = 256 * (i + 1), n
    assert lib.mel_train_log_scratch_bytes(C.byref(t)) == 8 * (1 + 1 + 2)
    t.count = 65
    assert lib.mel_train_log_scratch_bytes(C.byref(t)) == 0


def test_state_header_takes_log_interval_only_when_given():
    base = dict(model="l_dgn", epoch=2)
    plain, logged = train_state.state_header(**base), train_state.state_header(**base, log_interval=100)
    assert "log_interval" not in plain and logged["log_interval"] == 100 and "log_interval" not in train_state.HEADER_KEYS
    train_state.check_state_header(dict(plain, state_epoch=1), plain)
    train_state.check_state_header(dict(logged, state_epoch=1), logged)
    with pytest.raises(train_state.StateMismatch, match="log_interval=100"):
        train_state.check_state_header(dict(logged, state_epoch=1), plain)
    with pytest.raises(train_state.StateMismatch, match="log_interval=None"):
        train_state.check_state_header(dict(plain, state_epoch=1), logged)


def _rows(rows):
    """(env, pool episode, num_moves, reward, coverage, coverage_interested, messages) -> (stats [n, 10], meta [n, 3])"""
    stats, meta = np.zeros((len(rows), 10)), np.zeros((len(rows), 3), dtype=np.int32)
    for r, (b, ep, moves, rew, cov, covi, msgs) in enumerate(rows):
        meta[r] = (b, ep, moves)
        stats[r, 9], stats[r, 1], stats[r, 6], stats[r, 0] = rew, cov, covi, msgs
    return stats, meta


def test_host_model_round_by_hand():
    m = TrainLogModel(capacity=2, interval=100)
    stats, meta = _rows([(2, 7, 10, -3.0, 0.5, 0.25, 12.0), (0, 4, 20, -1.0, 1.0, 0.75, 8.0)])
    m.round(50, stats, meta, 2, 8, 3, eps=0.5)                         # not armed: nothing
    assert (m.interval_id == -1).all() and not m.records.any() and not m.counters.any()
    m.base = 100
    m.round(99, stats, meta, 2, 8, 3, eps=0.5)                         # before the base: nothing
    assert (m.interval_id == -1).all() and not m.counters.any()
    m.round(150, stats, meta, 2, 8, 3, eps=0.5)
    m.round(199, stats[:0], meta[:0], 0, 8, 3, eps=0.25)               # no row: a round all the same
    rec = m.records[0]
    want = empty_record()
    want[[_lib.TL_EPISODES, _lib.TL_REW_SUM, _lib.TL_REW_SQ, _lib.TL_REW_MIN, _lib.TL_REW_MAX]] = (2, -4, 10, -3, -1)
    want[[_lib.TL_MOVES_SUM, _lib.TL_COVERAGE_SUM, _lib.TL_COV_INTERESTED_SUM, _lib.TL_MESSAGES_SUM]] = (30, 1.5, 1.0, 20)
    want[[_lib.TL_ROUNDS, _lib.TL_ENV_STEP_LAST, _lib.TL_EPS_LAST]] = (2, 199, 0.25)
    np.testing.assert_array_equal(rec, want)
    assert m.interval_id.tolist() == [0, -1]
    # the log overflowed by 3, one row names no env, env 0 has two rows (folded in episode order: sums do not show it, the counter does)
    stats, meta = _rows([(0, 9, 1, 1.0, 0, 0, 0), (5, 1, 1, 100.0, 0, 0, 0), (0, 3, 1, 2.0, 0, 0, 0)])
    m.round(200, stats, meta, 6, 3, 3)
    assert m.interval_id.tolist() == [0, 1] and m.counters.tolist() == [0, 4, 1, 0]
    assert m.records[1][_lib.TL_EPISODES] == 2 and m.records[1][_lib.TL_REW_SUM] == 3.0 and m.records[1][_lib.TL_EPS_LAST] == -1.0
    # the ring wraps: interval 2 takes interval 0's slot, which nobody read (lost); after a drain up to 2 interval 3 loses nothing
    m.round(300, stats[:0], meta[:0], 0, 3, 3)
    assert m.interval_id.tolist() == [2, 1] and m.counters[_lib.TLC_LOST_RECORDS] == 1
    m.drained_upto = 2
    m.round(400, stats[:0], meta[:0], 0, 3, 3)
    assert m.interval_id.tolist() == [2, 3] and m.counters[_lib.TLC_LOST_RECORDS] == 1
    m.round(1000, stats[:0], meta[:0], 0, 3, 3)                        # several intervals skipped: 9 -> slot 1, interval 3 (>= 2) lost
    assert m.interval_id.tolist() == [2, 9] and m.counters[_lib.TLC_LOST_RECORDS] == 2


def test_host_model_update_by_hand():
    m = TrainLogModel(capacity=4, interval=10)
    m.base = 0
    td = np.array([1.0, -3.0, 0.5, -0.5], dtype=np.float32)
    m.update(5, np.float32(0.75), td, [np.array([3.0], np.float32), np.array([0.0, 4.0], np.float32)])
    m.update(9, np.float32(0.25), td * 2, [np.array([12.0], np.float32), np.array([5.0, 0.0], np.float32)])
    rec = m.records[0]
    assert rec[_lib.TL_UPDATES] == 2 and rec[_lib.TL_LOSS_SUM] == 1.0 and rec[_lib.TL_LOSS_MAX] == 0.75 and rec[_lib.TL_LOSS_LAST] == 0.25
    assert rec[_lib.TL_TD_ABS_SUM] == 1.25 + 2.5 and rec[_lib.TL_TD_ABS_MEAN_MAX] == 2.5 and rec[_lib.TL_TD_ABS_MAX] == 6.0
    assert rec[_lib.TL_GRAD_NORM_SUM] == 18.0 and rec[_lib.TL_GRAD_NORM_MAX] == 13.0 and rec[_lib.TL_GRAD_NORM_LAST] == 13.0
    assert rec[_lib.TL_ENV_STEP_LAST] == 9 and rec[_lib.TL_ROUNDS] == 0 and rec[_lib.TL_EPISODES] == 0
    m.update(10, np.float32("nan"), td, [np.array([float("nan"), 1.0], np.float32)])
    m.update(11, np.float32(1.0), td, [np.array([1.0], np.float32)])
    rec = m.records[1]
    assert math.isnan(rec[_lib.TL_LOSS_MAX]) and math.isnan(rec[_lib.TL_GRAD_NORM_MAX]) and rec[_lib.TL_LOSS_LAST] == 1.0
    assert rec[_lib.TL_GRAD_NORM_LAST] == 1.0 and rec[_lib.TL_TD_ABS_MAX] == 3.0


def test_host_model_sums_against_fsum():
    rng = np.random.default_rng(0)
    grads = [rng.standard_normal(n).astype(np.float32) for n in (1, 63, 4097, 70001)]
    exact = math.fsum(float(x) * float(x) for g in grads for x in g)
    total = sum(g.size for g in grads)
    assert abs(grad_sq_sum(grads) - exact) <= total * 2.0 ** -52 * exact
    td = rng.standard_normal(300).astype(np.float32)
    asum, amax = td_stats(td)
    assert abs(asum - math.fsum(abs(float(x)) for x in td)) <= 300 * 2.0 ** -52 * asum and amax == float(np.abs(td).max())
