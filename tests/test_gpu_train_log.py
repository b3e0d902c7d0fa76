"""The training log on the MI355X: ``mel_train_log_round`` / ``mel_train_log_update`` on hand-built buffers against the float64
host model (tests/train_log_ref.py) - bit for bit, except the gradient norm's distance from ``math.fsum``, whose bound
``total_numel * 2^-52`` (relative) is the worst case of adding ``total_numel`` exact non-negative squares in double in any order
(<= (n - 1) * 2^-53 relative on the sum, half of it after the square root, one rounding of the root) - then the log inside
``RoundLoop``, the learners and tiny ``train`` runs.  Each case prints what it measured (run with -s)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.train_log_ref import TrainLogModel, grad_sq_sum

NOT_ARMED = -1


def _stream():
    from melissa_amd import _lib
    return _lib.current_stream_ptr(torch.device("cuda"))


class Bench:
    """A ``mel_train_log`` over hand-set decision counters and a hand-built episode log, with its host model."""

    def __init__(self, n_envs, capacity=4, interval=100, scale=1, log_capacity=None, base=0):
        from melissa_amd import _lib
        self.n_envs, self.scale = n_envs, scale
        self.log_capacity = log_capacity if log_capacity is not None else max(n_envs, 4)
        dev = "cuda"
        self.scalars = torch.zeros(n_envs, _lib.ENV_SCALARS, dtype=torch.int32, device=dev)
        self.records = torch.zeros(capacity, _lib.TRAIN_LOG_DOUBLES, dtype=torch.float64, device=dev)
        self.interval_id = torch.full((capacity,), -1, dtype=torch.int64, device=dev)
        self.counters = torch.zeros(4, dtype=torch.int64, device=dev)
        self.base = torch.full((1,), NOT_ARMED if base is None else base, dtype=torch.int64, device=dev)
        self.drained_upto = torch.zeros(1, dtype=torch.int64, device=dev)
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self.stats = torch.zeros(self.log_capacity, 10, dtype=torch.float64, device=dev)
        self.meta = torch.zeros(self.log_capacity, 3, dtype=torch.int32, device=dev)
        self.log = g = _lib.MelTrainLog()
        g.records, g.interval_id, g.counters = self.records.data_ptr(), self.interval_id.data_ptr(), self.counters.data_ptr()
        g.base, g.drained_upto = self.base.data_ptr(), self.drained_upto.data_ptr()
        g.decisions, g.stride = self.scalars.data_ptr() + 4 * _lib.S_DECISIONS, _lib.ENV_SCALARS
        g.interval, g.capacity, g.n_envs, g.scale = interval, capacity, n_envs, scale
        self.env = e = _lib.MelEnvBatch()
        e.n_envs, e.n_nodes, e.log_capacity = n_envs, 12, self.log_capacity
        e.log_cursor, e.log_stats, e.log_meta = self.cursor.data_ptr(), self.stats.data_ptr(), self.meta.data_ptr()
        self.model = TrainLogModel(capacity, interval)
        self.model.base = base
        self.env_step = 0

    def decisions(self, per_env):
        from melissa_amd import _lib
        per_env = np.asarray(per_env, dtype=np.int64)
        assert per_env.shape == (self.n_envs,) and per_env.max() < 2 ** 31
        self.scalars[:, _lib.S_DECISIONS] = torch.from_numpy(per_env.astype(np.int32)).cuda()
        self.env_step = self.scale * int(per_env.sum())

    def step_to(self, env_step):
        """Decision counters (spread over the envs) whose scaled sum is ``env_step``."""
        assert env_step % self.scale == 0
        d, per = env_step // self.scale, np.zeros(self.n_envs, dtype=np.int64)
        per[:] = d // self.n_envs
        per[: d % self.n_envs] += 1
        self.decisions(per)

    def drained(self, upto):
        self.drained_upto.fill_(upto)
        self.model.drained_upto = upto

    def round(self, stats, meta, cursor=None, eps=None):
        from melissa_amd import _lib
        n = len(stats)
        cursor = n if cursor is None else cursor
        keep = min(n, self.log_capacity)
        self.stats[:keep] = torch.from_numpy(np.asarray(stats, dtype=np.float64)[:keep]).cuda()
        self.meta[:keep] = torch.from_numpy(np.asarray(meta, dtype=np.int32)[:keep]).cuda()
        self.cursor.fill_(cursor)
        eps_dev = None if eps is None else torch.tensor([eps], dtype=torch.float32, device="cuda")
        st = _lib.load().mel_train_log_round(C.byref(self.log), C.byref(self.env), eps_dev.data_ptr() if eps is not None else None,
                                             _stream())
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert int(self.cursor.item()) == 0, "the round launch leaves the episode log empty"
        self.model.round(self.env_step, np.asarray(stats)[:keep], np.asarray(meta)[:keep], cursor, self.log_capacity, self.n_envs, eps)

    def update(self, loss, td, grads, model=True):
        from melissa_amd import _lib
        lib = _lib.load()
        dev = [torch.from_numpy(np.ascontiguousarray(g)).cuda() for g in grads]
        t = _lib.MelAdamTensors()
        t.count = len(dev)
        for i, g in enumerate(dev):
            t.grad[i], t.numel[i] = g.data_ptr(), g.numel()
        need = lib.mel_train_log_scratch_bytes(C.byref(t))
        assert need == 8 * sum(-(-g.numel() // 4096) for g in dev)
        scratch = torch.full((need // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")
        loss_dev, td_dev = torch.tensor([loss], dtype=torch.float32, device="cuda"), torch.from_numpy(td).cuda()
        st = lib.mel_train_log_update(C.byref(self.log), loss_dev.data_ptr(), td_dev.data_ptr(), len(td), C.byref(t),
                                      scratch.data_ptr(), need, _stream())
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert torch.isnan(scratch[need // 8:]).all(), "scratch written beyond mel_train_log_scratch_bytes"
        if model:
            self.model.update(self.env_step, loss, td, grads)

    def got(self):
        torch.cuda.synchronize()
        return self.records.cpu().numpy(), self.interval_id.cpu().numpy(), self.counters.cpu().numpy()

    def assert_equals_model(self, skip=()):
        rec, ids, counters = self.got()
        np.testing.assert_array_equal(ids, self.model.interval_id)
        np.testing.assert_array_equal(counters, self.model.counters)
        keep = [f for f in range(rec.shape[1]) if f not in skip]
        assert rec[:, keep].tobytes() == self.model.records[:, keep].tobytes(), (rec, self.model.records)


# ------------------------------------------------------------------------------------------------------------ 1. update launch
def _table(name):
    rng = np.random.default_rng({"one": 1, "three": 3, "many": 64}[name])
    sizes = {"one": [1], "three": [63, 64, 65],
             "many": [4097, 1005315] + [int(x) for x in rng.integers(1, 3000, 60)] + [1, 4096]}[name]
    assert len(sizes) <= 64
    grads = []
    for i, n in enumerate(sizes):
        if i % 2:                # exactly representable: small integers and halves
            grads.append((rng.integers(-8, 9, n) * 0.5).astype(np.float32))
        else:
            grads.append((rng.standard_normal(n) * 10.0 ** rng.integers(-3, 2)).astype(np.float32))
    return grads


@pytest.fixture(scope="module")
def tables():
    """The gradient tables with their exact squared norm (math.fsum over float64 squares, each exact), computed once."""
    out = {}
    for name in ("one", "three", "many"):
        grads = _table(name)
        exact = math.fsum(math.fsum((g.astype(np.float64) ** 2).tolist()) for g in grads)
        out[name] = (grads, math.sqrt(exact), sum(g.size for g in grads))
    return out


@pytest.mark.parametrize("batch", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("table", ["one", "three", "many"])
def test_update_launch(tables, table, batch):
    from melissa_amd import _lib
    grads, exact_norm, numel = tables[table]
    rng = np.random.default_rng(batch)
    td = rng.standard_normal(batch).astype(np.float32)
    td[::3] = np.round(td[::3] * 4) / 4                               # some exactly representable
    loss = np.float32(rng.random())
    benches = [Bench(3, interval=100), Bench(3, interval=100)]
    for b in benches:
        b.step_to(120)
        # the model of the big table is not recomputed per batch: its norm is checked against fsum below, the rest against the model
        b.update(loss, td, grads, model=table != "many")
        if table != "many":
            b.update(np.float32(loss * 2), td[::-1].copy(), grads)    # a second update into the same record: sums in stream order
    rec = benches[0].got()[0][1]
    assert benches[0].got()[0].tobytes() == benches[1].got()[0].tobytes(), "two calls on the same inputs give the same bits"
    if table != "many":
        benches[0].assert_equals_model()
        norm = rec[_lib.TL_GRAD_NORM_LAST]
    else:
        m = TrainLogModel(4, 100)
        m.base = 0
        m.update(120, loss, td, [np.zeros(1, np.float32)])
        norm_fields = (_lib.TL_GRAD_NORM_SUM, _lib.TL_GRAD_NORM_MAX, _lib.TL_GRAD_NORM_LAST)
        keep = [f for f in range(rec.size) if f not in norm_fields]
        assert rec[keep].tobytes() == m.records[1][keep].tobytes()
        norm = rec[_lib.TL_GRAD_NORM_LAST]
        assert norm == rec[_lib.TL_GRAD_NORM_SUM] == rec[_lib.TL_GRAD_NORM_MAX]
    err = abs(norm - exact_norm) / exact_norm
    print(f"update {table} batch {batch}: grad_norm {norm!r}, relative error {err:.3e}, bound {numel * 2.0 ** -52:.3e}")
    assert err <= numel * 2.0 ** -52


def test_update_launch_big_table_equals_the_model_bits(tables):
    """The fixed order of the partial sums, restated on the host: the same double, not only one within the bound."""
    from melissa_amd import _lib
    grads = tables["many"][0]
    b = Bench(3)
    b.step_to(7)
    b.update(np.float32(0.5), np.ones(2, np.float32), grads, model=False)
    assert b.got()[0][0][_lib.TL_GRAD_NORM_LAST] == math.sqrt(grad_sq_sum(grads))


def test_update_launch_nan_propagates():
    from melissa_amd import _lib
    grads = [np.ones(70, np.float32), np.ones(5000, np.float32)]
    grads[1][4500] = np.nan
    td = np.ones(65, np.float32)
    b = Bench(3)
    b.step_to(10)
    b.update(np.float32(1.0), td, [np.ones(3, np.float32)])
    b.update(np.float32(2.0), td, grads)
    b.update(np.float32(3.0), td, [np.ones(3, np.float32)])           # a later clean update does not wash it out of sum and max
    td_nan = td.copy()
    td_nan[64] = np.nan
    b.step_to(110)
    b.update(np.float32("nan"), td_nan, [np.ones(3, np.float32)])
    b.assert_equals_model()
    rec = b.got()[0]
    assert math.isnan(rec[0][_lib.TL_GRAD_NORM_SUM]) and math.isnan(rec[0][_lib.TL_GRAD_NORM_MAX])
    assert rec[0][_lib.TL_GRAD_NORM_LAST] == math.sqrt(3.0) and rec[0][_lib.TL_LOSS_MAX] == 3.0
    for f in (_lib.TL_LOSS_SUM, _lib.TL_LOSS_MAX, _lib.TL_LOSS_LAST, _lib.TL_TD_ABS_SUM, _lib.TL_TD_ABS_MEAN_MAX, _lib.TL_TD_ABS_MAX):
        assert math.isnan(rec[1][f]), f


# ------------------------------------------------------------------------------------------------------------- 2. round launch
def _episode_rows(n_envs, rng, share=0.6):
    """One finished episode for a random ``share`` of the envs, in env order."""
    envs = np.flatnonzero(rng.random(n_envs) < share)
    if len(envs) == 0:
        envs = np.array([n_envs - 1])
    stats, meta = rng.standard_normal((len(envs), 10)) * 7.0, np.zeros((len(envs), 3), dtype=np.int32)
    stats[:, 1], stats[:, 6], stats[:, 0] = rng.random(len(envs)), rng.random(len(envs)), rng.integers(1, 90, len(envs))
    meta[:, 0], meta[:, 1], meta[:, 2] = envs, rng.integers(0, 1000, len(envs)), rng.integers(3, 60, len(envs))
    return stats, meta


@pytest.mark.parametrize("n_envs", [3, 64, 65, 257])
def test_round_launch_equals_the_model_in_any_row_order(n_envs):
    rng = np.random.default_rng(n_envs)
    stats, meta = _episode_rows(n_envs, rng)
    stats2, meta2 = _episode_rows(n_envs, rng)
    results = []
    for order in (np.arange(len(stats)), np.arange(len(stats))[::-1], rng.permutation(len(stats))):
        b = Bench(n_envs, interval=1000)
        b.step_to(40)
        b.round(stats[order], meta[order], eps=0.75)
        b.step_to(90)
        b.round(stats2, meta2, eps=0.5)                                # a second round into the same record
        b.round(stats[:0], meta[:0])                                   # zero rows: a round all the same, eps kept
        b.assert_equals_model()
        results.append(b.got()[0].tobytes())
    assert results[0] == results[1] == results[2], "the record depends on the order the rows were appended in"
    print(f"round {n_envs} envs: {len(stats)} + {len(stats2)} rows")


def test_round_launch_overflow_duplicates_and_unarmed():
    from melissa_amd import _lib
    rng = np.random.default_rng(5)
    stats, meta = _episode_rows(65, rng, share=1.0)
    b = Bench(65, log_capacity=40)
    b.step_to(10)
    b.round(stats, meta, cursor=65)                                    # 65 episodes ended, the log kept 40
    b.assert_equals_model()
    assert b.got()[2].tolist() == [0, 25, 0, 0] and b.got()[0][0][_lib.TL_EPISODES] == 40
    # two rows of env 7 (episodes 900 and 12, in that row order) and two of env 64: counted, folded in (env, episode) order
    stats, meta = _episode_rows(65, rng, share=0.3)
    extra_s, extra_m = rng.standard_normal((2, 10)), np.array([[7, 900, 5], [64, 3, 9]], dtype=np.int32)
    meta[meta[:, 0] == 7, 1], meta[meta[:, 0] == 64, 1] = 12, 800
    if not (meta[:, 0] == 7).any():
        extra_s, extra_m = np.vstack([extra_s, rng.standard_normal((1, 10))]), np.vstack([extra_m, [[7, 12, 4]]]).astype(np.int32)
    if not (meta[:, 0] == 64).any():
        extra_s, extra_m = np.vstack([extra_s, rng.standard_normal((1, 10))]), np.vstack([extra_m, [[64, 800, 4]]]).astype(np.int32)
    s2, m2 = np.vstack([extra_s, stats]), np.vstack([extra_m, meta])
    images = []
    for order in (np.arange(len(s2)), np.arange(len(s2))[::-1]):
        d = Bench(65, log_capacity=80)
        d.step_to(10)
        d.round(s2[order], m2[order])
        d.assert_equals_model()
        assert d.got()[2].tolist() == [0, 0, 2, 0]
        images.append(d.got()[0].tobytes())
    assert images[0] == images[1]
    # not armed, and armed with env_step < base: rows are consumed, nothing is recorded, no counter moves
    for base, step in ((None, 500), (1000, 999)):
        u = Bench(65, log_capacity=40, base=base)
        u.step_to(step)
        u.round(s2, m2, cursor=len(s2))
        u.update(np.float32(1.0), np.ones(4, np.float32), [np.ones(4, np.float32)])
        rec, ids, counters = u.got()
        assert not rec.any() and (ids == -1).all() and not counters.any()
        u.assert_equals_model()


# -------------------------------------------------------------------------------------------------------------------- 3. slots
def test_slots_intervals_wrap_and_scale():
    from melissa_amd import _lib
    rng = np.random.default_rng(9)
    b = Bench(5, capacity=2, interval=100, base=1000)
    one = lambda: _episode_rows(5, rng)
    td, g = np.ones(3, np.float32), [np.ones(3, np.float32)]
    for step in (1000, 1050, 1099):                                    # one interval
        b.step_to(step)
        b.round(*one(), eps=0.5)
        b.update(np.float32(0.5), td, g)                               # ... and the update lands in the round's slot
    assert b.got()[1].tolist() == [0, -1]
    b.step_to(1100)                                                    # across one boundary
    b.update(np.float32(0.25), td, g)
    b.round(*one())
    assert b.got()[1].tolist() == [0, 1] and b.got()[2][_lib.TLC_LOST_RECORDS] == 0
    rec = b.got()[0]
    assert rec[0][_lib.TL_ROUNDS] == 3 and rec[0][_lib.TL_UPDATES] == 3 and rec[1][_lib.TL_ROUNDS] == 1 and rec[1][_lib.TL_UPDATES] == 1
    b.step_to(1200)                                                    # wraps onto interval 0, which nobody drained: lost
    b.round(*one())
    assert b.got()[1].tolist() == [2, 1] and b.got()[2][_lib.TLC_LOST_RECORDS] == 1
    b.drained(2)
    b.step_to(1310)                                                    # interval 1 was drained: overwritten without a loss
    b.update(np.float32(0.25), td, g)
    assert b.got()[1].tolist() == [2, 3] and b.got()[2][_lib.TLC_LOST_RECORDS] == 1
    b.step_to(1990)                                                    # several intervals skipped: 9 takes slot 1 from 3 (not drained)
    b.round(*one())
    assert b.got()[1].tolist() == [2, 9] and b.got()[2][_lib.TLC_LOST_RECORDS] == 2
    b.assert_equals_model()
    # scale = 8 and counters whose sum passes 2^32: the 64-bit sum
    w = Bench(5, capacity=3, interval=10 ** 9, scale=8, base=8 * 5 * 2 ** 30)
    w.decisions([2 ** 30] * 5)
    assert w.env_step == 8 * 5 * 2 ** 30 > 2 ** 35
    w.round(*one(), eps=0.1)
    w.decisions([2 ** 30 + 2 ** 28] * 5)                               # + 8 * 5 * 2^28 = 1.07e10 env steps: interval 10
    w.update(np.float32(0.5), td, g)
    w.round(*one())
    assert w.got()[1].tolist() == [0, 10, -1] and w.got()[0][1][_lib.TL_ENV_STEP_LAST] == float(w.env_step)
    w.assert_equals_model()


# ------------------------------------------------------------------------------------------------------------ 4. bad arguments
def test_bad_arguments():
    from melissa_amd import _lib
    lib = _lib.load()
    b = Bench(3)
    td, loss = torch.ones(4, device="cuda"), torch.ones(1, device="cuda")
    g = torch.ones(5000, device="cuda")
    t = _lib.MelAdamTensors()
    t.count, t.grad[0], t.numel[0] = 1, g.data_ptr(), g.numel()
    scratch = torch.zeros(2, dtype=torch.float64, device="cuda")
    good_round = lambda: lib.mel_train_log_round(C.byref(b.log), C.byref(b.env), None, _stream())
    good_update = lambda batch=4, bytes_=16: lib.mel_train_log_update(C.byref(b.log), loss.data_ptr(), td.data_ptr(), batch, C.byref(t),
                                                                     scratch.data_ptr(), bytes_, _stream())
    assert good_round() == 0 and good_update() == 0
    assert lib.mel_train_log_round(None, C.byref(b.env), None, _stream()) == _lib.ERR_INVALID_ARG
    assert lib.mel_train_log_round(C.byref(b.log), None, None, _stream()) == _lib.ERR_INVALID_ARG
    for field, bad in (("capacity", 0), ("interval", 0), ("n_envs", 0), ("stride", 0), ("records", None), ("interval_id", None),
                       ("counters", None), ("base", None), ("drained_upto", None), ("decisions", None)):
        old = getattr(b.log, field)
        setattr(b.log, field, bad)
        assert good_round() == _lib.ERR_INVALID_ARG and good_update() == _lib.ERR_INVALID_ARG, field
        assert field in _lib.last_error() or "null buffer" in _lib.last_error()
        setattr(b.log, field, old)
    old = b.env.log_capacity
    b.env.log_capacity = 0                                             # an env batch without an episode log
    assert good_round() == _lib.ERR_INVALID_ARG and "no episode log" in _lib.last_error()
    b.env.log_capacity = old
    b.env.n_envs = 4
    assert good_round() == _lib.ERR_INVALID_ARG
    b.env.n_envs = 3
    assert good_update(batch=0) == _lib.ERR_INVALID_ARG and good_update(batch=_lib.TD_MAX_BATCH + 1) == _lib.ERR_INVALID_ARG
    assert good_update(bytes_=8) == _lib.ERR_WORKSPACE and "16 needed" in _lib.last_error()
    assert lib.mel_train_log_update(C.byref(b.log), None, td.data_ptr(), 4, C.byref(t), scratch.data_ptr(), 16, _stream()) == _lib.ERR_INVALID_ARG
    assert lib.mel_train_log_update(C.byref(b.log), loss.data_ptr(), None, 4, C.byref(t), scratch.data_ptr(), 16, _stream()) == _lib.ERR_INVALID_ARG
    assert lib.mel_train_log_update(C.byref(b.log), loss.data_ptr(), td.data_ptr(), 4, None, scratch.data_ptr(), 16, _stream()) == _lib.ERR_INVALID_ARG
    t.count = 65
    assert good_update() == _lib.ERR_INVALID_ARG
    t.count, t.grad[0] = 1, None
    assert good_update() == _lib.ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert good_round() == 0


# ---------------------------------------------------------------------------------------------------------------- 5, 6. the loop
N, B, ROUNDS = 12, 6, 64


def _loop(model, log, use_graph, graph_rounds=1, big_episode_log=False):
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DGNPolicy, DQNPolicy
    from melissa_amd.replay import RoundReplay
    from melissa_amd.train import build_network
    from melissa_amd.train_log import TrainLog
    torch.manual_seed(3)
    net = build_network(model, N, torch.device("cuda"))
    venv = HipGraphVectorEnv(B, N, graph_pool=synthetic_graph_pool(N, 4, first_seed=5), dynamic_graph=True, device="cuda", max_moves=48,
                             construct_like_reference=False)
    tl = None
    if log:
        tl = TrainLog(venv, interval=40, capacity=256)
        tl.arm(0)
    elif big_episode_log:
        venv.enable_episode_log(4096)
    replay = RoundReplay(B, N, 8, "cuda")
    policy = (DGNPolicy if model == "dgn_r" else DQNPolicy)(net)
    loop = RoundLoop(venv, policy, seed=3, eps=0.1, use_graph=use_graph, graph_rounds=graph_rounds, replay=replay, train_log=tl)
    return loop, venv, replay, tl


def _image(loop, venv, replay):
    torch.cuda.synchronize()
    parts = [venv.scalars(), venv.node_sets(), venv.positions(), loop.act, loop.live, replay.obs, replay.obs_next, replay.acted,
             replay.done, replay.act, replay.rew, replay.episode, replay.cursor]
    return [p.cpu().numpy().copy() for p in parts], loop.counters()


@pytest.mark.parametrize("model", ["l_dgn", "dgn_r"])
def test_loop_eager_and_captured_records_are_the_models(model):
    from melissa_amd import _lib
    logs, images = [], []
    for use_graph, graph_rounds in ((False, 1), (True, 4)):
        loop, venv, replay, tl = _loop(model, True, use_graph, graph_rounds)
        with torch.no_grad():
            loop.run(ROUNDS)
        images.append(_image(loop, venv, replay))
        assert (loop.group_graph is not None) == use_graph
        assert tl.read_counters() == dict(lost_records=0, lost_episodes=0, duplicate_env_rows=0)
        logs.append((tl.records.cpu().numpy(), tl.interval_id.cpu().numpy(), tl))
    assert logs[0][0].tobytes() == logs[1][0].tobytes() and (logs[0][1] == logs[1][1]).all()
    # an eager twin without the training log, with a large episode log that is never reset: its rows, round by round, into the model
    loop, venv, replay, _ = _loop(model, False, False, big_episode_log=True)
    m = TrainLogModel(256, 40)
    m.base = 0
    seen = 0
    with torch.no_grad():
        for _ in range(ROUNDS):
            loop.run(1)
            stats, meta, total = venv.read_episode_log()
            env_step = int(venv.scalars()[:, _lib.S_DECISIONS].sum().item())
            m.round(env_step, stats[seen:], meta[seen:], total - seen, 64, B)
            seen = total
    # 6. the log changes nothing else: the twin ran without it
    for mine, theirs in zip(images[0][0], _image(loop, venv, replay)[0]):
        np.testing.assert_array_equal(mine, theirs)
    assert images[0][1] == loop.counters() == images[1][1]
    assert seen > 10 and (m.interval_id >= 0).sum() > 5
    np.testing.assert_array_equal(logs[0][1], m.interval_id)
    assert logs[0][0].tobytes() == m.records.tobytes()
    rows = logs[0][2].drain(final=True)
    assert sum(r.get("train/episode", 0) for r in rows) == seen and [r["env_step"] for r in rows] == [40 * (i + 1) for i in range(len(rows))]
    print(f"{model}: {seen} episodes in {len(rows)} intervals over {ROUNDS} rounds")


# ------------------------------------------------------------------------------------------------------------- 7, 8. train runs
RUN = dict(model="l_dgn", n_nodes=N, envs=B, test_num=2, exploration_fraction=1.0, model_name="run", log=lambda line: None,
           epoch=2, step_per_epoch=300, batch_size=8, log_interval=100)
PACED = dict(update_per_step=0.1, step_per_collect=10, buffer_size=8 * N * B)


def _train(monkeypatch_ctx, **kw):
    """train(...) -> (result, rows of the file, the run's TrainLog, episodes the envs had finished when the log was armed)"""
    from melissa_amd import _lib
    from melissa_amd.train import train
    from melissa_amd.train_log import TrainLog
    seen = {}
    arm, load_state = TrainLog.arm, TrainLog.load_state

    def spy_arm(self, base):
        seen["log"], seen["episodes_at_base"] = self, int(self.venv.scalars()[:, _lib.S_EPISODES_DONE].sum().item())
        return arm(self, base)

    def spy_load(self, state):
        seen["log"] = self
        return load_state(self, state)

    monkeypatch_ctx.setattr(TrainLog, "arm", spy_arm)
    monkeypatch_ctx.setattr(TrainLog, "load_state", spy_load)
    out = train(**dict(RUN, **kw))
    rows = [json.loads(line) for line in open(out["log_file"])] if "log_file" in out else None
    return out, rows, seen.get("log"), seen.get("episodes_at_base")


def _check_file(out, rows, log, episodes_at_base):
    assert out["log_rows"] == len(rows)
    tests = [r for r in rows if "epoch" in r]
    curve = [r for r in rows if "epoch" not in r]
    assert [r["epoch"] for r in tests] == [0, 1, 2] and all(set(r) == {"env_step", "epoch", "test/reward", "test/reward_std", "test/length"}
                                                          for r in tests)
    assert [r["test/reward"] for r in tests] == [e["test_rew"] for e in out["epochs"]]
    base = tests[0]["env_step"]
    assert [r["env_step"] for r in curve] == [base + 100 * (i + 1) for i in range(len(curve))], "intervals are consecutive"
    assert all(r["ranks_pooled"] == 1 for r in curve) and len(curve) >= 6
    assert sum(r.get("train/episode", 0) for r in curve) == out["episodes"] - episodes_at_base
    assert sum(r.get("update/n", 0) for r in curve) == out["updates"]
    assert [r for r in curve if "update/n" in r][-1]["update/loss_last"] == out["loss_last"]
    assert all(0.0 < r["train/eps"] <= 1.0 for r in curve if "train/eps" in r)
    assert log.read_counters() == dict(lost_records=0, lost_episodes=0, duplicate_env_rows=0)
    print(f"{len(curve)} intervals, {out['episodes'] - episodes_at_base} episodes, {out['updates']} updates, last row {curve[-1]}")


def test_train_unpaced_eager_updates(tmp_path, monkeypatch):
    out, rows, log, at_base = _train(monkeypatch, logdir=str(tmp_path), capture_updates=False)
    assert out["log_file"] == os.path.join(str(tmp_path), "l_dgn", "run_progress.jsonl") and not out["updates_from_hip_graphs"]
    _check_file(out, rows, log, at_base)


def test_train_paced_captured_updates_and_resume(tmp_path, monkeypatch):
    kw = dict(PACED, save_state=True, capture_updates=True)
    S, s_rows, log, at_base = _train(monkeypatch, logdir=str(tmp_path / "straight"), **kw)
    assert S["updates_from_hip_graphs"]
    _check_file(S, s_rows, log, at_base)
    A, a_rows, _, _ = _train(monkeypatch, logdir=str(tmp_path / "cut"), stop_after_epoch=1, **kw)
    assert [r["epoch"] for r in a_rows if "epoch" in r] == [0, 1]
    state = torch.load(A["state_path"], map_location="cpu", weights_only=True)
    assert state["config"]["log_interval"] == 100 and set(state["train_log"]) >= {"records", "interval_id", "base", "drained_upto"}
    R, r_rows, log, _ = _train(monkeypatch, logdir=str(tmp_path / "cut"), resume_state=A["state_path"], **kw)
    assert R["log_file"] == A["log_file"] and R["log_rows"] == len(r_rows) - len(a_rows)
    assert open(R["log_file"]).read() == open(S["log_file"]).read(), "the resumed run leaves the straight run's file"
    assert R["param_checksum"] == S["param_checksum"] and log.read_counters() == dict(lost_records=0, lost_episodes=0, duplicate_env_rows=0)


def test_a_state_written_with_the_log_off_has_todays_keys(tmp_path, monkeypatch):
    from melissa_amd import train_state
    out, rows, log, _ = _train(monkeypatch, logdir=str(tmp_path), log_interval=None, save_state=True, epoch=1, capture_updates=False)
    assert rows is None and log is None and "log_file" not in out and "log_rows" not in out
    assert not os.path.exists(os.path.join(str(tmp_path), "l_dgn", "run_progress.jsonl"))
    state = torch.load(out["state_path"], map_location="cpu", weights_only=True)
    assert set(state) == {"format", "config", "run", "policy", "learner", "rng", "replay", "loop", "venv", "stream"}
    assert set(state["config"]) == set(train_state.HEADER_KEYS) | {"state_epoch"}
    assert set(state["venv"]) == {"state"}
    assert all("rew_std" not in e for e in out["epochs"])
