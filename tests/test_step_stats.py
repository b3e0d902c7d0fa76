"""The per-step ``logger_stats`` pool without a GPU: the host model of the device accumulator (collect.StepStatsPool, the
Chan / Welford merge the env kernels run) against numpy on the rows the REAL reference recorded, the argument checks of
``mel_env_step_stats``, and the sampling contract (one sample per ``pz.step`` whose info holds stats, none per reset) on the
oracle env."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from melissa_amd import _lib
from tests.trace_replay import LOGGER_KEYS, set_ints

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "env_trace_*.npz")))


def step_rows(tr) -> np.ndarray:
    """float64 [m, 10]: the logger_stats of every ``env.step`` row of a trace that holds stats - what the reference's collector
    pools (multi_agent_collector.py:276,316-322).  Row 0 and the ``was_reset`` rows are observations after ``env.reset``."""
    has, was_reset = tr["has_stats"].astype(bool), tr["was_reset"].astype(bool)
    keep = has & ~was_reset
    keep[0] = False
    return np.asarray(tr["stats"][keep], dtype=np.float64)


def assert_pool_equals_numpy(count, summary, rows, what="", max_rows=2 ** 13):
    """count / min / max exact; mean within 1e-12 * max(1, max|x|); std within that or 1e-12 relative, whichever is looser.
    (At most 2^13 samples, a few roundings of 2^-53 per merge: the error stays under n * 2^-53 ~ 1e-12 of the magnitude;
    numpy's pairwise mean is inside the same bound.  ``max_rows=None``: a caller whose set is somewhat larger keeps the SAME
    1e-12, which is then tighter than that derivation allows.)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, len(LOGGER_KEYS))
    assert max_rows is None or len(rows) <= max_rows
    assert count == len(rows), what
    if len(rows) == 0:
        assert summary == {}, what
        return
    assert list(summary) == list(LOGGER_KEYS)
    for k, key in enumerate(LOGGER_KEYS):
        x, got = rows[:, k], summary[key]
        tol = 1e-12 * max(1.0, float(np.abs(x).max()))
        mean_err, std_err = abs(got.mean - x.mean()), abs(got.std - x.std())
        print(f"{what} {key}: n={len(x)} mean err {mean_err:.2e} std err {std_err:.2e} (tol {tol:.2e})")
        assert got.min == x.min() and got.max == x.max(), (what, key)
        assert mean_err <= tol, (what, key, got.mean, x.mean())
        assert std_err <= max(tol, 1e-12 * float(x.std())), (what, key, got.std, x.std())


def feed_in_blocks(pool, rows, rng):
    """Add ``rows`` in order; a run of identical consecutive rows goes in as ONE ``count=k`` merge now and then.
    -> the number of such block merges."""
    blocks, i = 0, 0
    while i < len(rows):
        k = 1
        while i + k < len(rows) and np.array_equal(rows[i + k], rows[i]):
            k += 1
        if k > 1 and rng.random() < 0.7:
            k = int(rng.integers(2, k + 1))
            pool.add(rows[i], count=k)
            blocks += 1
        else:
            k = 1
            pool.add(rows[i])
        i += k
    return blocks


@pytest.mark.parametrize("path", TRACES, ids=[os.path.basename(p)[10:-4] for p in TRACES])
def test_host_accumulator_matches_numpy_on_reference_rows(path):
    from melissa_amd.collect import StepStatsPool
    tr = np.load(path)
    rows = step_rows(tr)
    assert 300 <= len(rows) <= 900
    step = ~tr["was_reset"].astype(bool)
    step[0] = False
    assert tr["has_stats"].astype(bool)[step].all()               # no step row without stats in the reference's traces
    rng = np.random.default_rng(len(rows))
    blocks = 0
    for envs in range(1, 8):
        # contiguous, unequal shares (one may be empty), one accumulator per pseudo-env, merged in env order
        cuts = np.sort(rng.integers(0, len(rows) + 1, size=envs - 1))
        shares = np.split(rows, cuts)
        pools = []
        for share in shares:
            p = StepStatsPool()
            blocks += feed_in_blocks(p, share, rng)
            assert_pool_equals_numpy(p.count, p.summary(), share, f"{envs} envs, share")
            pools.append(p)
        # through the device's row layout and back, merged in a rotated order: the result may not depend on it
        total = StepStatsPool()
        for p in pools[envs // 2:] + pools[:envs // 2]:
            total.merge(StepStatsPool.from_row(p.to_row()))
        assert_pool_equals_numpy(total.count, total.summary(), rows, f"{envs} envs, merged")
    assert blocks >= 7
    # a block of k identical rows appended as one merge
    p = StepStatsPool()
    feed_in_blocks(p, rows, rng)
    p.add(rows[17], count=23)
    assert_pool_equals_numpy(p.count, p.summary(), np.concatenate([rows, np.repeat(rows[17:18], 23, axis=0)]), "tail block")


def test_constant_sequence_has_zero_std():
    from melissa_amd.collect import StepStatsPool
    value = np.array([1592.0, 0.35, 3.0, 1e5 + 1.0, 0.1, 7.0, 1.0 / 3.0, 2.0, 0.0, -12.7])
    a, b = StepStatsPool(), StepStatsPool()
    for _ in range(300):
        a.add(value)
    a.add(value, count=41)
    b.add(value, count=3)
    b.add(value)
    a.merge(b)
    s = a.summary()
    assert a.count == 345
    for k, key in enumerate(LOGGER_KEYS):
        assert s[key].std == 0.0 and s[key].mean == s[key].min == s[key].max == value[k]
    empty = StepStatsPool()
    assert empty.summary() == {} and empty.merge(StepStatsPool()).count == 0
    assert StepStatsPool().merge(a).summary() == s                       # an empty side leaves the other as it is


def test_large_near_equal_values_do_not_cancel():
    """total_messages_transmitted-sized values: a sum / sum-of-squares accumulator loses the std here, mean / M2 must not."""
    from melissa_amd.collect import StepStatsPool
    rng = np.random.default_rng(3)
    rows = np.zeros((4096, len(LOGGER_KEYS)))
    rows[:] = 1e5 + rng.integers(0, 3, size=(4096, 1))
    rows[:, 9] = -rng.uniform(0, 40, size=4096)
    p = StepStatsPool()
    for r in rows:
        p.add(r)
    assert_pool_equals_numpy(p.count, p.summary(), rows, "large")


def test_step_stats_export_validation_and_abi():
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "melissa_hip.h")).read()
    assert re.search(r"#define MEL_ENV_STEP_STATS_DOUBLES \(1 \+ 4 \* MEL_ENV_LOGGER_STATS\)", header)
    assert _lib.STEP_STATS_DOUBLES == 1 + 4 * _lib.ENV_LOGGER_STATS == 41
    assert [f[0] for f in _lib.MelEnvBatch._fields_[-2:]] == ["step_stats", "received_from"]
    assert C.sizeof(_lib.MelEnvBatch) == lib.mel_abi_sizeof(5)
    out = (C.c_double * _lib.STEP_STATS_DOUBLES)()
    env = _lib.MelEnvBatch()
    assert lib.mel_env_step_stats(None, out, 0, None) == _lib.ERR_INVALID_ARG
    assert lib.mel_env_step_stats(C.byref(env), None, 0, None) == _lib.ERR_INVALID_ARG
    env.n_envs, env.n_nodes = 4, 20
    assert lib.mel_env_step_stats(C.byref(env), out, 0, None) == _lib.ERR_INVALID_ARG        # not bound
    assert b"not bound" in lib.mel_last_error()
    # "bound" as far as the checks look (they never follow the pointers), the pool off: rejected before any launch
    env.pos = env.scalars = C.addressof(out)
    assert lib.mel_env_step_stats(C.byref(env), out, 1, None) == _lib.ERR_INVALID_ARG
    assert b"step_stats" in lib.mel_last_error()


def oracle_round_rows(pz, act_of_agent, rows):
    """One env round on the oracle in mel_env_round's order (pending dead steps, then each active agent; the driver of
    tests/test_gpu_round.py::oracle_round), recording one entry per ``pz.step``: the ten logger_stats of the info it
    returned, or None when that info holds none.  The reset at an episode's end records nothing.  -> episode ended"""
    n = pz.env.n
    for _ in range(3 * n + 4):
        sel = pz.env.agent_selection
        dead = (pz.env.terminated >> sel) & 1
        obs, rew, term, trunc, info = pz.step(0 if dead else int(act_of_agent[sel]))
        stats = info.get("logger_stats")
        rows.append(None if stats is None else [float(stats[k]) for k in LOGGER_KEYS])
        if term:
            pz.done_count += 1
            if info.get("explicit_reset") or pz.done_count == n:
                _obs, reset_info = pz.reset()
                pz.reset_infos.append(reset_info)
                pz.done_count = 0
                return True
        if info.get("environment_step"):
            return False
    raise AssertionError("round did not terminate")


def test_oracle_rounds_one_sample_per_step_none_per_reset():
    """Bookkeeping on the oracle alone: which rows the contract names (every ``pz.step`` info with stats, no reset
    observation) and that the host accumulator summarises exactly those.  The count equals the rows by construction here; that
    the KERNELS sample these rows is what tests/test_gpu_step_stats.py::test_round_pool_matches_oracle_rows checks."""
    from melissa_amd.collect import StepStatsPool
    from melissa_amd.env import synthetic_graph_pool
    from oracle import env_oracle as eo
    n, rounds = 12, 40
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    total, all_rows, episodes = StepStatsPool(), [], 0
    for b in range(3):
        env = eo.OracleGraphEnv(n, graph_pool=[eo.GraphSpec(g.pos.copy(), set_ints(g.one_hop)) for g in graphs],
                                dynamic_graph=bool(b % 2),
                                np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(77 + b))))
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count, pz.reset_infos = env, n, [0] * n, 0, []
        env.last()
        rng = np.random.RandomState(b)
        rows, pool = [], StepStatsPool()
        for _ in range(rounds):
            before = len(rows)
            episodes += oracle_round_rows(pz, rng.randint(0, 2, size=n), rows)
            for r in rows[before:]:
                if r is not None:
                    pool.add(r)
        with_stats = [r for r in rows if r is not None]
        assert len(rows) > rounds and pool.count == len(with_stats)
        # the observation after a reset holds no logger_stats: the reference's d.pop('logger_stats', {}) pools nothing
        assert pz.reset_infos and all("logger_stats" not in i for i in pz.reset_infos)
        assert_pool_equals_numpy(pool.count, pool.summary(), with_stats, f"oracle env {b}")
        total.merge(pool)
        all_rows += with_stats
    assert episodes >= 3
    assert_pool_equals_numpy(total.count, total.summary(), all_rows, "oracle, merged")


def test_collect_stats_flags_of_train_and_watch():
    """--collect-stats: parsed by both tools, handed on by train_kwargs, refused with --spread and for unknown values - all
    before anything touches a GPU."""
    from melissa_amd import train, watch
    assert train.train_kwargs(train.parse_args([]))["collect_stats"] == "episodes"
    assert train.train_kwargs(train.parse_args(["--collect-stats", "steps"]))["collect_stats"] == "steps"
    with pytest.raises(SystemExit):
        train.parse_args(["--collect-stats", "rows"])
    with pytest.raises(ValueError, match="collect_stats"):
        train.train(collect_stats="rows")
    assert watch.arg_parser().parse_args([]).collect_stats == "episodes"
    assert watch.arg_parser().parse_args(["--collect-stats", "steps"]).collect_stats == "steps"
    with pytest.raises(ValueError, match="spread"):
        watch.watch(envs=4, episodes=8, spread=True, collect_stats="steps")
    with pytest.raises(SystemExit):
        watch.main(["--envs", "4", "--spread", "--collect-stats", "steps"])
