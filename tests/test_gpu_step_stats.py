"""The per-step ``logger_stats`` pool on the GPU (mel_env_batch.step_stats, mel_env_step_stats): the AEC path against the rows
the REAL reference recorded, the round path (fast-forwards included) against the oracle played in lockstep, graph replay,
"off means off", the collectors' ``stats="steps"`` surface and the reset flag."""
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_env import OneEnvAdapter, build_venv
from tests.test_gpu_round import make_ldgn
from tests.test_step_stats import GOLDEN, LOGGER_KEYS, assert_pool_equals_numpy, step_rows
from tests.trace_replay import replay, set_int, set_ints

pytestmark = pytest.mark.gpu


def pool_of_row(row):
    from melissa_amd.collect import StepStatsPool
    p = StepStatsPool.from_row(row)
    return p.count, p.summary()


@pytest.mark.parametrize("name", ["n12_fixture_dynamic", "n20_pool_dynamic", "n20_scripted_silent_testing",
                                  "n100_pool_dynamic"])
def test_aec_pool_matches_reference_trace(name):
    """mel_env_step with an output adds one sample per call: the pool over a replayed trace equals numpy over the trace's own
    step rows (count / min / max exactly, mean / std within the derived bound); resets add nothing."""
    tr = np.load(os.path.join(GOLDEN, f"env_trace_{name}.npz"))
    venv = build_venv(tr)
    venv.enable_step_stats()
    pz = OneEnvAdapter(venv, 0)
    assert replay(tr, pz) > 300
    rows = step_rows(tr)
    assert_pool_equals_numpy(*venv.read_step_stats(), rows, f"{name} device merge")
    per_env = venv.read_step_stats(per_env=True)
    assert per_env.shape == (1, 41)
    assert_pool_equals_numpy(*pool_of_row(per_env[0]), rows, f"{name} accumulator")
    assert_pool_equals_numpy(*venv.read_step_stats(on_host=True), rows, f"{name} host merge")


def test_aec_pool_of_one_env_in_a_busy_batch():
    """The traced env is slot 3 of 5; the others are stepped with other actions in launches of their own and pool their own
    rows: the accumulators must not interfere, and the device merge must hold every env's rows."""
    tr = np.load(os.path.join(GOLDEN, "env_trace_n20_pool_dynamic.npz"))
    venv = build_venv(tr, env_num=5, slot=3)
    venv.enable_step_stats()
    others = [i for i in range(5) if i != 3]
    rng = np.random.RandomState(0)
    venv.reset(others)
    other_rows = {i: [] for i in others}

    class Busy(OneEnvAdapter):
        def step(self, a):
            obs, rew, term, trunc, info = self.venv.step(rng.randint(0, 2, size=4), others)
            for i, t, inf in zip(others, term, info):
                if "logger_stats" in inf:
                    other_rows[i].append([float(inf["logger_stats"][k]) for k in LOGGER_KEYS])
                if t and inf.get("explicit_reset"):
                    self.venv.reset([i])
            return super().step(a)

    busy = Busy(venv, 3)
    assert replay(tr, busy) > 300
    per_env = venv.read_step_stats(per_env=True)
    assert per_env.shape == (5, 41)
    assert_pool_equals_numpy(*pool_of_row(per_env[3]), step_rows(tr), "slot 3")
    for i in others:
        assert_pool_equals_numpy(*pool_of_row(per_env[i]), other_rows[i], f"slot {i}")
    everything = np.concatenate([step_rows(tr)] + [np.asarray(other_rows[i]) for i in others])
    assert_pool_equals_numpy(*venv.read_step_stats(), everything, "all five envs")


def lowest(x: int) -> int:
    return (x & -x).bit_length() - 1


def oracle_round_with_rows(pz, act_of_agent, live, rows, took):
    """One env round on the oracle in mel_env_round's order (tests/test_gpu_round.py::oracle_round), one entry per ``pz.step``
    in ``rows`` (its info's ten logger_stats, or None).  ``took``: counts the rounds in which the kernel's fast-forwards apply,
    by a hand copy of the kernel's conditions evaluated on the oracle's state - (1) pending dead agents at the start of the
    round, (2) the k - 1 early live steps, looked at when the first live agent is about to act.  The counts say that the run
    held rounds of both kinds; they do not observe which path the kernel took (a changed kernel condition would not show
    here).  What pins the kernel is the pooled values against these independently recorded rows, whichever path it takes."""
    from oracle import env_oracle as eo
    env, n = pz.env, pz.env.n
    dead = env.agents & env.terminated
    ff1 = bool(dead and env.skip_selection >= 0 and env.agent_selection == lowest(dead) and env.agents & ~dead
               and pz.done_count + eo.popcount(dead) - 1 < n)
    took["ff1"] += ff1
    dead_steps_left = eo.popcount(dead)
    seen_live = False
    for _ in range(3 * n + 4):
        env = pz.env
        sel = env.agent_selection
        is_dead = (env.terminated >> sel) & 1
        if not is_dead and not seen_live:
            seen_live = True
            took["ff2"] += bool((ff1 or not dead) and dead_steps_left == 0 and env.skip_selection == eo.SKIP_NONE
                                and not env.agents & env.terminated and live and live == env.sel_active
                                and not live & ~env.agents and sel == lowest(live) and env.sel_selected == 1 << sel
                                and eo.popcount(live) >= 2)
        dead_steps_left -= int(is_dead)
        obs, rew, term, trunc, info = pz.step(0 if is_dead else int(act_of_agent[sel]))
        stats = info.get("logger_stats")
        rows.append(None if stats is None else [float(stats[k]) for k in LOGGER_KEYS])
        if term:
            pz.done_count += 1
            if info.get("explicit_reset") or pz.done_count == n:
                pz.reset()
                pz.done_count = 0
                took["episodes"] += 1
                return
        if info.get("environment_step"):
            return
    raise AssertionError("round did not terminate")


@pytest.mark.parametrize("n,dynamic", [(12, False), (20, True), (100, True)])
def test_round_pool_matches_oracle_rows(n, dynamic, B=6, K=40):
    """RoundLoop with the pool on, the oracle envs in lockstep under the device's own actions: per env and merged, the pool
    equals numpy over every oracle ``pz.step`` info row that holds stats."""
    from melissa_amd import _lib as L
    from melissa_amd.collect import RoundLoop, sample_episode_table
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from oracle import env_oracle as eo
    seed = 77
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=dynamic, device="cuda", max_moves=48,
                             construct_like_reference=False)
    venv.enable_step_stats()
    net, _sd = make_ldgn(n)
    packed, table = sample_episode_table(venv, 14, seed)        # (the oracle env consumes two samplings while constructed)
    loop = RoundLoop(venv, DQNPolicy(net), eps=0.0, seed=seed, episodes=(dict(packed), np.ascontiguousarray(table[:, 1:])))
    assert venv.read_step_stats() == (0, {})                    # the reset and the `first` launch are no samples
    refs = []
    for b in range(B):
        env = eo.OracleGraphEnv(n, graph_pool=[eo.GraphSpec(g.pos.copy(), set_ints(g.one_hop)) for g in graphs],
                                dynamic_graph=dynamic,
                                np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b))))
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count = env, n, [0] * n, 0
        env.last()
        refs.append(pz)
    rows = [[] for _ in range(B)]
    took = dict(ff1=0, ff2=0, episodes=0)
    for it in range(K):
        live = loop.live.cpu().numpy().view(np.uint64).copy()
        loop.step()
        torch.cuda.synchronize()
        offsets, act = loop.offsets.cpu().numpy(), loop.act.cpu().numpy()
        for b, pz in enumerate(refs):
            mine = set_int(live[b])
            assert mine == pz.env.sel_active, (it, b)
            acts = {a: act[offsets[b] + k] for k, a in enumerate(a for a in range(n) if (mine >> a) & 1)}
            oracle_round_with_rows(pz, acts, mine, rows[b], took)
    sc = venv.scalars().cpu().numpy()
    assert int(np.bitwise_or.reduce(sc[:, L.S_ERROR])) == 0
    for b, pz in enumerate(refs):                               # still in lockstep at the end
        assert int(sc[b, L.S_SELECTION]) == pz.env.agent_selection and int(sc[b, L.S_NUM_MOVES]) == pz.env.num_moves
    print(f"N={n}: {took}, {sum(len(r) for r in rows)} oracle steps")
    assert took["episodes"] >= 3 and took["episodes"] == int(sc[:, L.S_EPISODES_DONE].sum())
    assert took["ff1"] >= 1 and took["ff2"] >= 1
    per_env = venv.read_step_stats(per_env=True)
    for b in range(B):
        assert_pool_equals_numpy(*pool_of_row(per_env[b]), [r for r in rows[b] if r is not None], f"N={n} env {b}")
    everything = [r for b in range(B) for r in rows[b] if r is not None]
    # (at N = 100 the six envs pool about 1.05e4 rows in 40 rounds, past the 2^13 of the bound's derivation: same 1e-12 kept)
    assert_pool_equals_numpy(*venv.read_step_stats(), everything, f"N={n} device merge", max_rows=None)
    assert_pool_equals_numpy(*venv.read_step_stats(on_host=True), everything, f"N={n} host merge", max_rows=None)


def run_rounds(n, B, rounds, pool_on, use_graph, eps=0.05):
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.replay import RoundReplay
    venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 4, first_seed=5), dynamic_graph=True, device="cuda",
                             max_moves=48, construct_like_reference=False)
    venv.enable_episode_log(256)
    if pool_on:
        venv.enable_step_stats()
    net, _ = make_ldgn(n)
    replay_buf = RoundReplay(B, n, 8, "cuda")
    loop = RoundLoop(venv, DQNPolicy(net), episodes_per_env=10, seed=3, eps=eps, use_graph=use_graph, replay=replay_buf)
    loop.run(rounds)
    torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0
    return venv, loop, replay_buf


def test_pool_is_bit_identical_under_graph_replay():
    eager, _, _ = run_rounds(20, 16, 30, True, False)
    graph, loop, _ = run_rounds(20, 16, 30, True, True)
    assert loop.graph is not None and loop.group_graph is not None
    a, b = eager.read_step_stats(per_env=True), graph.read_step_stats(per_env=True)
    assert a.shape == (16, 41) and (a[:, 0] > 0).all()
    np.testing.assert_array_equal(a, b)
    assert eager.read_step_stats() == graph.read_step_stats()


def test_off_means_off():
    """With the pool enabled, env state, episode log and replay records are bit-identical to a run without it."""
    off, loop_off, rp_off = run_rounds(20, 16, 20, False, False)
    on, loop_on, rp_on = run_rounds(20, 16, 20, True, False)
    assert getattr(off, "step_stats", None) is None and not off.env.step_stats
    assert on.read_step_stats()[0] > 0
    np.testing.assert_array_equal(off.state.cpu().numpy(), on.state.cpu().numpy())
    assert loop_off.counters() == loop_on.counters() and loop_on.counters()["episodes"] > 0
    # (envs whose episodes end in the same launch claim their log rows in whatever order their wavefronts run: compared per
    # env, where the order is the order the episodes ended in)
    (stats_a, meta_a, total_a), (stats_b, meta_b, total_b) = off.read_episode_log(), on.read_episode_log()
    order_a, order_b = np.argsort(meta_a[:, 0], kind="stable"), np.argsort(meta_b[:, 0], kind="stable")
    assert total_a == total_b == len(stats_a) > 0
    np.testing.assert_array_equal(meta_a[order_a], meta_b[order_b])
    np.testing.assert_array_equal(stats_a[order_a], stats_b[order_b])
    for name in ("obs", "obs_next", "acted", "done", "act", "rew", "episode", "cursor"):
        np.testing.assert_array_equal(getattr(rp_off, name).cpu().numpy(), getattr(rp_on, name).cpu().numpy())
    with pytest.raises(RuntimeError, match="enable_step_stats"):
        off.read_step_stats()


def episode_rows(result) -> np.ndarray:
    """The per-episode rows of a collect result (lens | episode_info in key order) in a canonical order: sorted."""
    rows = np.column_stack([np.asarray(result.lens, dtype=np.float64)] + [np.asarray(result.episode_info[k]) for k in LOGGER_KEYS])
    return rows[np.lexsort(rows.T[::-1])] if len(rows) else rows.reshape(0, 1 + len(LOGGER_KEYS))


def test_collectors_pool_steps():
    """``MultiAgentCollector(..., stats="steps")``: ``info`` is there before any episode has ended, every collect reports its
    own rows only, and the default collector returns what it did."""
    from melissa_amd.collect import CollectiveExperienceCollector, DictOfSequenceSummaryStats, MultiAgentCollector
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    n, B = 12, 4
    net, _ = make_ldgn(n)
    policy = DQNPolicy(net)

    def make(cls=MultiAgentCollector, **kw):
        venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 3, first_seed=50), dynamic_graph=True, device="cuda",
                                 max_moves=48, seed=11, construct_like_reference=False)
        return cls(n, policy=policy, env=venv, chunk=1, seed=4, **kw)

    steps, default, twin = make(stats="steps"), make(), make(stats="steps")
    assert default.stats == "episodes" and getattr(default.venv, "step_stats", None) is None
    results = []
    for kw in (dict(n_step=30), dict(n_step=30), dict(n_episode=3)):
        s, d = steps.collect(**kw), default.collect(**kw)
        results.append(s)
        # the default collector's result is what it was: info summarises the episodes' final rows; and both collectors walked
        # the same trajectory
        assert d.n_collected_steps == s.n_collected_steps and d.n_collected_episodes == s.n_collected_episodes
        assert d.info.stats == DictOfSequenceSummaryStats.from_dict(d.episode_info).stats
        assert d.n_info_rows == len(d.returns)
        # Episodes that end in the same launch claim their log rows (atomicAdd on the log cursor) in whatever order their
        # wavefronts get there, and the two collectors run different instantiations of the round kernel: the rows are the same
        # SET, their order need not be.  Compared as sorted rows (length | the ten values), never position by position.
        np.testing.assert_array_equal(episode_rows(d), episode_rows(s))
        assert episode_rows(d).shape == (len(d.returns), 1 + len(LOGGER_KEYS))
        np.testing.assert_array_equal(np.sort(d.returns), np.sort(s.returns))
    first, second, third = results
    print(f"collect 1: {first.n_collected_steps} steps {first.n_collected_episodes} episodes {first.n_info_rows} rows; "
          f"collect 2: {second.n_info_rows} rows; collect 3: {third.n_info_rows} rows")
    # 30 decisions of 4 envs are collected within three rounds: no episode has ended, the episode rows are empty ...
    assert first.n_collected_episodes == 0 and len(first.returns) == 0
    # ... and the step pool is not
    assert first.n_info_rows > 0 and list(first.info.stats) == list(LOGGER_KEYS)
    assert 0.0 < first.info.stats["coverage"].mean <= 1.0 and first["coverage"] == first.info.stats["coverage"].mean
    assert second.n_info_rows > 0 and third.n_info_rows > 0 and third.n_collected_episodes >= 3
    # every collect reports its own rows: a twin that plays the same rounds without emptying its pool holds the sum
    twin.venv.step_stats.zero_()
    twin.loop.run(steps.loop.iterations - twin.loop.iterations)
    total, pooled = twin.venv.read_step_stats()
    assert total == first.n_info_rows + second.n_info_rows + third.n_info_rows
    assert steps.venv.read_step_stats()[0] == third.n_info_rows
    assert pooled["coverage"].max >= third.info.stats["coverage"].max
    col = make(CollectiveExperienceCollector, stats="steps")
    res = col.collect(n_step=10)
    assert col.stats == "steps" and res.n_info_rows > 0 and list(res.info.stats) == list(LOGGER_KEYS)
    with pytest.raises(ValueError, match="episodes"):
        make(stats="rows")


def test_reset_flag_empties_the_pool_in_the_reading_launch():
    venv, loop, _ = run_rounds(12, 5, 6, True, False)
    before = venv.read_step_stats(per_env=True)
    count, stats = venv.read_step_stats(reset=True)
    assert count == int(before[:, 0].sum()) > 0 and list(stats) == list(LOGGER_KEYS)
    assert not venv.step_stats.cpu().numpy().any()
    assert venv.read_step_stats() == (0, {})
    loop.run(2)
    again, _ = venv.read_step_stats()
    assert 0 < again < count


TRAIN_QUIET = dict(model="hl_dgn", n_nodes=12, envs=8, batch_size=16, rounds_per_update=2, capture_updates=False,
                   log=lambda *_: None)


def test_train_collect_stats_steps_epoch_records(tmp_path):
    """``train --collect-stats steps``, epoch mode: every epoch record holds the rows pooled since the previous record (epoch
    0: the pre-fill rounds), read and emptied before that record's evaluation.  (The fixed-updates mode hands the same
    ``pooled()`` dict to its result once; the default result's key set is pinned by tests/test_gpu_eps_schedule.py.)"""
    from melissa_amd.train import train
    out = train(epoch=1, step_per_epoch=100, test_num=1, collect_stats="steps", logdir=str(tmp_path), **TRAIN_QUIET)
    assert [r["epoch"] for r in out["epochs"]] == [0, 1] and "train_info_rows" not in out
    for rec in out["epochs"]:
        assert rec["train_info_rows"] > 0 and 0.0 < rec["train_coverage"] <= 1.0


def test_watch_collect_stats_steps():
    from melissa_amd.watch import watch
    got = watch(model="l_dgn", n_nodes=12, envs=2, episodes=2, collect_stats="steps")
    assert got["n_info_rows"] > got["n/ep"] >= 2 and 0.0 < got["coverage"] <= 1.0
