"""GPU checks of the per-round recorder (csrc/round_record.hpp, melissa_amd/round_record.py): the device's accumulators, carry and
trace records against the NumPy model of the sampling rules (tests/round_record_ref.py) fed with the env state after every round -
bit for bit -, against the oracle env's trajectory, from replayed HIP graphs, under a quota (``evaluate_spread``), past
``max_rounds``, round a small trace ring, and through ``watch``."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.round_record_ref import RoundRecordModel, state_of
from tests.test_gpu_round import make_ldgn, oracle_round
from tests.test_round_record_ref import test_abi_sizeof_and_argument_errors  # noqa: F401  (runs here too)
from tests.trace_replay import set_int, set_ints

SEED = 9
TRACE_KEYS = ("meta", "pos", "one_hop", "sets", "agent_msgs", "received")


@functools.lru_cache(maxsize=None)
def _policy(n):
    from melissa_amd.policy import DQNPolicy
    return DQNPolicy(make_ldgn(n)[0])


def _venv(n, B, **kw):
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    return HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 3, first_seed=50), dynamic_graph=True, device="cuda",
                             max_moves=48, seed=SEED, construct_like_reference=False, **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def device_state(rec):
    out = dict(running=rec.running, ended=rec.ended, carry=rec.carry, last=rec.last, overflow=rec.overflow, skipped=rec.skipped,
               unlogged=rec.unlogged)
    if rec.trace_envs:
        out.update(cursor=rec.trace_cursor, **{k: getattr(rec, "trace_" + k) for k in TRACE_KEYS})
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def model_state(model):
    out = dict(running=model.running, ended=model.ended, carry=model.carry, last=model.last, overflow=model.overflow,
               skipped=model.skipped, unlogged=model.unlogged)
    if model.trace_envs:
        out.update(cursor=model.cursor, **model.ring)
    return out


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        g, w = bits(got[k]), bits(np.asarray(want[k]))
        if k in ("one_hop", "sets"):
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=k)


def assert_clean(rec):
    _run, _end, counters = rec.curves()
    assert counters == dict(overflow=0, skipped=0, unlogged=0)
    assert rec.drain_traces()[1] == 0


def play(n, B, rounds, trace_envs=(), trace_capacity=64, max_rounds=None, use_graph=False, graph_rounds=1, eps=0.05, double=False):
    """An eager (or graph-replayed) round loop with a recorder, and the model fed with the env state after every round."""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.round_record import RoundRecorder
    venv = _venv(n, B)
    rec = RoundRecorder(venv, max_rounds=max_rounds, trace_envs=trace_envs, trace_capacity=trace_capacity)
    model = None
    if not use_graph:
        model = RoundRecordModel(B, n, rec.max_rounds, trace_envs=trace_envs, trace_capacity=trace_capacity)
    loop = RoundLoop(venv, _policy(n), episodes_per_env=12, seed=3, eps=eps, use_graph=use_graph, graph_rounds=graph_rounds,
                     recorder=rec, episode_stream=False)
    if use_graph:
        loop.run(2)
        loop.run(rounds - 2)
        torch.cuda.synchronize()
    else:
        model.launch(state_of(venv))                     # the launch behind the constructor's `first` launch: round 0
        for _ in range(rounds):
            loop.step()
            if double:
                rec.launch()
            model.launch(state_of(venv))
    assert loop.counters()["errors"] == 0
    return venv, rec, model, loop


@pytest.mark.parametrize("n,B,traced", [(20, 5, (0, 4)), (70, 2, (1,))])
def test_eager_rounds_equal_the_model_bit_for_bit(n, B, traced):
    """5 envs: the second workgroup holds one env only; 70 nodes: two-word node sets, two nodes per lane."""
    venv, rec, model, loop = play(n, B, 40, trace_envs=traced)
    got = device_state(rec)
    assert_same(got, model_state(model))
    np.testing.assert_array_equal(rec.seen.cpu().numpy(), model.seen)
    assert got["ended"][:, :, 0].sum() >= B and (got["running"][:, 0, 0] >= 2).all()        # episodes ended in every env
    assert got["cursor"].min() == 41                     # round 0 and one record per round
    run, end, counters = rec.curves()
    want_run, want_end, want_counters = model.folded()
    np.testing.assert_array_equal(bits(run), bits(want_run))
    np.testing.assert_array_equal(bits(end), bits(want_end))
    assert counters == want_counters == dict(overflow=0, skipped=0, unlogged=0)
    traces, lost = rec.drain_traces()
    assert lost == 0 and sorted(traces) == sorted(traced)
    from melissa_amd.round_record import group_episodes
    for env in traced:
        want = group_episodes(model.all_records[env])
        assert [e["ordinal"] for e in traces[env]] == [e["ordinal"] for e in want] and len(want) >= 2
        for mine, theirs in zip(traces[env], want):
            assert mine["env"] == env and (mine["rounds"] == np.arange(len(mine["rounds"]))).all()
            for k in ("pos", "one_hop", "sets", "agent_msgs", "received", "world_msgs"):
                np.testing.assert_array_equal(bits(mine[k]), bits(theirs[k]), err_msg=k)


def test_doubled_launch_changes_nothing():
    venv, rec, model, loop = play(20, 3, 12, trace_envs=(1,), double=True)
    assert_same(device_state(rec), model_state(model))
    before = device_state(rec)
    rec.launch(), rec.launch()
    torch.cuda.synchronize()
    assert_same(device_state(rec), before)
    assert_clean(rec)


def test_graph_replays_give_the_eager_accumulators():
    """The one-round graph and the four-round group graph (7 group replays + 2 single rounds here) against eager launches."""
    finals = []
    for use_graph, graph_rounds in ((False, 1), (True, 1), (True, 4)):
        venv, rec, _model, loop = play(20, 5, 32, trace_envs=(0, 4), use_graph=use_graph, graph_rounds=graph_rounds)
        assert (loop.group_graph is not None) == (graph_rounds == 4)
        finals.append(device_state(rec))
        assert_clean(rec)
    assert finals[0]["ended"][:, :, 0].sum() >= 5
    for other in finals[1:]:
        assert_same(other, finals[0])


def test_oracle_trajectory_gives_the_same_accumulators():
    """The oracle env (pinned to the real reference by the golden traces) plays the device's actions; its states, fed through the
    model, must give the device's accumulators - episodes and actions shared as in tests/test_gpu_round.py."""
    from melissa_amd import _lib as L
    from melissa_amd.collect import RoundLoop, sample_episode_table
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.round_record import RoundRecorder
    from oracle import env_oracle as eo
    from tests.round_record_ref import pack_set
    n, B, K, seed = 20, 5, 30, 77
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=48, construct_like_reference=False)
    packed, table = sample_episode_table(venv, 14, seed)
    rec = RoundRecorder(venv)
    loop = RoundLoop(venv, _policy(n), eps=0.0, seed=seed, recorder=rec,
                     episodes=({k: v for k, v in packed.items()}, np.ascontiguousarray(table[:, 1:])))
    refs = []
    for b in range(B):
        env = eo.OracleGraphEnv(n, graph_pool=[eo.GraphSpec(g.pos.copy(), set_ints(g.one_hop)) for g in graphs],
                                dynamic_graph=True, np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b))))
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count = env, n, [0] * n, 0
        env.last()
        refs.append(pz)

    olog = []                                            # the oracle's episode log: (env, final logger_stats, num_moves)

    def oracle_state():
        member = lambda m: pack_set([(m >> i) & 1 for i in range(n)])
        sc = np.zeros((B, 16), dtype=np.int32)
        ns, ss = np.zeros((B, 8, 1), dtype=np.uint64), np.zeros((B, 4, 1), dtype=np.uint64)
        for b, pz in enumerate(refs):
            e = pz.env
            sc[b, L.S_EPISODES_DONE], sc[b, L.S_NUM_MOVES] = len(getattr(pz, "finished", [])), e.num_moves
            sc[b, L.S_WORLD_MSGS], sc[b, L.S_ORIGIN] = e.messages_transmitted, e.origin_agent
            ns[b, L.SET_HAS_MESSAGE], ns[b, L.SET_ORIGIN] = member(e.has_message), member(e.message_origin)
            ns[b, L.SET_INTERESTED], ns[b, L.SET_SCRIPTED] = member(e.interested), member(e.scripted)
            ss[b, 0], ss[b, 3] = member(e.sel_active), member(e.has_taken_action)
        return dict(scalars=sc, node_sets=ns, sel_sets=ss, pos=np.stack([np.asarray(pz.env.pos, dtype=np.float64) for pz in refs]),
                    one_hop=np.stack([np.stack([member(m) for m in pz.env.adj]) for pz in refs]),
                    agent_msgs=np.array([pz.env.agent_msgs for pz in refs], dtype=np.int32),
                    received=np.array([pz.env.received_count for pz in refs], dtype=np.int32),
                    log_cursor=len(olog), log_capacity=int(venv.env.log_capacity),
                    log_stats=np.array([[float(s[k]) for k in L.LOGGER_KEYS] for _b, s, _m in olog], dtype=np.float64).reshape(-1, 10),
                    log_meta=np.array([[b_, 0, m] for b_, _s, m in olog], dtype=np.int32).reshape(-1, 3))

    model = RoundRecordModel(B, n, rec.max_rounds)
    model.launch(oracle_state())
    late = 0
    for _ in range(K):
        live = loop.live.cpu().numpy().view(np.uint64).copy()
        loop.step()
        torch.cuda.synchronize()
        offsets, act = loop.offsets.cpu().numpy(), loop.act.cpu().numpy()
        for b, pz in enumerate(refs):
            acts = {a: act[offsets[b] + k] for k, a in enumerate(a for a in range(n) if (set_int(live[b]) >> a) & 1)}
            before, moves = len(getattr(pz, "finished", [])), pz.env.num_moves
            oracle_round(pz, acts)
            olog.extend((b, s, m) for s, m in getattr(pz, "finished", [])[before:])
            late += sum(m != moves for _s, m in getattr(pz, "finished", [])[before:])
        model.launch(oracle_state())
    assert loop.counters()["errors"] == 0
    got = device_state(rec)
    assert_same(got, model_state(model))
    assert got["ended"][:, :, 0].sum() >= B
    # the case the episode log is there for: an episode that ended in the launch of its last world step
    print(f"{len(olog)} episodes ended, {late} of them in the launch of their last world step")
    assert late >= 1 and len(olog) >= B
    assert_clean(rec)


def test_quota_keeps_the_surplus_episodes_of_a_spread_evaluation_out():
    from melissa_amd import _lib as L
    from melissa_amd.collect import evaluate_spread, test_shares
    from melissa_amd.round_record import RoundRecorder, summarise
    n, B, T = 12, 3, 7
    venv = _venv(n, B, is_testing=True, num_test_episodes=T, spread_test_episodes=True)
    rec = RoundRecorder(venv, trace_envs=(0,), trace_capacity=64)
    res, _positions = evaluate_spread(_policy(n), venv, T, eps=0.0, seed=SEED, use_graph=True, recorder=rec)
    shares = test_shares(T, B)
    assert shares == [3, 2, 2]
    run, end, counters = rec.curves()
    assert counters == dict(overflow=0, skipped=0, unlogged=0)
    assert run[0, 0] == T and end[:, 0].sum() == T
    ended = rec.ended.cpu().numpy()
    stats, meta, total = venv.read_episode_log()
    # there WERE surplus episodes to keep out: every env went on into the episode after its share, and the recorder saw it
    assert (rec.seen[:, 0].cpu().numpy() >= np.asarray(shares)).all() and total >= T
    R = rec.max_rounds
    used = 0
    for b in range(B):
        mine = np.flatnonzero(meta[:, 0] == b)[:shares[b]]              # the env's counted rows, in play order
        assert len(mine) == shares[b]
        want = np.zeros((R, 2))
        for k in mine:                                   # the device adds an env's rows in play order, round by round
            want[meta[k, 2]] += (stats[k, L.LOGGER_KEYS.index("total_messages_transmitted")],
                                 stats[k, L.LOGGER_KEYS.index("coverage_interested_fraction")])
            used += 1
        np.testing.assert_array_equal(bits(ended[b][:, L.RR_MESSAGES]), bits(want[:, 0]))
        np.testing.assert_array_equal(bits(ended[b][:, L.RR_COVERAGE_FRACTION]), bits(want[:, 1]))
        tot_msgs = tot_frac = dev_msgs = dev_frac = 0.0
        for r in range(R):
            tot_msgs, tot_frac = tot_msgs + want[r, 0], tot_frac + want[r, 1]
            dev_msgs, dev_frac = dev_msgs + ended[b][r, L.RR_MESSAGES], dev_frac + ended[b][r, L.RR_COVERAGE_FRACTION]
        assert (dev_msgs, dev_frac) == (tot_msgs, tot_frac)
        assert ended[b][:, 0].sum() == shares[b] and rec.running[b, 0, 0].item() == shares[b]
    assert used == T
    s = summarise(run, end, n_nodes=n)
    assert s["episodes"] == T and (s["carried_count"] == T).all()
    assert s["messages"][-1] == pytest.approx(float(np.mean(res.episode_info["total_messages_transmitted"])))
    traces, lost = rec.drain_traces()
    assert lost == 0 and [e["ordinal"] for e in traces[0]] == list(range(shares[0]))
    # a trace ends at the episode's last round, or one before it where that round's launch also reset the env
    for e, moves in zip(traces[0], meta[np.flatnonzero(meta[:, 0] == 0)[:shares[0]], 2].tolist()):
        assert len(e["rounds"]) - 1 in (moves, moves - 1)
    with pytest.raises(ValueError, match="trace_capacity"):
        evaluate_spread(_policy(n), venv, T, recorder=RoundRecorder(venv, trace_envs=(0,), trace_capacity=15), chunk=8)


def test_rounds_past_max_rounds_overflow_and_touch_nothing_else():
    from melissa_amd.collect import RoundLoop
    from melissa_amd.round_record import RoundRecorder
    n, B, guard = 12, 3, 4096
    venv = _venv(n, B)
    rec = RoundRecorder(venv, max_rounds=3, trace_envs=(2,), trace_capacity=4)
    rec.set_quota([1000] * B)
    names = dict(running="running", ended="ended", carry="seen", last="last", overflow="overflow", skipped="skipped",
                 unlogged="unlogged", quota="quota",
                 trace_cursor="trace_cursor", trace_meta="trace_meta", trace_pos="trace_pos", trace_one_hop="trace_one_hop",
                 trace_sets="trace_sets", trace_agent_msgs="trace_agent_msgs", trace_received="trace_received", _out=None,
                 _counters=None)
    homes = {}
    for attr, field in names.items():                    # every buffer moves between two sentinel pages
        t = getattr(rec, attr)
        nbytes = t.numel() * t.element_size()
        home = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        inner = home[guard:guard + nbytes].view(t.dtype).view(t.shape)
        inner.copy_(t)
        setattr(rec, attr, inner)
        if field is not None:                            # (the read launch's outputs are arguments, not struct fields)
            setattr(rec.c, field, inner.data_ptr())
        homes[attr] = (home, nbytes)
    model = RoundRecordModel(B, n, 3, trace_envs=(2,), trace_capacity=4, quota=[1000] * B)
    loop = RoundLoop(venv, _policy(n), episodes_per_env=12, seed=3, eps=0.05, use_graph=False, recorder=rec, episode_stream=False)
    model.launch(state_of(venv))
    for _ in range(25):
        loop.step()
        model.launch(state_of(venv))
    assert loop.counters()["errors"] == 0
    assert_same(device_state(rec), model_state(model))
    _run, _end, counters = rec.curves()
    assert counters["overflow"] == int(model.overflow.sum()) > 0 and counters["skipped"] == 0 and counters["unlogged"] == 0
    for attr, (home, nbytes) in homes.items():
        h = home.cpu().numpy()
        assert (h[:guard] == 0xA5).all() and (h[guard + nbytes:] == 0xA5).all(), attr


def test_trace_ring_wraps_in_order_and_reports_what_it_lost():
    from melissa_amd.collect import RoundLoop
    from melissa_amd.round_record import RoundRecorder, group_episodes
    n, B = 12, 3
    venv = _venv(n, B)
    rec = RoundRecorder(venv, trace_envs=(1,), trace_capacity=4)
    model = RoundRecordModel(B, n, rec.max_rounds, trace_envs=(1,), trace_capacity=4)
    loop = RoundLoop(venv, _policy(n), episodes_per_env=12, seed=3, eps=0.05, use_graph=False, recorder=rec, episode_stream=False)
    model.launch(state_of(venv))
    for it in range(14):
        loop.step()
        model.launch(state_of(venv))
        if it % 2 == 1:                                  # a drain every 2 rounds: at most 3 records between two drains
            assert rec.drain_traces()[1] == 0
    traces, lost = rec.drain_traces()
    assert lost == 0 and len(rec.records[1]) == len(model.all_records[1]) == 15
    for mine, theirs in zip(rec.records[1], model.all_records[1]):
        for k in TRACE_KEYS:
            np.testing.assert_array_equal(bits(mine[k]), bits(theirs[k]), err_msg=k)
    assert [e["ordinal"] for e in traces[1]] == [e["ordinal"] for e in group_episodes(model.all_records[1])]
    for _ in range(7):                                   # the drain withheld: 7 records into a ring of 4
        loop.step()
        model.launch(state_of(venv))
    traces, lost = rec.drain_traces()
    assert lost == 3 and len(rec.records[1]) == 15 + 4
    for mine, theirs in zip(rec.records[1][15:], model.all_records[1][18:]):
        np.testing.assert_array_equal(mine["meta"], theirs["meta"])
    _run, _end, counters = rec.curves()
    assert counters == dict(overflow=0, skipped=0, unlogged=0) and loop.counters()["errors"] == 0


def test_watch_writes_curves_traces_and_frames(tmp_path):
    import xml.etree.ElementTree as ET
    from melissa_amd.watch import watch
    kw = dict(model="l_dgn", n_nodes=20, envs=3, episodes=5, seed=SEED, spread=True, graphs=4)
    plain = watch(**kw)
    curves, trace, frames = tmp_path / "curves.json", tmp_path / "trace.npz", tmp_path / "frames"
    out = watch(**kw, curves_out=str(curves), trace_out=str(trace), trace_envs=2, render_out=str(frames))
    timing = ("collect_time", "collect_speed")           # wall-clock figures: the only keys that may differ
    assert out.keys() == plain.keys()
    assert {k: v for k, v in out.items() if k not in timing} == {k: v for k, v in plain.items() if k not in timing}
    doc = json.loads(curves.read_text())
    assert doc["episodes"] == 5 and doc["counters"] == dict(overflow=0, skipped=0, unlogged=0, lost_trace_records=0)
    assert doc["running"][0] == 5 and len(doc["coverage"]) == 65 and doc["messages"][-1] == pytest.approx(out["total_messages_transmitted"])
    assert doc["coverage_interested_fraction"][-1] == pytest.approx(out["coverage_interested_fraction"])
    saved = np.load(str(trace))
    episodes = sorted({k.rsplit("_", 1)[0] for k in saved.files if k.endswith("_rounds")})
    assert episodes == ["e0_o0", "e0_o1", "e1_o0", "e1_o1"]             # shares [2, 2, 1]: envs 0 and 1 traced
    svgs = sorted(os.listdir(frames))
    assert len(svgs) == sum(len(saved[e + "_rounds"]) for e in episodes)
    root = ET.parse(str(frames / svgs[0])).getroot()
    assert len(root.findall("{http://www.w3.org/2000/svg}circle")) == 20
    with pytest.raises(ValueError, match="spread"):
        watch(model="l_dgn", n_nodes=20, envs=1, episodes=2, curves_out=str(curves))
