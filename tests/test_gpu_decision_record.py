"""GPU checks of the decision recorder (csrc/decision_record.hpp, melissa_amd/decision_record.py): the device's tables, counters
and trace records against the NumPy model of the booking rules (tests/decision_record_ref.py) - bit for bit - on hand-built
launches over a real env batch and inside the round loop (both row layouts), from replayed HIP graphs, under a quota
(``evaluate_spread``), through ``watch``; and that a loop without the recorder is the loop it was."""
import functools
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from melissa_amd import _lib as L
from tests.decision_record_ref import DecisionRecordModel, members, pack, state_of
from tests.test_decision_record_ref import test_abi_sizeof_and_argument_errors  # noqa: F401  (runs here too)

SEED = 9
ROUNDS = 24
INT_FIELDS, FLOAT_FIELDS = [0, 1, 6, 7], [2, 3, 4, 5]


@functools.lru_cache(maxsize=None)
def _policy(model, n):
    from melissa_amd.policy import DQNPolicy
    from tests.test_gpu_forward import make_net
    return DQNPolicy(make_net(model, n, 9)[0])


def _venv(n, B, **kw):
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    return HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 3, first_seed=50), dynamic_graph=True, device="cuda",
                             max_moves=48, seed=SEED, construct_like_reference=False, **kw)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32, np.dtype(np.int64): np.uint64}.get(a.dtype, a.dtype))


def device_state(rec):
    out = dict(by_round=rec.by_round, by_degree=rec.by_degree, overflow=rec.overflow, skipped=rec.skipped)
    if rec.trace_envs:
        out.update(cursor=rec.trace_cursor, meta=rec.trace_meta, sets=rec.trace_sets, q=rec.trace_q)
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def model_state(model):
    out = dict(by_round=model.by_round, by_degree=model.by_degree, overflow=model.overflow, skipped=model.skipped)
    if model.trace_envs:
        out.update(cursor=model.cursor, **model.ring)
    return out


def assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        g, w = bits(got[k]), bits(np.asarray(want[k]))
        np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=k)


def assert_tables_equal_model(rec, model):
    by_round, by_degree, counters = rec.tables()
    want_round, want_degree, want_counters = model.folded()
    np.testing.assert_array_equal(bits(by_round), bits(want_round))
    np.testing.assert_array_equal(bits(by_degree), bits(want_degree))
    assert counters == want_counters
    return by_round, by_degree, counters


def guard_buffers(rec, guard=4096):
    """Every buffer of the recorder moves between two sentinel pages -> {attr: (home, nbytes)}."""
    names = dict(by_round="by_round", by_degree="by_degree", overflow="overflow", skipped="skipped", quota="quota",
                 trace_cursor="trace_cursor", trace_meta="trace_meta", trace_sets="trace_sets", trace_q="trace_q",
                 _out_round=None, _out_degree=None, _counters=None)
    homes = {}
    for attr, field in names.items():
        t = getattr(rec, attr)
        nbytes = t.numel() * t.element_size()
        home = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
        inner = home[guard:guard + nbytes].view(t.dtype).view(t.shape)
        inner.copy_(t)
        setattr(rec, attr, inner)
        if field is not None and (field != "quota" or rec.c.quota):   # (the read launch's outputs are arguments, not struct fields)
            setattr(rec.c, field, inner.data_ptr())
        homes[attr] = (home, nbytes, guard)
    return homes


def assert_guards_untouched(homes):
    for attr, (home, nbytes, guard) in homes.items():
        h = home.cpu().numpy()
        assert (h[:guard] == 0xA5).all() and (h[guard + nbytes:] == 0xA5).all(), attr


def played_venv(n, B, rounds=3, **kw):
    """A real env batch after a few rounds of the L-DGN loop."""
    from melissa_amd.collect import RoundLoop
    venv = _venv(n, B, **kw)
    loop = RoundLoop(venv, _policy("l_dgn", n), seed=3, eps=0.05, use_graph=False)
    loop.run(rounds)
    torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0
    return venv, loop


def live_cases(n):
    cases = [[], [0], [n - 1], list(range(n))]
    return cases + [[63, 64, 69]] if n > 64 else cases


def hand_inputs(rng, n, B, lives, dense):
    """live / logits / act / row_offsets of one launch, on the host and on the device; one exact tie, one negative pair."""
    live = np.stack([pack(ids, n) for ids in lives])
    rows = B if dense else sum(len(ids) for ids in lives)
    logits = rng.standard_normal((rows + 2, 2)).astype(np.float32)
    logits[0], logits[1] = (0.375, 0.375), (-1.25, -0.5)
    act = rng.integers(0, 2, size=B * n if dense else rows + 2).astype(np.int32)
    offsets = None if dense else np.concatenate([[0], np.cumsum([len(ids) for ids in lives])]).astype(np.int32)
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    return (live, logits, act, offsets), (dev(logits), dev(act), dev(offsets), dev(live))


@pytest.mark.parametrize("dense", [False, True], ids=["rows", "dense"])
@pytest.mark.parametrize("n,B,scripted", [(12, 6, 0.0), (12, 6, 0.5), (70, 4, 0.0), (70, 4, 0.5)])
def test_hand_built_launches_equal_the_model_bit_for_bit(n, B, scripted, dense):
    """Every env meets every live set (empty, node 0, the highest node, the full set, beyond 64 nodes 63 + 64 + 69); then env 0
    stands at ``max_rounds``, env 1 in error and env 2 has met its quota, and they meet them again.  With ``scripted`` every env
    has scripted nodes, so the full sets (and some of the others) hold nodes that are not the policy's.  A ring of 4 records
    wraps.  Doubles as int64, guard pages round every buffer."""
    from melissa_amd.decision_record import DecisionRecorder
    kw = dict(scripted_agents_ratio=scripted, heuristic="simple_broadcast") if scripted else {}
    venv, _loop = played_venv(n, B, **kw)
    R, D, traced = 8, 4, (0, 2, B - 1)
    quota = [1000] * B
    rec = DecisionRecorder(venv, max_rounds=R, n_degrees=D, trace_envs=traced, trace_capacity=4, quota=quota)
    homes = guard_buffers(rec)
    model = DecisionRecordModel(B, n, R, D, trace_envs=traced, trace_capacity=4, quota=quota)
    rng, cases = np.random.default_rng(n + B), live_cases(n)
    sc = venv.scalars()
    for phase in range(2):
        if phase == 1:
            sc[0, L.S_NUM_MOVES] = R                                     # past the round table
            sc[1, L.S_ERROR] = 4
            quota[2] = int(sc[2, L.S_EPISODES_DONE].item())              # met
            rec.quota.copy_(torch.tensor(quota, dtype=torch.int32))
            model.quota = np.asarray(quota, dtype=np.int64)
        state = state_of(venv)
        for k in range(len(cases)):
            host, dev = hand_inputs(rng, n, B, [cases[(b + k) % len(cases)] for b in range(B)], dense)
            rec.launch(*dev)
            model.launch(state, *host)
    torch.cuda.synchronize()
    assert_same(device_state(rec), model_state(model))
    by_round, by_degree, counters = assert_tables_equal_model(rec, model)
    scripted_sets = state["node_sets"][:, L.SET_SCRIPTED]
    assert (scripted_sets.any(axis=1)).all() == bool(scripted)
    booked = sum(len([i for i in ids if i not in members(scripted_sets[b], n)]) for b in range(B) for ids in cases)
    assert booked > 0 and by_degree[:, 0].sum() == 2 * booked - sum(
        len([i for i in ids if i not in members(scripted_sets[b], n)]) for b in (1, 2) for ids in cases)
    assert counters["skipped"] == len(cases) and counters["overflow"] == by_degree[:, 0].sum() - by_round[:, 0].sum() > 0
    assert by_degree[D - 1, 0] > 0                                       # degrees past the table were clamped into its last row
    if not scripted:
        assert model.cursor.max() > 4                                    # the ring wrapped
    assert_guards_untouched(homes)


def test_a_second_launch_doubles_every_integer_field():
    from melissa_amd.decision_record import DecisionRecorder
    n, B = 12, 6
    venv, _loop = played_venv(n, B)
    sc = venv.scalars()
    sc[0, L.S_NUM_MOVES], sc[1, L.S_ERROR] = 8, 4
    rec = DecisionRecorder(venv, max_rounds=8, n_degrees=4, trace_envs=(3,), trace_capacity=4)
    model = DecisionRecordModel(B, n, 8, 4, trace_envs=(3,), trace_capacity=4)
    host, dev = hand_inputs(np.random.default_rng(1), n, B, [list(range(n))] * B, dense=False)
    state = state_of(venv)
    rec.launch(*dev)
    model.launch(state, *host)
    torch.cuda.synchronize()
    once = device_state(rec)
    assert_same(once, model_state(model))
    rec.launch(*dev)
    model.launch(state, *host)
    torch.cuda.synchronize()
    twice = device_state(rec)
    assert_same(twice, model_state(model))
    for k in ("by_round", "by_degree"):
        np.testing.assert_array_equal(twice[k][..., INT_FIELDS], 2 * once[k][..., INT_FIELDS], err_msg=k)
    assert once["by_degree"][..., 0].sum() == (B - 1) * n and once["by_round"][..., 0].sum() == (B - 2) * n
    for k in ("overflow", "skipped", "cursor"):
        np.testing.assert_array_equal(twice[k], 2 * once[k], err_msg=k)
    assert once["overflow"].tolist() == [n, 0, 0, 0, 0, 0] and once["skipped"].tolist() == [0, 1, 0, 0, 0, 0]
    np.testing.assert_array_equal(twice["meta"][0, 1], twice["meta"][0, 0])


def play(model_name, n, B, use_graph=False, graph_rounds=1, decisions=True, feed_model=False, eps=0.1):
    """``ROUNDS`` rounds of the round loop from one seed, with a recorder that traces every env; eager loops can feed the model."""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.decision_record import DecisionRecorder
    venv = _venv(n, B)
    rec = DecisionRecorder(venv, trace_envs=range(B), trace_capacity=64) if decisions else None
    model = DecisionRecordModel(B, n, rec.max_rounds, rec.n_degrees, trace_envs=range(B), trace_capacity=64) if feed_model else None
    loop = RoundLoop(venv, _policy(model_name, n), episodes_per_env=12, seed=3, eps=eps, use_graph=use_graph,
                     graph_rounds=graph_rounds, decisions=rec, episode_stream=False)
    before = venv.scalars()[:, L.S_DECISIONS].cpu().numpy().astype(np.int64)
    if feed_model:
        W = L.set_words(n)
        for _ in range(ROUNDS):
            live = loop.live.cpu().numpy().view(np.uint64).reshape(B, W).copy()
            state = state_of(venv)
            loop.run(1)
            torch.cuda.synchronize()
            model.launch(state, live, loop.logits.cpu().numpy(), loop.act.cpu().numpy(),
                         None if loop.per_env_logits else loop.offsets.cpu().numpy())
    else:
        loop.run(ROUNDS)
        torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0 and loop.iterations == ROUNDS
    grown = int((venv.scalars()[:, L.S_DECISIONS].cpu().numpy().astype(np.int64) - before).sum())
    return venv, rec, model, loop, grown


@functools.lru_cache(maxsize=None)
def eager(model_name, n, B):
    """The eager loop with the model fed round by round: played once, shared by the tests that read it (nothing changes it)."""
    venv, rec, model, loop, grown = play(model_name, n, B, feed_model=True)
    return rec, model, device_state(rec), (venv.state.cpu().numpy().copy(), loop.act.cpu().numpy().copy(),
                                           loop.logits.cpu().numpy().copy()), grown


LOOPS = [("l_dgn", 12, 6), ("hl_dgn", 12, 4)]


@pytest.mark.parametrize("model_name,n,B", LOOPS)
def test_the_loop_equals_the_model_bit_for_bit(model_name, n, B):
    from melissa_amd.decision_record import group_decision_episodes
    rec, model, got, _final, grown = eager(model_name, n, B)
    assert_same(got, model_state(model))
    by_round, by_degree, counters = assert_tables_equal_model(rec, model)
    assert counters == dict(overflow=0, skipped=0)
    # no scripted agents: every decision the env counted was the policy's
    print(f"{model_name}: {by_round[:, 0].sum():.0f} decisions booked, MEL_S_DECISIONS grew by {grown}")
    assert by_round[:, 0].sum() == grown > ROUNDS
    assert by_round[:, L.DR_NON_GREEDY].sum() > 0 and by_round[:, L.DR_FIRST].sum() > 0 and (by_round[:, 0] > 0).sum() > 3
    traces, lost = rec.drain_traces()
    assert lost == 0 and sorted(traces) == list(range(B))
    for env in range(B):
        want = group_decision_episodes(model.all_records[env])
        assert [e["ordinal"] for e in traces[env]] == [e["ordinal"] for e in want] and len(want) >= 1
        for mine, theirs in zip(traces[env], want):
            assert mine["env"] == env
            for k in ("rounds", "decisions", "relays", "sets", "q"):
                np.testing.assert_array_equal(bits(mine[k]), bits(theirs[k]), err_msg=k)


@pytest.mark.parametrize("model_name,n,B", LOOPS)
def test_captured_rounds_equal_eager_rounds(model_name, n, B):
    """One eager warm-up round, the one-round graph, then groups of four rounds from one graph - against eager launches."""
    _rec, _model, want, _final, _grown = eager(model_name, n, B)
    _venv_, rec, _m, loop, _g = play(model_name, n, B, use_graph=True, graph_rounds=4)
    assert loop.group_graph is not None
    assert_same(device_state(rec), want)
    assert rec.tables()[2] == dict(overflow=0, skipped=0) and rec.drain_traces()[1] == 0


@pytest.mark.parametrize("model_name,n,B", LOOPS)
def test_a_loop_without_the_recorder_is_the_loop_it_was(model_name, n, B):
    from melissa_amd.decision_record import DecisionRecorder
    _rec, _model, _got, final, grown = eager(model_name, n, B)
    calls = DecisionRecorder.launches
    assert calls >= ROUNDS                               # (the counter does count: the eager loop's launches)
    venv, rec, _m, loop, grown_plain = play(model_name, n, B, decisions=False)
    assert rec is None and loop.decisions is None
    assert DecisionRecorder.launches == calls            # the library's new entry points were never called
    assert grown_plain == grown
    for got, want, name in zip((venv.state, loop.act, loop.logits), final, ("env state", "act", "logits")):
        np.testing.assert_array_equal(bits(got.cpu().numpy()), bits(want), err_msg=name)


@pytest.mark.parametrize("model_name,n,B", LOOPS)
def test_the_two_tables_hold_the_same_totals(model_name, n, B):
    """Integer fields exactly; floating fields within ``len * 2**-52 * sum(|x|)`` of the model's addends - the two tables add
    the same numbers in different orders, and a sum of ``len`` doubles in any order is within ``(len - 1) * 2**-53 * sum(|x|)``
    of the exact one (to first order), so two orders differ by less than twice that."""
    rec, model, _got, _final, _grown = eager(model_name, n, B)
    by_round, by_degree, counters = rec.tables()
    assert counters["overflow"] == 0 and all(a[1] is not None for a in model.addends)
    rows = np.stack([a[3] for a in model.addends])
    for f in INT_FIELDS:
        assert by_round[:, f].sum() == by_degree[:, f].sum() == rows[:, f].sum(), f
    for f in FLOAT_FIELDS:
        bound = len(rows) * 2.0 ** -52 * np.abs(rows[:, f]).sum()
        diff = abs(by_round[:, f].sum() - by_degree[:, f].sum())
        print(f"field {f}: |by_round - by_degree| = {diff:.3e}, bound {bound:.3e}")
        assert diff <= bound, f


def _watch_setup(n, envs, episodes, seed):
    """The policy and env batch ``watch`` builds for these arguments."""
    from melissa_amd.env import HipGraphVectorEnv, connected_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network
    torch.manual_seed(seed)
    net = build_network("l_dgn", n, "cuda:0")
    policy = DQNPolicy(net, target_update_freq=1)
    net.eval()
    net.set_feature_dtype("f32")
    venv = HipGraphVectorEnv(envs, n, graph_pool=connected_graph_pool(n, 4, first_seed=0, device="cuda:0"), dynamic_graph=True,
                             device="cuda:0", max_moves=64, seed=seed, construct_like_reference=False, is_testing=True,
                             num_test_episodes=episodes, scripted_agents_ratio=0.0, heuristic=None, spread_test_episodes=True)
    return policy, venv


def test_spread_evaluation_counts_the_counted_episodes_only_and_watch_writes_them(tmp_path):
    from melissa_amd.collect import Collector, evaluate_spread, test_shares
    from melissa_amd.decision_record import DecisionRecorder, summarise_decisions
    from melissa_amd.watch import watch
    n, B, T = 12, 4, 10
    shares = np.asarray(test_shares(T, B))
    assert shares.tolist() == [3, 3, 2, 2]
    # the count, on the host: the same schedule stepped eagerly, the live sets of the envs that are inside their share
    policy, venv = _watch_setup(n, B, T, SEED)
    venv.scalars().zero_()
    col = Collector(policy, venv, seed=SEED, eps=0.0, chunk=8, use_graph=False, log_capacity=1024, episode_stream="test")
    counted = surplus = 0
    with torch.no_grad():
        for _ in range(400):
            done = venv.scalars()[:, L.S_EPISODES_DONE].cpu().numpy()
            if (done >= shares).all():
                break
            live = col.loop.live.cpu().numpy().view(np.uint64).reshape(B, -1)
            for b in range(B):
                k = len(members(live[b], n))
                counted, surplus = counted + (k if done[b] < shares[b] else 0), surplus + (k if done[b] >= shares[b] else 0)
            col.loop.step()
    assert (done >= shares).all() and surplus > 0        # there WERE surplus episodes to keep out
    # the evaluation itself, with the recorder
    policy, venv = _watch_setup(n, B, T, SEED)
    rec = DecisionRecorder(venv, trace_envs=range(2), trace_capacity=64)
    evaluate_spread(policy, venv, T, eps=0.0, seed=SEED, decisions=rec)
    by_round, by_degree, counters = rec.tables()
    print(f"{by_round[:, 0].sum():.0f} decisions booked, {counted} in the counted episodes, {surplus} in surplus ones")
    assert counters == dict(overflow=0, skipped=0)
    assert by_round[:, 0].sum() == by_degree[:, 0].sum() == counted
    assert by_round[:, L.DR_NON_GREEDY].sum() == 0       # eps = 0
    traces, lost = rec.drain_traces()
    assert lost == 0 and [[e["ordinal"] for e in traces[b]] for b in range(2)] == [[0, 1, 2], [0, 1, 2]]
    with pytest.raises(ValueError, match="trace_capacity"):
        evaluate_spread(policy, venv, T, decisions=DecisionRecorder(venv, trace_envs=(0,), trace_capacity=15), chunk=8)
    # watch: the same evaluation, into files
    kw = dict(model="l_dgn", n_nodes=n, envs=B, episodes=T, seed=SEED, spread=True, graphs=4)
    out_json, out_npz = tmp_path / "decisions.json", tmp_path / "decisions.npz"
    out = watch(**kw, decisions_out=str(out_json), decision_trace_out=str(out_npz), trace_envs=2)
    assert out["n/ep"] == T
    doc = json.loads(out_json.read_text())
    np.testing.assert_array_equal(bits(np.asarray(doc["by_round_sums"])), bits(by_round))
    np.testing.assert_array_equal(bits(np.asarray(doc["by_degree_sums"])), bits(by_degree))
    assert doc["counters"] == dict(overflow=0, skipped=0, lost_trace_records=0)
    s = summarise_decisions(by_round, by_degree)
    assert doc["total"]["decisions"] == counted and doc["total"]["relay_rate"] == s["total"]["relay_rate"]
    assert doc["by_round"]["relay_rate"][0] == s["by_round"]["relay_rate"][0] and None in doc["by_round"]["relay_rate"]
    saved = np.load(str(out_npz))
    assert sorted({k.rsplit("_", 1)[0] for k in saved.files if k.endswith("_rounds")}) == [f"e{b}_o{o}" for b in range(2) for o in range(3)]
    for b in range(2):
        for ep in traces[b]:
            for k in ("rounds", "decisions", "relays", "sets", "q"):
                np.testing.assert_array_equal(bits(saved[f"e{b}_o{ep['ordinal']}_{k}"]), bits(ep[k]), err_msg=k)
