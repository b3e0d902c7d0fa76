"""GPU checks of the attention recorder (csrc/attention_record.hpp, melissa_amd/attention_record.py): the device's tables,
counters and trace records against the NumPy model of the booking rules (tests/attention_record_ref.py) - bit for bit - on
hand-built launches over a real env batch and inside the round loop, from replayed HIP graphs, beside the other two recorders,
through ``evaluate_spread`` and ``watch``; and that a loop without the recorder is the loop it was."""
import functools
import json
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from melissa_amd import _lib as L
from tests import test_gpu_decision_record as DR
from tests import test_gpu_round_record as RR
from tests.attention_record_ref import MAX_SOURCES, AttentionRecordModel, members, pack, state_of

ROUNDS = 24
bits = DR.bits


def device_state(rec):
    out = dict(by_round=rec.by_round, by_degree=rec.by_degree, by_head=rec.by_head, overflow=rec.overflow, skipped=rec.skipped)
    if rec.trace_envs:
        out.update(cursor=rec.trace_cursor, meta=rec.trace_meta, sets=rec.trace_sets, fields=rec.trace_fields)
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def model_state(model):
    out = dict(by_round=model.by_round, by_degree=model.by_degree, by_head=model.by_head, overflow=model.overflow,
               skipped=model.skipped)
    if model.trace_envs:
        out.update(cursor=model.cursor, **model.ring)
    return out


def assert_tables_equal_model(rec, model):
    got, want = rec.tables(), model.folded()
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(bits(g), bits(w))
    assert got[3] == want[3]
    return got


def guarded(t, homes, name, guard=4096):
    """A copy of ``t`` between two sentinel pages, noted in ``homes``."""
    nbytes = t.numel() * t.element_size()
    home = torch.full((nbytes + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    inner = home[guard:guard + nbytes].view(t.dtype).view(t.shape)
    inner.copy_(t)
    homes.append((name, home, nbytes, guard))
    return inner


def guard_buffers(rec):
    """Every buffer of the recorder moves between two sentinel pages -> [(name, home, nbytes, guard)]."""
    fields = ("by_round", "by_degree", "by_head", "overflow", "skipped", "quota", "trace_cursor", "trace_meta", "trace_sets",
              "trace_fields")
    homes = []
    for attr in fields + ("_out_round", "_out_degree", "_out_head", "_counters"):     # (the read launch's outputs are arguments)
        inner = guarded(getattr(rec, attr), homes, attr)
        setattr(rec, attr, inner)
        if attr in fields and (attr != "quota" or rec.c.quota):
            setattr(rec.c, attr, inner.data_ptr())
    return homes


def assert_guards_untouched(homes):
    for name, home, nbytes, guard in homes:
        h = home.cpu().numpy()
        assert (h[:guard] == 0xA5).all() and (h[guard + nbytes:] == 0xA5).all(), name


def stub_net(heads):
    """What AttentionRecorder reads of a network, for launches on hand-built coefficients of any head count."""
    return types.SimpleNamespace(_MODEL=L.MODEL_LDGN, conv2=types.SimpleNamespace(heads=heads), feature_dtype="f32")


def hand_rows(rng, n, H, lives, state):
    """alpha / sources of one launch: a row per member of every live set.  Of three rows in four the sources hold the node
    itself, up to two neighbours that hold the message, up to two that wait for it and a few others; one in eight has none."""
    rows = sum(len(ids) for ids in lives)
    alpha = rng.random((rows + 2, MAX_SOURCES, H), dtype=np.float32)
    sources = np.zeros((rows + 2, (n + 63) // 64), dtype=np.uint64)
    r = 0
    for b, ids in enumerate(lives):
        sets = state["node_sets"][b].reshape(8, -1)
        has = members(sets[L.SET_HAS_MESSAGE], n)
        waiting = [j for j in members(sets[L.SET_INTERESTED], n) if j not in has]
        for i in ids:
            kind = rng.integers(0, 8)
            if kind == 0:
                chosen = []
            elif kind == 1:
                chosen = rng.choice(n, size=min(n, MAX_SOURCES), replace=False).tolist()     # a row at the cap
            else:
                pick = lambda pool, k: rng.choice(pool, size=min(k, len(pool)), replace=False).tolist() if pool else []
                chosen = [i] + pick([j for j in has if j != i], 2) + pick([j for j in waiting if j != i], 2) + pick(list(range(n)), 2)
            sources[r] = pack(sorted(set(chosen)), n)
            r += 1
    sources[rows:] = ~np.uint64(0)
    offsets = np.concatenate([[0], np.cumsum([len(ids) for ids in lives])]).astype(np.int32)
    live = np.stack([pack(ids, n) for ids in lives])
    return live, alpha, sources, offsets


@pytest.mark.parametrize("n,B,scripted,H", [(12, 6, 0.0, 4), (12, 6, 0.5, 6), (70, 4, 0.0, 16), (70, 4, 0.5, 1)])
def test_hand_built_launches_equal_the_model_bit_for_bit(n, B, scripted, H):
    """Every env meets every live set (empty, node 0, the highest node, the full set, beyond 64 nodes 63 + 64 + 69); then env 0
    stands at ``max_rounds``, env 1 in error and env 2 has met its quota, and they meet them again.  Random coefficients,
    hand-built source sets over the env's real message sets.  A ring of 4 records wraps.  Guard pages round every buffer."""
    from melissa_amd.attention_record import AttentionRecorder
    kw = dict(scripted_agents_ratio=scripted, heuristic="simple_broadcast") if scripted else {}
    venv, _loop = DR.played_venv(n, B, **kw)
    R, D, traced = 8, 4, (0, 2, B - 1)
    quota = [1000] * B
    rec = AttentionRecorder(venv, stub_net(H), max_rounds=R, n_degrees=D, trace_envs=traced, trace_capacity=4, quota=quota)
    homes = guard_buffers(rec)
    model = AttentionRecordModel(B, n, R, D, H, trace_envs=traced, trace_capacity=4, quota=quota)
    rng, cases = np.random.default_rng(n + B + H), DR.live_cases(n)
    sc = venv.scalars()
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()
    for phase in range(2):
        if phase == 1:
            sc[0, L.S_NUM_MOVES] = R                                     # past the round table
            sc[1, L.S_ERROR] = 4
            quota[2] = int(sc[2, L.S_EPISODES_DONE].item())              # met
            rec.quota.copy_(torch.tensor(quota, dtype=torch.int32))
            model.quota = np.asarray(quota, dtype=np.int64)
        state = state_of(venv)
        for k in range(len(cases)):
            live, alpha, sources, offsets = hand_rows(rng, n, H, [cases[(b + k) % len(cases)] for b in range(B)], state)
            h2 = []
            d_alpha, d_sources, d_offsets, d_live = (guarded(dev(t), h2, name) for t, name in (
                (alpha, "alpha"), (sources, "sources"), (offsets, "row_offsets"), (live, "live")))
            rec.launch_record(d_alpha, d_sources, d_offsets, d_live)
            model.launch(state, live, alpha, sources, offsets)
            torch.cuda.synchronize()
            assert_guards_untouched(h2)
    DR.assert_same(device_state(rec), model_state(model))
    by_round, by_degree, by_head, counters = assert_tables_equal_model(rec, model)
    booked = np.asarray(model.booked)
    both = (booked[:, 3] > 0) & (booked[:, 4] > 0)
    print(f"n={n} H={H}: {len(booked)} decisions booked, {both.sum()} with informed and waiting sources, most sources {booked[:, 2].max()}")
    assert len(booked) > 0 and 4 * both.sum() >= len(booked) and booked[:, 2].max() >= 3 and (booked[:, 2] == 0).any()
    assert by_degree[:, 0].sum() == len(booked) == by_head[:, 0].sum() / H
    assert counters["skipped"] == len(cases) and counters["overflow"] == by_degree[:, 0].sum() - by_round[:, 0].sum() > 0
    assert by_degree[D - 1, 0] > 0                                       # degrees past the table were clamped into its last row
    if not scripted:
        assert model.cursor.max() > 4                                    # the ring wrapped
    assert_guards_untouched(homes)


def play(n, B, use_graph=False, graph_rounds=1, attention=True, others=False, feed=False, model_name="l_dgn"):
    """``ROUNDS`` rounds of the round loop from one seed; the attention recorder traces every env.  ``feed``: the eager loop is
    stepped round by round, the model is fed with the loop's own coefficients and the tables are folded from the loop's own
    trace records."""
    from melissa_amd.attention_record import AttentionRecorder
    from melissa_amd.collect import RoundLoop
    from melissa_amd.decision_record import DecisionRecorder
    from melissa_amd.round_record import RoundRecorder
    venv = DR._venv(n, B)
    policy = DR._policy(model_name, n)
    att = AttentionRecorder(venv, policy.model, trace_envs=range(B), trace_capacity=64) if attention else None
    rec = RoundRecorder(venv, trace_envs=range(B), trace_capacity=64) if others else None
    dec = DecisionRecorder(venv, trace_envs=range(B), trace_capacity=64) if others else None
    loop = RoundLoop(venv, policy, episodes_per_env=12, seed=3, eps=0.1, use_graph=use_graph, graph_rounds=graph_rounds,
                     recorder=rec, decisions=dec, attention=att, episode_stream=False)
    model = folds = None
    if feed:
        H, W = att.heads, L.set_words(n)
        model = AttentionRecordModel(B, n, att.max_rounds, att.n_degrees, H, trace_envs=range(B), trace_capacity=64)
        folds = np.zeros((B, att.max_rounds, 8)), np.zeros((B, att.n_degrees, 8))
        seen = [0] * B
        for _ in range(ROUNDS):
            live = loop.live.cpu().numpy().view(np.uint64).reshape(B, W).copy()
            state = state_of(venv)
            loop.run(1)
            torch.cuda.synchronize()
            model.launch(state, live, att.alpha.cpu().numpy(), att.sources.cpu().numpy(), loop.offsets.cpu().numpy())
            att.drain_traces()
            for b in range(B):                                           # the loop's own records of this round, folded
                for r in att.records[b][seen[b]:]:
                    for i in members(r["sets"], n):
                        d = min(max(int(state["degree"][b][i]), 0), att.n_degrees - 1)
                        folds[0][b, int(r["meta"][3])] += r["fields"][i]
                        folds[1][b, d] += r["fields"][i]
                seen[b] = len(att.records[b])
    else:
        loop.run(ROUNDS)
        torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0 and loop.iterations == ROUNDS
    final = (venv.state.cpu().numpy().copy(), loop.act.cpu().numpy().copy(), loop.logits.cpu().numpy().copy())
    return dict(att=att, rec=rec, dec=dec, loop=loop, model=model, folds=folds, final=final)


@functools.lru_cache(maxsize=None)
def eager(n, B):
    """The eager loop with the model fed round by round: played once, shared by the tests that read it (nothing changes it)."""
    out = play(n, B, feed=True)
    out["state"] = device_state(out["att"])
    return out


LOOPS = [(12, 4), (70, 2)]


@pytest.mark.parametrize("n,B", LOOPS)
def test_the_loop_equals_the_model_and_the_fold_of_its_own_records(n, B):
    from melissa_amd.attention_record import group_attention_episodes
    e = eager(n, B)
    att, model = e["att"], e["model"]
    DR.assert_same(e["state"], model_state(model))
    by_round, by_degree, by_head, counters = assert_tables_equal_model(att, model)
    assert counters == dict(overflow=0, skipped=0)
    np.testing.assert_array_equal(bits(e["state"]["by_round"]), bits(e["folds"][0]))
    np.testing.assert_array_equal(bits(e["state"]["by_degree"]), bits(e["folds"][1]))
    booked = np.asarray(model.booked)
    print(f"n={n}: {len(booked)} decisions, informed attention {by_round[:, L.AR_INFORMED].sum():.3f}, waiting "
          f"{by_round[:, L.AR_WAITING].sum():.3f}, self {by_round[:, L.AR_SELF].sum():.3f}")
    assert by_round[:, 0].sum() == len(booked) > ROUNDS and (by_round[:, 0] > 0).sum() > 3
    assert by_round[:, L.AR_INFORMED].sum() > 0 and by_round[:, L.AR_WAITING].sum() > 0 and by_round[:, L.AR_SELF].sum() > 0
    # GATv2 coefficients of a row sum to 1: self + informed + waiting + the rest, so the three stay below the decisions
    assert (by_round[:, [L.AR_SELF, L.AR_INFORMED, L.AR_WAITING]].sum(1) <= by_round[:, 0] * (1 + 1e-6)).all()
    traces, lost = att.drain_traces()
    assert lost == 0 and sorted(traces) == list(range(B))
    for env in range(B):
        want = group_attention_episodes(model.all_records[env])
        assert [ep["ordinal"] for ep in traces[env]] == [ep["ordinal"] for ep in want] and len(want) >= 1
        for mine, theirs in zip(traces[env], want):
            for k in ("rounds", "decisions", "without_sources", "sets", "fields"):
                np.testing.assert_array_equal(bits(mine[k]), bits(theirs[k]), err_msg=k)


@pytest.mark.parametrize("n,B", LOOPS)
def test_captured_rounds_equal_eager_rounds(n, B):
    """One eager warm-up round, the one-round graph, then groups of four rounds from one graph - against eager launches."""
    want = eager(n, B)["state"]
    out = play(n, B, use_graph=True, graph_rounds=4)
    assert out["loop"].group_graph is not None
    DR.assert_same(device_state(out["att"]), want)
    assert out["att"].tables()[3] == dict(overflow=0, skipped=0) and out["att"].drain_traces()[1] == 0


def test_beside_the_other_recorders_nothing_changes_and_without_it_nothing_is_launched():
    from melissa_amd.attention_record import AttentionRecorder
    n, B = 12, 4
    e = eager(n, B)
    calls = AttentionRecorder.launches
    assert calls >= ROUNDS                                               # (the counter does count: the eager loop's launches)
    plain = play(n, B, attention=False, others=True)
    assert plain["att"] is None and plain["loop"].attention is None and AttentionRecorder.launches == calls
    both = play(n, B, attention=True, others=True)
    assert AttentionRecorder.launches == calls + ROUNDS
    RR.assert_same(RR.device_state(both["rec"]), RR.device_state(plain["rec"]))
    DR.assert_same(DR.device_state(both["dec"]), DR.device_state(plain["dec"]))
    DR.assert_same(device_state(both["att"]), e["state"])
    for got, want, alone, name in zip(both["final"], plain["final"], e["final"], ("env state", "act", "logits")):
        np.testing.assert_array_equal(bits(got), bits(want), err_msg=name)
        np.testing.assert_array_equal(bits(got), bits(alone), err_msg=name)


def test_dgn_r_rides_too_and_hl_dgn_and_bf16_raise():
    from melissa_amd.attention_record import AttentionRecorder
    from melissa_amd.collect import RoundLoop
    n, B = 12, 4
    out = play(n, B, model_name="dgn_r")
    by_round, by_degree, by_head, counters = out["att"].tables()
    assert counters == dict(overflow=0, skipped=0) and by_round[:, 0].sum() > ROUNDS
    assert by_round[:, L.AR_SELF].sum() == 0 and by_round[:, L.AR_INFORMED].sum() > 0       # TransformerConv: no self-loop
    venv = DR._venv(n, B)
    with pytest.raises(ValueError, match="HL-DGN"):
        AttentionRecorder(venv, DR._policy("hl_dgn", n).model)
    from tests.test_gpu_forward import make_net
    net = make_net("l_dgn", n, 9)[0].set_feature_dtype("bf16")
    with pytest.raises(ValueError, match="bf16"):
        AttentionRecorder(venv, net)
    with pytest.raises(ValueError, match="another"):
        RoundLoop(venv, DR._policy("l_dgn", n), use_graph=False, attention=AttentionRecorder(venv, DR._policy("dgn_r", n).model))
    with pytest.raises(ValueError, match="another env batch"):
        RoundLoop(DR._venv(n, B), DR._policy("l_dgn", n), use_graph=False, attention=AttentionRecorder(venv, DR._policy("l_dgn", n).model))


def test_spread_evaluation_and_watch_write_both_files(tmp_path):
    from melissa_amd.attention_record import AttentionRecorder, summarise_attention
    from melissa_amd.collect import evaluate_spread
    from melissa_amd.watch import watch
    n, B, T = 12, 4, 10
    policy, venv = DR._watch_setup(n, B, T, DR.SEED)
    att = AttentionRecorder(venv, policy.model, trace_envs=range(2), trace_capacity=64)
    evaluate_spread(policy, venv, T, eps=0.0, seed=DR.SEED, attention=att)
    by_round, by_degree, by_head, counters = att.tables()
    assert counters == dict(overflow=0, skipped=0) and by_round[:, 0].sum() == by_degree[:, 0].sum() > 0
    traces, lost = att.drain_traces()
    assert lost == 0 and [[ep["ordinal"] for ep in traces[b]] for b in range(2)] == [[0, 1, 2], [0, 1, 2]]
    with pytest.raises(ValueError, match="trace_capacity"):
        evaluate_spread(policy, venv, T, attention=AttentionRecorder(venv, policy.model, trace_envs=(0,), trace_capacity=15), chunk=8)
    out_json, out_npz = tmp_path / "attention.json", tmp_path / "attention.npz"
    out = watch(model="l_dgn", n_nodes=n, envs=B, episodes=T, seed=DR.SEED, spread=True, graphs=4,
                attention_curves_out=str(out_json), attention_trace_out=str(out_npz), trace_envs=2)
    assert out["n/ep"] == T
    doc = json.loads(out_json.read_text())
    for key, want in (("by_round_sums", by_round), ("by_degree_sums", by_degree), ("by_head_sums", by_head)):
        np.testing.assert_array_equal(bits(np.asarray(doc[key])), bits(want), err_msg=key)
    assert doc["counters"] == dict(overflow=0, skipped=0, lost_trace_records=0)
    s = summarise_attention(by_round, by_degree, by_head)
    assert doc["total"]["decisions"] == by_degree[:, 0].sum() and doc["total"]["informed_lift"] == s["total"]["informed_lift"]
    assert doc["by_round"]["effective_neighbours"][0] == s["by_round"]["effective_neighbours"][0] and None in doc["by_round"]["self_mean"]
    saved = np.load(str(out_npz))
    assert sorted({k.rsplit("_", 1)[0] for k in saved.files if k.endswith("_rounds")}) == [f"e{b}_o{o}" for b in range(2) for o in range(3)]
    for b in range(2):
        for ep in traces[b]:
            for k in ("rounds", "decisions", "without_sources", "sets", "fields"):
                np.testing.assert_array_equal(bits(saved[f"e{b}_o{ep['ordinal']}_{k}"]), bits(ep[k]), err_msg=k)
