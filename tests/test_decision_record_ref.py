"""CPU checks of the decision recorder's host side (melissa_amd/decision_record.py) and of the NumPy model of its launch
(tests/decision_record_ref.py) that the GPU tests hold the device to: the booking rules on hand examples with known sums,
``summarise_decisions`` on hand tables, the ``watch`` argument errors, and every argument error of the two entry points (all of
them returned before anything is launched)."""
import math

import numpy as np
import pytest

from melissa_amd import _lib
from melissa_amd.decision_record import (FIELDS, check_decision_args, group_decision_episodes, save_decision_traces,
                                         summarise_decisions)
from tests.decision_record_ref import DecisionRecordModel, greedy, members, pack

N = 5


def state(B=2, num_moves=(1, 2), episodes_done=(0, 0), error=(0, 0), scripted=((), ()), taken=((), ()), degree=None):
    sc = np.zeros((B, 16), dtype=np.int32)
    sc[:, _lib.S_NUM_MOVES], sc[:, _lib.S_EPISODES_DONE], sc[:, _lib.S_ERROR] = num_moves, episodes_done, error
    sc[:, _lib.S_EPISODE] = 40 + np.arange(B)
    ns, ss = np.zeros((B, 8, 1), dtype=np.uint64), np.zeros((B, 4, 1), dtype=np.uint64)
    for b in range(B):
        ns[b, _lib.SET_SCRIPTED], ss[b, 3] = pack(scripted[b], N), pack(taken[b], N)
    degree = np.array([[1, 2, 2, 0, 7]] * B, dtype=np.float32) if degree is None else np.asarray(degree, dtype=np.float32)
    return dict(scalars=sc, node_sets=ns, sel_sets=ss, degree=degree)


# env 0: nodes 1 and 3 decide (rows 0, 1); env 1: nodes 0, 2, 4 (rows 2, 3, 4).  Values exact in fp32.
LIVE = np.stack([pack([1, 3], N), pack([0, 2, 4], N)])
OFFSETS = np.array([0, 2, 5], dtype=np.int32)
LOGITS = np.array([[0.5, 1.5], [2.0, -1.0], [0.25, 0.25], [-3.0, -2.0], [1.0, 0.0]], dtype=np.float32)
ACT = np.array([1, 1, 0, 1, 1], dtype=np.int32)


def test_hand_example_with_known_sums():
    m = DecisionRecordModel(2, N, max_rounds=4, n_degrees=3, trace_envs=(1,), trace_capacity=2)
    m.launch(state(taken=((3,), (0, 2))), LIVE, LOGITS, ACT, OFFSETS)
    # env 0, round 1: node 1 (gap 1, relays, greedy, first) and node 3 (gap -3, relays against the greedy 0, not first)
    np.testing.assert_array_equal(m.by_round[0, 1], [2, 2, -2, 10, 0.5, 3.5, 1, 1])
    assert not m.by_round[0, [0, 2, 3]].any()
    # env 1, round 2: node 0 (a tie: greedy is 0, silent), node 2 (gap 1, relays), node 4 (gap -1, relays, not greedy, first)
    np.testing.assert_array_equal(m.by_round[1, 2], [3, 2, 0, 2, 0.25 - 2.0 + 0.0, 0.25 - 2.0 + 1.0, 1, 1])
    # by degree: the nodes' degrees 1, 2, 2, 0, 7 -> rows 1, 2, 2, 0, 2 (clamped to the last row)
    np.testing.assert_array_equal(m.by_degree[0, :, 0], [1, 0, 1])       # node 3 (degree 0), node 1 (degree 2)
    np.testing.assert_array_equal(m.by_degree[1, :, 0], [0, 1, 2])       # node 0 (degree 1); nodes 2 and 4 (2 and 7 -> 2)
    np.testing.assert_array_equal(m.by_degree[1, 2], [2, 2, 0, 2, -2.0 + 0.0, -2.0 + 1.0, 1, 1])
    assert m.by_round.sum(axis=(0, 1)).tolist() == m.by_degree.sum(axis=(0, 1)).tolist()
    assert m.overflow.tolist() == [0, 0] and m.skipped.tolist() == [0, 0]
    # the trace of env 1: one record, env / ordinal / pool episode / round / decisions / relays
    assert m.cursor.tolist() == [1]
    assert m.ring["meta"][0, 0].tolist() == [1, 0, 41, 2, 3, 2, 0, 0]
    assert members(m.ring["sets"][0, 0, 0], N) == [0, 2, 4] and members(m.ring["sets"][0, 0, 1], N) == [2, 4]
    np.testing.assert_array_equal(m.ring["q"][0, 0], [[0.25, 0.25], [0, 0], [-3, -2], [0, 0], [1, 0]])
    by_round, by_degree, counters = m.folded()
    assert by_round[:, 0].tolist() == [0, 2, 3, 0] and by_degree[:, 0].tolist() == [1, 1, 3] and counters == dict(overflow=0, skipped=0)
    # a second launch on the same inputs doubles every sum and writes the next ring slot
    m.launch(state(taken=((3,), (0, 2))), LIVE, LOGITS, ACT, OFFSETS)
    np.testing.assert_array_equal(m.by_round[0, 1], [4, 4, -4, 20, 1.0, 7.0, 2, 2])
    assert m.cursor.tolist() == [2] and (m.ring["meta"][0, 1] == m.ring["meta"][0, 0]).all() and len(m.all_records[1]) == 2


def test_dense_layout_serves_every_agent_from_the_envs_row():
    """row_offsets None (HL-DGN): logits row b for every agent of env b, act in the dense [B, N] layout."""
    m = DecisionRecordModel(2, N, max_rounds=4, n_degrees=8)
    act = np.zeros((2, N), dtype=np.int32)
    act[0, 3], act[1, 2], act[1, 4] = 1, 1, 1
    m.launch(state(), LIVE, np.array([[1.0, 3.0], [2.0, 0.5]], dtype=np.float32), act, None)
    np.testing.assert_array_equal(m.by_round[0, 1], [2, 1, 4, 8, 1.0 + 3.0, 6, 1, 2])      # node 1 silent against the greedy 1
    np.testing.assert_array_equal(m.by_round[1, 2], [3, 2, -4.5, 6.75, 2.0 + 0.5 + 0.5, 6, 2, 3])
    assert m.by_degree[1, 7].tolist()[0] == 1 and m.by_degree[:, 3:7].sum() == 0


def test_the_gap_is_one_fp32_subtraction():
    q = np.array([[np.float32(0.1), np.float32(0.3)]], dtype=np.float32)
    m = DecisionRecordModel(1, N, max_rounds=2, n_degrees=2)
    m.launch(state(B=1, num_moves=(0,), episodes_done=(0,), error=(0,), scripted=((),), taken=((),)),
             np.stack([pack([2], N)]), q, np.array([1], dtype=np.int32), np.array([0, 1], dtype=np.int32))
    gap = float(np.float32(0.3) - np.float32(0.1))
    assert m.by_round[0, 0, 2] == gap != float(np.float32(0.3)) - float(np.float32(0.1))
    assert m.by_round[0, 0, 3] == gap * gap


def test_greedy_is_the_first_maximum():
    f = lambda *q: greedy(np.array(q, dtype=np.float32))
    assert (f(1, 2), f(2, 1), f(1, 1), f(-1, -1), f(np.nan, 0), f(0, np.nan), f(np.nan, np.nan)) == (1, 0, 0, 0, 1, 0, 0)


def test_scripted_nodes_are_excluded_but_keep_their_rows():
    """A scripted member of live has a row (the forward covers it), so the ranks of the others do not move."""
    m = DecisionRecordModel(2, N, max_rounds=4, n_degrees=3, trace_envs=(0, 1))
    m.launch(state(scripted=((1, 3), (2,))), LIVE, LOGITS, ACT, OFFSETS)
    assert not m.by_round[0].any() and not m.by_degree[0].any()          # every live node of env 0 is scripted
    np.testing.assert_array_equal(m.by_round[1, 2], [2, 1, -1, 1, 0.25 + 0.0, 0.25 + 1.0, 1, 2])      # rows 2 and 4
    assert m.cursor.tolist() == [0, 1]                                   # no decision, no record
    assert members(m.ring["sets"][1, 0, 0], N) == [0, 4] and (m.ring["q"][1, 0, 2] == 0).all()


def test_quota_and_error_skips():
    m = DecisionRecordModel(2, N, max_rounds=4, n_degrees=3, quota=[1, 1])
    m.launch(state(episodes_done=(1, 0), error=(0, 0)), LIVE, LOGITS, ACT, OFFSETS)      # env 0 has met its quota
    assert not m.by_round[0].any() and m.by_round[1, 2, 0] == 3 and m.skipped.tolist() == [0, 0]
    m.launch(state(episodes_done=(0, 0), error=(0, 4)), LIVE, LOGITS, ACT, OFFSETS)      # env 1 is in error
    assert m.by_round[0, 1, 0] == 2 and m.by_round[1, 2, 0] == 3 and m.skipped.tolist() == [0, 1]
    m.launch(state(episodes_done=(5, 0), error=(2, 0)), LIVE, LOGITS, ACT, OFFSETS)      # the error counts before the quota
    assert m.skipped.tolist() == [1, 1] and m.overflow.tolist() == [0, 0]
    assert m.folded()[2] == dict(overflow=0, skipped=2)


def test_degree_clamping_and_round_overflow():
    m = DecisionRecordModel(2, N, max_rounds=2, n_degrees=2)
    m.launch(state(num_moves=(1, 2)), LIVE, LOGITS, ACT, OFFSETS)
    assert m.by_round[0, 1, 0] == 2 and not m.by_round[1].any()          # env 1 is at round 2 >= max_rounds
    assert m.overflow.tolist() == [0, 3]                                 # one per dropped row
    np.testing.assert_array_equal(m.by_degree[:, :, 0], [[1, 1], [0, 3]])            # the by-degree rows are still booked
    assert [a[1] for a in m.addends] == [1, 1, None, None, None] and [a[2] for a in m.addends] == [1, 0, 1, 1, 1]


def test_summarise_decisions_on_hand_tables():
    by_round = np.zeros((3, 8))
    by_round[1] = [4, 3, 2.0, 5.0, 6.0, 8.0, 1, 2]
    by_degree = np.zeros((2, 8))
    by_degree[0], by_degree[1] = [1, 1, 1.0, 1.0, 2.0, 2.0, 0, 1], [3, 2, 1.0, 4.0, 4.0, 6.0, 1, 1]
    s = summarise_decisions(by_round, by_degree)
    assert s["rounds"].tolist() == [0, 1, 2] and s["degrees"].tolist() == [0, 1]
    r = s["by_round"]
    assert r["decisions"].tolist() == [0, 4, 0]
    for key, want in (("relay_rate", 0.75), ("gap_mean", 0.5), ("gap_std", 1.0), ("chosen_q_mean", 1.5), ("max_q_mean", 2.0),
                      ("non_greedy_share", 0.25), ("first_decision_share", 0.5)):
        assert r[key][1] == want, key
        assert math.isnan(r[key][0]) and math.isnan(r[key][2]), key
    d = s["by_degree"]
    assert d["relay_rate"].tolist() == [1.0, 2 / 3] and d["gap_std"][0] == 0.0
    assert d["gap_std"][1] == pytest.approx(math.sqrt(4 / 3 - 1 / 9))
    assert s["total"] == dict(decisions=4.0, relay_rate=0.75, gap_mean=0.5, gap_std=1.0, chosen_q_mean=1.5, max_q_mean=2.0,
                              non_greedy_share=0.25, first_decision_share=0.5)
    empty = summarise_decisions(np.zeros((2, 8)), np.zeros((1, 8)))
    assert empty["total"]["decisions"] == 0.0 and all(math.isnan(v) for k, v in empty["total"].items() if k != "decisions")
    with pytest.raises(ValueError, match="by_degree"):
        summarise_decisions(np.zeros((2, 8)), np.zeros((2, 7)))
    assert len(FIELDS) == _lib.DR_FIELDS


def test_records_group_by_episode_ordinal_and_save(tmp_path):
    m = DecisionRecordModel(2, N, max_rounds=4, n_degrees=3, trace_envs=(1,))
    for ep, mv in ((0, 0), (0, 1), (1, 0)):
        m.launch(state(num_moves=(0, mv), episodes_done=(0, ep)), LIVE, LOGITS, ACT, OFFSETS)
    episodes = group_decision_episodes(m.all_records[1])
    assert [(e["env"], e["ordinal"], e["pool_episode"], e["rounds"].tolist()) for e in episodes] == [(1, 0, 41, [0, 1]), (1, 1, 41, [0])]
    assert episodes[0]["q"].shape == (2, N, 2) and episodes[0]["sets"].shape == (2, 2, 1) and episodes[0]["relays"].tolist() == [2, 2]
    out = tmp_path / "d.npz"
    save_decision_traces(str(out), {1: episodes})
    saved = np.load(str(out))
    assert sorted(saved.files) == sorted(f"e1_o{o}_{k}" for o in (0, 1) for k in episodes[0])
    assert (saved["e1_o0_q"] == episodes[0]["q"]).all() and saved["e1_o1_sets"].dtype == np.uint64


def test_decision_arguments():
    check_decision_args(False)
    check_decision_args(True, "d.json", "t.npz", 4)
    for kw in (dict(decisions_out="d.json"), dict(decision_trace_out="t.npz")):
        with pytest.raises(ValueError, match="spread"):
            check_decision_args(False, **kw)
    with pytest.raises(ValueError, match="trace_envs"):
        check_decision_args(True, decision_trace_out="t.npz", trace_envs=17)


def test_watch_flags_need_spread(capsys):
    from melissa_amd import watch
    for flags in (["--decisions-out", "d.json"], ["--decision-trace-out", "t.npz"]):
        with pytest.raises(SystemExit):
            watch.parse_args(flags)
        assert "spread" in capsys.readouterr().err
    a = watch.parse_args(["--spread", "--decisions-out", "d.json", "--decision-trace-out", "t.npz", "--trace-envs", "2"])
    assert (a.decisions_out, a.decision_trace_out, a.trace_envs) == ("d.json", "t.npz", 2)
    assert not hasattr(watch.parse_args(["--spread"]), "decisions_out")            # a plain call's namespace is what it was
    # the function refuses at argument time too: before a network or an env is built
    with pytest.raises(ValueError, match="spread"):
        watch.watch(model="l_dgn", n_nodes=20, envs=1, episodes=2, decisions_out="d.json", device="no-such-device")


def test_abi_sizeof_and_argument_errors():
    """``mel_abi_sizeof`` id 16 against the ctypes twin, and every argument error of the two entry points: all of them are
    returned before anything is launched, so made-up (never dereferenced) pointers do."""
    import ctypes as C
    lib = _lib.load()
    assert C.sizeof(_lib.MelDecisionRecord) == lib.mel_abi_sizeof(16) == 160
    for name in ("mel_decision_record_round", "mel_decision_record_read"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    fake = 0x10000
    pointers = [name for name, kind in _lib.MelDecisionRecord._fields_ if kind is C.c_void_p and name != "quota"]

    def record(**kw):
        r = _lib.MelDecisionRecord()
        for name in pointers:
            setattr(r, name, fake)
        r.n_envs, r.n_nodes, r.max_rounds, r.n_degrees, r.n_trace, r.trace_capacity = 4, 20, 8, 20, 0, 0
        for k, v in kw.items():
            if k == "trace_env":
                for i, t in enumerate(v):
                    r.trace_env[i] = t
            else:
                setattr(r, k, v)
        return r

    env = _lib.MelEnvBatch()
    env.n_envs, env.n_nodes = 4, 20
    for name in ("scalars", "node_sets", "sel_sets", "obs_matrix"):
        setattr(env, name, fake)
    read = lib.mel_decision_record_read

    def round_(ref, env_ref, logits=fake, act=fake, offsets=fake, live=fake, n_actions=2):
        return lib.mel_decision_record_round(ref, env_ref, logits, act, offsets, live, n_actions, None)

    def refused(r, word):
        ref = C.byref(r) if r is not None else None
        for st in (round_(ref, C.byref(env)), read(ref, fake, fake, fake, None)):
            assert st == _lib.ERR_INVALID_ARG and word.encode() in lib.mel_last_error(), (word, lib.mel_last_error())

    refused(None, "null")
    for name in ("by_round", "by_degree", "overflow", "skipped"):
        refused(record(**{name: None}), "null buffer")
    refused(record(max_rounds=0), "max_rounds")
    refused(record(max_rounds=_lib.DR_MAX_ROUNDS + 1), "max_rounds")
    refused(record(n_degrees=0), "n_degrees")
    refused(record(n_degrees=_lib.DR_MAX_DEGREES + 1), "n_degrees")
    refused(record(n_trace=-1), "n_trace")
    refused(record(n_trace=_lib.DR_MAX_TRACE + 1), "n_trace")
    refused(record(n_trace=1, trace_capacity=0, trace_env=[0]), "trace_capacity")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[0, 4]), "outside")
    refused(record(n_trace=1, trace_capacity=4, trace_env=[-1]), "outside")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[1, 1]), "twice")
    for name in ("trace_cursor", "trace_meta", "trace_sets", "trace_q"):
        refused(record(n_trace=1, trace_capacity=4, trace_env=[0], **{name: None}), "trace sink")
    # the env batch: null, unbound, other sizes; the forward's outputs (the round entry point only; row_offsets may be null)
    ok = C.byref(record())
    assert round_(ok, None) == _lib.ERR_INVALID_ARG and b"env is null" in lib.mel_last_error()
    assert round_(ok, C.byref(_lib.MelEnvBatch())) == _lib.ERR_INVALID_ARG and b"not bound" in lib.mel_last_error()
    assert round_(C.byref(record(n_envs=5)), C.byref(env)) == _lib.ERR_INVALID_ARG and b"envs" in lib.mel_last_error()
    assert round_(C.byref(record(n_nodes=21)), C.byref(env)) == _lib.ERR_INVALID_ARG
    for kw in (dict(logits=None), dict(act=None), dict(live=None)):
        assert round_(ok, C.byref(env), **kw) == _lib.ERR_INVALID_ARG and b"null input" in lib.mel_last_error()
    for na in (1, 3):
        assert round_(ok, C.byref(env), n_actions=na) == _lib.ERR_UNSUPPORTED and b"n_actions" in lib.mel_last_error()
    # the read entry point's outputs
    for outs in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert read(ok, *outs, None) == _lib.ERR_INVALID_ARG and b"null output" in lib.mel_last_error()
