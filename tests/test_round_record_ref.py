"""CPU checks of the per-round recorder's host side: the NumPy model of the device's sampling rules
(tests/round_record_ref.py) on the states of the REAL reference env (tests/golden/render_trace_n12_fixture.npz, written by
tests/golden/make_render_golden.py), the reference's colour rule, ``summarise``'s invariants and the SVG frames."""
import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

from melissa_amd import _lib, render
from melissa_amd.round_record import FIELDS, check_record_args, group_episodes, save_traces, summarise
from tests.round_record_ref import RoundRecordModel

HERE = os.path.dirname(os.path.abspath(__file__))
N = 12
TRACES = ("static", "dynamic")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "render_trace_n12_fixture.npz"))


def launch_states(golden, name):
    """The golden's rows as the per-launch states of ONE env (the layout of round_record_ref), with their colours."""
    g = {k[len(name) + 1:]: golden[k] for k in golden.files if k.startswith(name + "_")}
    out = []
    for r in range(len(g["ordinal"])):
        sc = np.zeros((1, 16), dtype=np.int32)
        sc[0, _lib.S_EPISODES_DONE], sc[0, _lib.S_NUM_MOVES] = g["ordinal"][r], g["num_moves"][r]
        sc[0, _lib.S_WORLD_MSGS], sc[0, _lib.S_ORIGIN], sc[0, _lib.S_EPISODE] = g["world_msgs"][r], g["origin"][r], g["ordinal"][r]
        ns, ss = np.zeros((1, 8, 1), dtype=np.uint64), np.zeros((1, 4, 1), dtype=np.uint64)
        ns[0, _lib.SET_HAS_MESSAGE, 0], ns[0, _lib.SET_ORIGIN, 0] = g["has_message"][r], g["origin_set"][r]
        ns[0, _lib.SET_INTERESTED, 0], ns[0, _lib.SET_SCRIPTED, 0] = g["interested"][r], g["scripted"][r]
        ss[0, 0, 0], ss[0, 3, 0] = g["active"][r], g["taken_action"][r]
        out.append((dict(scalars=sc, node_sets=ns, sel_sets=ss, pos=g["pos"][r][None], one_hop=g["one_hop"][r].reshape(1, N, 1),
                         agent_msgs=g["agent_msgs"][r][None], received=g["received"][r][None]), g["colour"][r]))
    return out


def closing_state(state, ordinal):
    """A state that only tells the recorder that episode ``ordinal - 1`` has ended (the next episode's reset)."""
    st = {k: v.copy() for k, v in state.items()}
    st["scalars"][0, _lib.S_EPISODES_DONE], st["scalars"][0, _lib.S_NUM_MOVES] = ordinal, 0
    return st


def run_model(golden, name, **kw):
    rows = launch_states(golden, name)
    model = RoundRecordModel(1, N, kw.pop("max_rounds", 16), trace_envs=[0], trace_capacity=64, quota=[2], **kw)
    for state, _colour in rows:
        model.launch(state)
    model.launch(closing_state(rows[0][0], 2))          # past the quota: books the second episode's end, samples nothing
    return model, rows


@pytest.mark.parametrize("name", TRACES)
def test_colour_classes_equal_the_reference(golden, name):
    model, rows = run_model(golden, name)
    classes = [str(c) for c in golden["classes"]]
    assert tuple(classes) == render.CLASSES
    episodes = group_episodes(model.all_records[0])
    assert [e["ordinal"] for e in episodes] == [0, 1] and sum(len(e["rounds"]) for e in episodes) == len(rows)
    got = [row for e in episodes for row in render.colour_classes(e)]
    drawn = 0
    for (_state, colour), mine in zip(rows, got):
        if colour[0] < 0:                               # a reset: the reference draws nothing there
            continue
        assert mine == [classes[c] for c in colour]
        drawn += 1
    assert drawn == len(rows) - 2
    used = {c for (_s, colour) in rows for c in colour if c >= 0}
    assert len(used) >= 4                               # the tape reaches (nearly) every branch of the rule


@pytest.mark.parametrize("name", TRACES)
def test_model_samples_follow_the_states(golden, name):
    model, rows = run_model(golden, name)
    run, end, counters = model.folded()
    assert counters == dict(overflow=0, skipped=0, unlogged=2)          # (the golden feeds no episode log: booked at the last sample)
    assert run[0, 0] == 2 and end[:, 0].sum() == 2      # two episodes started, two booked as ended
    g = {k: golden[f"{name}_{k}"] for k in ("ordinal", "num_moves", "world_msgs", "has_message", "interested")}
    for r in range(run.shape[0]):
        at = np.flatnonzero(g["num_moves"] == r)
        assert run[r, 0] == len(at)
        assert run[r, _lib.RR_MESSAGES] == g["world_msgs"][at].sum()
        assert run[r, _lib.RR_HAS_MESSAGE] == sum(bin(int(m)).count("1") for m in g["has_message"][at])
        frac = 0.0
        for i in at:                                    # play order
            n_int = bin(int(g["interested"][i])).count("1")
            frac += (bin(int(g["has_message"][i] & g["interested"][i])).count("1") / n_int) if n_int else 0.0
        assert run[r, _lib.RR_COVERAGE_FRACTION] == frac
    # an ended episode's row is its last sample
    for o in (0, 1):
        last = np.flatnonzero(g["ordinal"] == o)[-1]
        assert end[g["num_moves"][last], 0] >= 1
    assert end[:, _lib.RR_MESSAGES].sum() == sum(g["world_msgs"][np.flatnonzero(g["ordinal"] == o)[-1]] for o in (0, 1))
    assert (model.seen == [[2, 0]]).all()


@pytest.mark.parametrize("name", TRACES)
def test_summarise_invariants(golden, name):
    model, _rows = run_model(golden, name)
    run, end, _ = model.folded()
    s = summarise(run, end, n_nodes=N)
    assert s["episodes"] == 2
    before = np.concatenate([[0.0], np.cumsum(end[:, 0])[:-1]])
    assert (run[:, 0] + before == 2).all() and (s["carried_count"] == 2).all()
    assert (s["running"] == run[:, 0]).all() and s["running"][0] == 2 and s["running"][-1] == 0
    assert (np.diff(s["covered_share"]) >= 0).all() and 0.0 <= s["covered_share"][-1] <= 1.0
    assert (np.diff(s["coverage"]) >= 0).all() and s["coverage"][-1] <= 1.0          # has_message only grows, ended episodes stay
    assert (np.diff(s["messages"]) >= 0).all()
    assert ((0.0 <= s["coverage_interested_fraction"]) & (s["coverage_interested_fraction"] <= 1.0)).all()
    for q, r in s["delay"].items():
        if r is not None:
            assert s["covered_share"][r] >= q and (r == 0 or s["covered_share"][r - 1] < q)
        else:
            assert s["covered_share"][-1] < q
    qs = [s["delay"][q] for q in sorted(s["delay"])]
    known = [r for r in qs if r is not None]
    assert known == sorted(known) and qs[:len(known)] == known                          # quantiles in order, unknown ones last


def test_summarise_hand_example():
    run, end = np.zeros((4, 8)), np.zeros((4, 8))
    # episode A: rounds 0..2, covered at round 1; episode B: rounds 0..1, never covered
    for r, (has, msgs, frac, newly) in enumerate([(1, 1, 0.0, 0), (5, 2, 1.0, 1), (6, 4, 1.0, 0)]):
        run[r] += [1, has, 0, 0, msgs, 0, frac, newly]
    end[2] += [1, 6, 0, 0, 4, 0, 1.0, 0]
    for r, (has, msgs, frac) in enumerate([(1, 1, 0.0), (2, 3, 0.5)]):
        run[r] += [1, has, 0, 0, msgs, 0, frac, 0]
    end[1] += [1, 2, 0, 0, 3, 0, 0.5, 0]
    s = summarise(run, end)
    assert s["episodes"] == 2 and s["running"].tolist() == [2, 2, 1, 0]
    assert s["messages"].tolist() == [1.0, 2.5, 3.5, 3.5]
    assert s["coverage_interested_fraction"].tolist() == [0.0, 0.75, 0.75, 0.75]
    assert s["covered_share"].tolist() == [0.0, 0.5, 0.5, 0.5]
    assert s["delay"] == {0.5: 1, 0.9: None, 1.0: None}
    with pytest.raises(ValueError):
        summarise(run[:, :7], end[:, :7])


def test_model_rules_idempotence_errors_overflow_ring(golden):
    rows = launch_states(golden, "static")
    model = RoundRecordModel(1, N, 3, trace_envs=[0], trace_capacity=4)
    for state, _ in rows:
        model.launch(state)
        snapshot = (model.running.copy(), model.ended.copy(), model.carry.copy(), model.cursor.copy())
        model.launch(state)                              # the same state again: nothing moves
        for a, b in zip(snapshot, (model.running, model.ended, model.carry, model.cursor)):
            assert (a == b).all()
    moves = golden["static_num_moves"]
    last = [int(moves[np.flatnonzero(golden["static_ordinal"] == o)[-1]]) for o in (0,)]      # only episode 0 has been booked
    assert model.overflow[0] == int((moves >= 3).sum()) + sum(m >= 3 for m in last) > 0
    assert model.cursor[0] == len(rows) and len(model.all_records[0]) == len(rows)
    for j in range(len(rows) - 4, len(rows)):            # the ring holds the last four records
        assert (model.ring["meta"][0, j % 4] == model.all_records[0][j]["meta"]).all()
    bad = {k: v.copy() for k, v in rows[1][0].items()}
    bad["scalars"][0, _lib.S_ERROR] = 2
    fresh = RoundRecordModel(1, N, 8)
    fresh.launch(bad)
    assert fresh.skipped[0] == 1 and fresh.running.sum() == 0 and (fresh.carry == -1).all()


def test_model_takes_the_final_sample_from_the_episode_log(golden):
    """An episode whose last world step also ends it: the launch after it sees the next episode's reset state only.  With the
    env's row in the episode log the model (and the device) books the final sample from the row; the result is what feeding
    the lost state would have given, but for field 5 (nobody acts after the end)."""
    rows = launch_states(golden, "static")
    ordinal, moves = golden["static_ordinal"], golden["static_num_moves"]
    final = int(np.flatnonzero(ordinal == 0)[-1])                    # episode 0's last world step: hide it from the model
    full = RoundRecordModel(1, N, 16)
    for state, _ in rows[:final + 2]:
        full.launch(state)
    lost = rows[final][0]
    has, interested = int(lost["node_sets"][0, 0, 0]), int(lost["node_sets"][0, 2, 0])
    n_int, cov = bin(interested).count("1"), bin(has & interested).count("1")
    stats = np.zeros((1, 10))
    stats[0, 0], stats[0, 1] = lost["scalars"][0, _lib.S_WORLD_MSGS], bin(has).count("1") / N
    stats[0, 5], stats[0, 6], stats[0, 7] = n_int, (cov / n_int if n_int else 0.0), cov
    log = dict(log_cursor=1, log_capacity=8, log_stats=stats, log_meta=np.array([[0, 0, moves[final]]], dtype=np.int32))
    blind = RoundRecordModel(1, N, 16)
    for k, (state, _) in enumerate(rows[:final + 2]):
        if k != final:
            blind.launch(dict(state, **(log if k > final else dict(log, log_cursor=0))))
    assert blind.unlogged[0] == 0 and full.unlogged[0] == 1
    keep = [f for f in range(8) if f != _lib.RR_ACTIVE]
    assert (blind.running[..., keep] == full.running[..., keep]).all() and (blind.ended[..., keep] == full.ended[..., keep]).all()
    assert blind.ended[0, moves[final], 0] == 1 and blind.running[0, moves[final], 0] == 1
    assert (blind.carry[0, :4] == full.carry[0, :4]).all()


@pytest.mark.parametrize("name", TRACES)
def test_svg_frames(golden, name, tmp_path):
    model, rows = run_model(golden, name)
    episodes = group_episodes(model.all_records[0])
    total = 0
    for ep in episodes:
        classes = render.colour_classes(ep)
        paths = render.write_svg_frames(ep, str(tmp_path / name))
        assert len(paths) == len(ep["rounds"]) == len(set(paths))
        for k, path in enumerate(paths):
            root = ET.parse(path).getroot()
            ns = {"s": "http://www.w3.org/2000/svg"}
            circles, lines, labels = root.findall("s:circle", ns), root.findall("s:line", ns), root.findall("s:text", ns)
            assert len(circles) == N and len(labels) == N
            assert len(lines) == len(render.edges(ep["one_hop"][k], N))
            assert [c.get("fill") for c in circles] == [render.FILL[c] for c in classes[k]]
            assert [c.get("class") for c in circles] == classes[k]
            assert [t.text for t in labels] == [str(i) for i in range(N)]
        total += len(paths)
    assert total == len(rows)
    if name == "static":                                 # the fixture graph: 13 edges, never moved
        assert len(render.edges(episodes[0]["one_hop"][0], N)) == 13
    out = tmp_path / f"{name}.npz"
    save_traces(str(out), {0: episodes})
    saved = np.load(str(out))
    assert (saved["e0_o1_agent_msgs"] == episodes[1]["agent_msgs"]).all() and saved["e0_o0_pos"].dtype == np.float64


def test_record_arguments():
    check_record_args(False)
    check_record_args(True, "c.json", "t.npz", "frames", 4)
    for kw in (dict(curves_out="c.json"), dict(trace_out="t.npz"), dict(render_out="frames")):
        with pytest.raises(ValueError, match="spread"):
            check_record_args(False, **kw)
    with pytest.raises(ValueError, match="trace_envs"):
        check_record_args(True, trace_out="t.npz", trace_envs=0)
    assert len(FIELDS) == _lib.RR_FIELDS


def test_abi_sizeof_and_argument_errors():
    """``mel_abi_sizeof`` id 15 against the ctypes twin, and every argument error of the two entry points: all of them are
    returned before anything is launched, so made-up (never dereferenced) pointers do."""
    import ctypes as C
    lib = _lib.load()
    assert C.sizeof(_lib.MelRoundRecord) == lib.mel_abi_sizeof(15) == 208
    fake = 0x10000
    pointers = [name for name, kind in _lib.MelRoundRecord._fields_ if kind is C.c_void_p and name != "quota"]

    def record(**kw):
        r = _lib.MelRoundRecord()
        for name in pointers:
            setattr(r, name, fake)
        r.n_envs, r.n_nodes, r.max_rounds, r.n_trace, r.trace_capacity = 4, 20, 8, 0, 0
        for k, v in kw.items():
            if k == "trace_env":
                for i, t in enumerate(v):
                    r.trace_env[i] = t
            else:
                setattr(r, k, v)
        return r

    env = _lib.MelEnvBatch()
    env.n_envs, env.n_nodes, env.log_capacity = 4, 20, 64
    for name in ("scalars", "node_sets", "sel_sets", "pos", "one_hop", "agent_msgs", "received", "log_cursor", "log_stats", "log_meta"):
        setattr(env, name, fake)
    round_, read = lib.mel_round_record_round, lib.mel_round_record_read

    def refused(r, word):
        ref = C.byref(r) if r is not None else None
        for st in (round_(ref, C.byref(env), None), read(ref, fake, fake, fake, None)):
            assert st == _lib.ERR_INVALID_ARG and word.encode() in lib.mel_last_error(), (word, lib.mel_last_error())

    refused(None, "null")
    for name in ("running", "ended", "seen", "last", "overflow", "skipped", "unlogged"):
        refused(record(**{name: None}), "null buffer")
    refused(record(max_rounds=0), "max_rounds")
    refused(record(max_rounds=_lib.RR_MAX_ROUNDS + 1), "max_rounds")
    refused(record(n_trace=-1), "n_trace")
    refused(record(n_trace=_lib.RR_MAX_TRACE + 1), "n_trace")
    refused(record(n_trace=1, trace_capacity=0, trace_env=[0]), "trace_capacity")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[0, 4]), "outside")
    refused(record(n_trace=1, trace_capacity=4, trace_env=[-1]), "outside")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[1, 1]), "twice")
    for name in ("trace_cursor", "trace_meta", "trace_pos", "trace_one_hop", "trace_sets", "trace_agent_msgs", "trace_received"):
        refused(record(n_trace=1, trace_capacity=4, trace_env=[0], **{name: None}), "trace sink")
    # the env batch: null, unbound, other sizes (the round entry point only)
    assert round_(C.byref(record()), None, None) == _lib.ERR_INVALID_ARG and b"env is null" in lib.mel_last_error()
    assert round_(C.byref(record()), C.byref(_lib.MelEnvBatch()), None) == _lib.ERR_INVALID_ARG
    assert round_(C.byref(record(n_envs=5)), C.byref(env), None) == _lib.ERR_INVALID_ARG and b"envs" in lib.mel_last_error()
    assert round_(C.byref(record(n_nodes=21)), C.byref(env), None) == _lib.ERR_INVALID_ARG
    env.log_capacity = 0
    assert round_(C.byref(record()), C.byref(env), None) == _lib.ERR_INVALID_ARG and b"episode log" in lib.mel_last_error()
    env.log_capacity = 64
    # the read entry point's outputs
    for outs in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert read(C.byref(record()), *outs, None) == _lib.ERR_INVALID_ARG and b"null output" in lib.mel_last_error()


def test_watch_flags_need_spread(capsys):
    from melissa_amd import watch
    with pytest.raises(SystemExit):
        watch.parse_args(["--curves-out", "c.json"])
    assert "spread" in capsys.readouterr().err
    a = watch.parse_args(["--spread", "--curves-out", "c.json", "--trace-out", "t.npz", "--trace-envs", "2", "--render-out", "d"])
    assert (a.curves_out, a.trace_out, a.trace_envs, a.render_out) == ("c.json", "t.npz", 2, "d")
