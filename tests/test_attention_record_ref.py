"""CPU checks of the attention recorder's host side (melissa_amd/attention_record.py) and of the references the GPU tests hold
the device to (tests/attention_record_ref.py): the coefficient references against each other and against the oracle's dense
softmax, the measurement behind the two bounds, the booking rules on hand examples with known sums, ``summarise_attention`` on
hand tables, the ``watch`` argument errors, and every argument error of the three entry points (all of them returned before
anything is launched)."""
import math

import numpy as np
import pytest

from melissa_amd import _lib
from melissa_amd.attention_record import (FIELDS, check_attention_args, group_attention_episodes, save_attention_traces,
                                          summarise_attention)
from tests import attention_record_ref as ar
from tests.attention_record_ref import AttentionRecordModel, members, pack

N = 5


def state(B=2, num_moves=(1, 2), episodes_done=(0, 0), error=(0, 0), scripted=((), ()), has=((), ()), interested=((), ()),
          degree=None):
    sc = np.zeros((B, 16), dtype=np.int32)
    sc[:, _lib.S_NUM_MOVES], sc[:, _lib.S_EPISODES_DONE], sc[:, _lib.S_ERROR] = num_moves, episodes_done, error
    sc[:, _lib.S_EPISODE] = 40 + np.arange(B)
    ns = np.zeros((B, 8, 1), dtype=np.uint64)
    for b in range(B):
        ns[b, _lib.SET_SCRIPTED], ns[b, _lib.SET_HAS_MESSAGE], ns[b, _lib.SET_INTERESTED] = \
            pack(scripted[b], N), pack(has[b], N), pack(interested[b], N)
    degree = np.array([[1, 2, 2, 0, 7]] * B, dtype=np.float32) if degree is None else np.asarray(degree, dtype=np.float32)
    return dict(scalars=sc, node_sets=ns, sel_sets=np.zeros((B, 4, 1), dtype=np.uint64), degree=degree)


# env 0: nodes 1 and 3 decide (rows 0, 1); env 1: nodes 0, 2, 4 (rows 2, 3, 4)
LIVE = np.stack([pack([1, 3], N), pack([0, 2, 4], N)])
OFFSETS = np.array([0, 2, 5], dtype=np.int32)


def rows(H, *specs):
    """alpha float32 [rows, 34, H] and sources uint64 [rows, 1] from one (source ids, [c, H] coefficients) pair per row."""
    alpha, sources = np.zeros((len(specs), ar.MAX_SOURCES, H), dtype=np.float32), np.zeros((len(specs), 1), dtype=np.uint64)
    for r, (ids, a) in enumerate(specs):
        sources[r] = pack(ids, N)
        if len(ids):
            alpha[r, :len(ids)] = np.asarray(a, dtype=np.float32).reshape(len(ids), H)
    return alpha, sources


THIRD = np.float32(1.0) / np.float32(3.0)


def test_uniform_attention_over_three_sources():
    """Fields (1, 1/3, c/3, c/3, w/3, w/3, 1/3, 1/3) with c informed and w waiting neighbours: every value the float32 third
    widened, summed as the device sums it."""
    t = np.float64(THIRD)
    for has, interested, c, w in (((0, 2), (0, 2, 4), 2, 0), ((0,), (0, 2), 1, 1), ((), (), 0, 0), ((1,), (1, 2), 0, 1)):
        m = AttentionRecordModel(2, N, max_rounds=4, n_degrees=3, heads=2)
        alpha, sources = rows(2, ([0, 1, 2], np.full((3, 2), THIRD)), ([], None), ([], None), ([], None), ([], None))
        m.launch(state(has=(has, ()), interested=(interested, ())), LIVE, alpha, sources, OFFSETS)
        informed = (t + t) if c == 2 else t if c == 1 else 0.0
        waiting = t if w == 1 else 0.0
        want = [1.0, t, informed, c / 3, waiting, w / 3, t * t + t * t + t * t, t]
        np.testing.assert_array_equal(m.by_head[0, 0], np.array(want) + [1, 0, 0, 0, 0, 0, 0, 0])        # + node 3's empty row
        np.testing.assert_array_equal(m.by_head[0, 1], m.by_head[0, 0])
        # the head mean of two equal heads is the value itself; node 1 (degree 2 -> row 2), node 3 (degree 0, no source)
        np.testing.assert_array_equal(m.by_degree[0, 2], want)
        np.testing.assert_array_equal(m.by_degree[0, 0], [1, 0, 0, 0, 0, 0, 0, 0])
        np.testing.assert_array_equal(m.by_round[0, 1], np.array(want) + [1, 0, 0, 0, 0, 0, 0, 0])
        assert abs(m.by_degree[0, 2, 6] - 1 / 3) < 1e-7 and m.booked[0] == (0, 1, 3, c, w)


def test_one_hot_attention_and_the_head_mean():
    """Head 0 gives everything to the informed neighbour 2, head 1 everything to the node itself."""
    m = AttentionRecordModel(2, N, max_rounds=4, n_degrees=8, heads=2)
    alpha, sources = rows(2, ([], None), ([], None), ([], None), ([0, 2, 3], [[0, 0], [1, 1], [0, 0]]), ([2, 4], [[1, 0], [0, 1]]))
    m.launch(state(has=((), (2,)), interested=((), (2, 3))), LIVE, alpha, sources, OFFSETS)
    # node 2 (row 3): itself in both heads; node 4 (row 4): head 0 -> node 2 (informed), head 1 -> itself
    np.testing.assert_array_equal(m.by_head[1, 0], [3, 1, 1, 0.5, 0, 1 / 3, 2, 2])
    np.testing.assert_array_equal(m.by_head[1, 1], [3, 2, 0, 0.5, 0, 1 / 3, 2, 2])
    np.testing.assert_array_equal(m.by_degree[1, 7], [1, 0.5, 0.5, 0.5, 0, 0, 1, 1])                # node 4, degree 7
    np.testing.assert_array_equal(m.by_degree[1, 2], [1, 1, 0, 0, 0, 1 / 3, 1, 1])                  # node 2: waiting node 3 of 3
    np.testing.assert_array_equal(m.by_degree[1, 1], [1, 0, 0, 0, 0, 0, 0, 0])                      # node 0: no source
    assert m.by_round[1, 2, 0] == 3 and not m.by_round[0, 1, 1:].any() and m.by_round[0, 1, 0] == 2


def test_a_decision_without_sources_books_the_count_alone_and_the_trace():
    m = AttentionRecordModel(2, N, max_rounds=4, n_degrees=3, heads=3, trace_envs=(1,), trace_capacity=2)
    alpha, sources = rows(3, ([], None), ([], None), ([], None), ([2], [[1, 1, 1]]), ([], None))
    alpha[4, :3] = 0.25                                                  # coefficients of a row without sources are not read
    m.launch(state(), LIVE, alpha, sources, OFFSETS)
    np.testing.assert_array_equal(m.by_round[1, 2], [3, 1, 0, 0, 0, 0, 1, 1])
    np.testing.assert_array_equal(m.by_head[1].sum(0), [9, 3, 0, 0, 0, 0, 3, 3])
    assert m.cursor.tolist() == [1] and m.ring["meta"][0, 0].tolist() == [1, 0, 41, 2, 3, 2, 0, 0]
    assert members(m.ring["sets"][0, 0], N) == [0, 2, 4]
    np.testing.assert_array_equal(m.ring["fields"][0, 0, :, 0], [1, 0, 1, 0, 1])
    np.testing.assert_array_equal(m.ring["fields"][0, 0, 2], [1, 1, 0, 0, 0, 0, 1, 1])
    for _ in range(2):                                                   # the ring of two wraps
        m.launch(state(), LIVE, alpha, sources, OFFSETS)
    assert m.cursor.tolist() == [3] and len(m.all_records[1]) == 3 and m.by_round[1, 2, 0] == 9


def test_scripted_quota_error_overflow_and_the_last_degree_row():
    alpha, sources = rows(1, *[([0, 1, 2, 3, 4], np.full((5, 1), 0.2))] * 5)
    m = AttentionRecordModel(2, N, max_rounds=2, n_degrees=2, heads=1, quota=[1, 1])
    m.launch(state(scripted=((1,), ())), LIVE, alpha, sources, OFFSETS)
    assert m.by_round[0, 1, 0] == 1 and [b[:2] for b in m.booked] == [(0, 3), (1, 0), (1, 2), (1, 4)]      # node 1 is scripted
    assert m.overflow.tolist() == [0, 3] and not m.by_round[1].any()     # env 1 stands at round 2 >= max_rounds
    np.testing.assert_array_equal(m.by_degree[:, :, 0], [[1, 0], [0, 3]])            # degrees 1, 2 and 7 share the last row
    assert m.by_head[1, 0, 0] == 3
    m.launch(state(episodes_done=(1, 0), error=(0, 4)), LIVE, alpha, sources, OFFSETS)      # quota met; in error
    assert m.by_degree[:, :, 0].sum() == 4 and m.skipped.tolist() == [0, 1]
    m.launch(state(episodes_done=(5, 0), error=(2, 0), num_moves=(1, 0)), LIVE, alpha, sources, OFFSETS)   # the error counts first
    assert m.skipped.tolist() == [1, 1] and m.by_round[1, 0, 0] == 3
    by_round, by_degree, by_head, counters = m.folded()
    assert counters == dict(overflow=3, skipped=2) and by_head[0, 0] == 7 and by_degree[:, 0].tolist() == [1, 6]


def test_alpha_references_agree_and_match_the_oracles_dense_softmax():
    """alpha64 against the oracle's dense conv2 coefficients (float64, full graphs); alpha32 within ALPHA_TOL of alpha64."""
    import torch
    for cell in (ar.CELLS[0], ar.CELLS[-1]):
        hidden, heads, model, n, bs = cell
        _obs, live = ar.cell_inputs(n, bs)
        keys, values, queries, att, bias, adj = ar.conv2_rows64(cell)
        src = ar.source_sets(adj, model == "l_dgn")
        e = np.zeros((bs, n, n, heads))
        for b, i in ar.agent_rows(live):
            js = np.flatnonzero(src[b, i])
            a = ar.alpha64(keys[b, js], queries[b, i], att, heads)
            assert a.shape == (len(js), heads)
            if len(js):
                np.testing.assert_allclose(a.sum(0), 1.0, rtol=0, atol=1e-12)
                x = torch.from_numpy
                k, q = x(keys).reshape(bs, n, heads, -1), x(queries).reshape(bs, n, heads, -1)
                if model == "l_dgn":
                    z = q[b, i][None] + k[b, js]
                    e = (torch.where(z > 0, z, 0.2 * z) * x(att).reshape(1, heads, -1)).sum(-1)
                else:
                    e = (k[b, js] * q[b, i][None]).sum(-1) / math.sqrt(hidden)
                np.testing.assert_allclose(a, torch.softmax(e, 0).numpy(), rtol=0, atol=1e-12)
                a32 = ar.alpha32(keys[b, js], queries[b, i], att, heads)
                assert a32.dtype == np.float32 and np.abs(a32 - a).max() < 1e-5
            else:
                assert model == "dgn_r" and (b, i) == (0, 0)             # the isolated agent of the TransformerConv cell
    assert (ar.alpha64(np.zeros((0, 8)), np.zeros(8), None, 2).shape, ar.alpha32(np.zeros((0, 8)), np.zeros(8), None, 2).shape) == ((0, 2), (0, 2))


def test_cells_hold_what_the_gpu_tests_need():
    for cell in ar.CELLS:
        hidden, heads, model, n, bs = cell
        obs, live = ar.cell_inputs(n, bs)
        counts = ar.source_sets(ar.adjacency(obs, n), model == "l_dgn").sum(2)
        if n > 64:
            assert live[0].all() and counts[0].max() == ar.MAX_SOURCES and live[1].sum() == 4 and live[1, 64:].any()
        else:
            assert live.sum(1).tolist() == [1, n, 0, 4] and counts[0, 0] == (1 if model == "l_dgn" else 0)
            assert counts[1].min() >= 3
    assert ar.cell_inputs(*ar.TABLE_CELL[3:])[1].any(1).all()


def test_bounds_are_eight_times_the_measured_error():
    """The measurement behind ALPHA_TOL and X3_TOL: the float32 restatements against float64 on the GPU tests' own cells."""
    worst_a = worst_x = 0.0
    for cell in ar.CELLS:
        a, x = ar.measure(cell)
        print(f"{ar.cell_id(cell)}: alpha32 - alpha64 {a:.3e}, x3_32 - x3_64 {x:.3e}")
        worst_a, worst_x = max(worst_a, a), max(worst_x, x)
    print(f"largest: alpha {worst_a:.3e} (ALPHA_TOL {ar.ALPHA_TOL:.1e}), x_3 {worst_x:.3e} (X3_TOL {ar.X3_TOL:.1e})")
    for tol, measured in ((ar.ALPHA_TOL, worst_a), (ar.X3_TOL, worst_x)):
        assert 0.8 * 8 * measured <= tol <= 8 * measured, (tol, measured)      # never above 8 x: the constants are rounded down


def test_summarise_attention_on_hand_tables():
    by_round = np.zeros((3, 8))
    by_round[1] = [4, 1.0, 2.0, 1.0, 0.5, 1.0, 2.0, 3.0]
    by_degree = np.zeros((2, 8))
    by_degree[0], by_degree[1] = [1, 0.25, 0.5, 0.5, 0.25, 0.25, 0.5, 0.5], [3, 0.75, 1.5, 0.5, 0.25, 0.75, 1.5, 2.5]
    by_head = np.zeros((2, 8))
    by_head[0] = [4, 2.0, 1.0, 1.0, 0, 0, 4.0, 4.0]
    s = summarise_attention(by_round, by_degree, by_head)
    assert s["rounds"].tolist() == [0, 1, 2] and s["degrees"].tolist() == [0, 1] and s["heads"].tolist() == [0, 1]
    r = s["by_round"]
    assert r["decisions"].tolist() == [0, 4, 0]
    for key, want in (("self_mean", 0.25), ("informed_mean", 0.5), ("informed_share_mean", 0.25), ("waiting_mean", 0.125),
                      ("waiting_share_mean", 0.25), ("squares_mean", 0.5), ("max_mean", 0.75), ("informed_lift", 2.0),
                      ("waiting_lift", 0.5), ("effective_neighbours", 2.0)):
        assert r[key][1] == want, key
        assert math.isnan(r[key][0]) and math.isnan(r[key][2]), key
    h = s["by_head"]
    assert h["effective_neighbours"][0] == 1.0 and math.isnan(h["waiting_lift"][0]) and math.isnan(h["self_mean"][1])
    assert s["total"]["decisions"] == 4.0 and s["total"]["informed_lift"] == 2.0 and s["total"]["waiting_lift"] == 0.5
    empty = summarise_attention(np.zeros((2, 8)), np.zeros((1, 8)), np.zeros((1, 8)))
    assert empty["total"]["decisions"] == 0.0 and all(math.isnan(v) for k, v in empty["total"].items() if k != "decisions")
    with pytest.raises(ValueError, match="by_head"):
        summarise_attention(np.zeros((2, 8)), np.zeros((2, 8)), np.zeros((2, 7)))
    assert len(FIELDS) == _lib.AR_FIELDS == ar.FIELDS and _lib.ATT_MAX_SOURCES == ar.MAX_SOURCES


def test_records_group_by_episode_ordinal_and_save(tmp_path):
    m = AttentionRecordModel(2, N, max_rounds=4, n_degrees=3, heads=1, trace_envs=(1,))
    alpha, sources = rows(1, *[([0, 2], [[0.5], [0.5]])] * 5)
    for ep, mv in ((0, 0), (0, 1), (1, 0)):
        m.launch(state(num_moves=(0, mv), episodes_done=(0, ep)), LIVE, alpha, sources, OFFSETS)
    episodes = group_attention_episodes(m.all_records[1])
    assert [(e["env"], e["ordinal"], e["pool_episode"], e["rounds"].tolist()) for e in episodes] == [(1, 0, 41, [0, 1]), (1, 1, 41, [0])]
    assert episodes[0]["fields"].shape == (2, N, 8) and episodes[0]["sets"].shape == (2, 1)
    assert episodes[0]["decisions"].tolist() == [3, 3] and episodes[0]["without_sources"].tolist() == [0, 0]
    out = tmp_path / "a.npz"
    save_attention_traces(str(out), {1: episodes})
    saved = np.load(str(out))
    assert sorted(saved.files) == sorted(f"e1_o{o}_{k}" for o in (0, 1) for k in episodes[0])
    assert (saved["e1_o0_fields"] == episodes[0]["fields"]).all() and saved["e1_o1_sets"].dtype == np.uint64


def test_attention_arguments():
    check_attention_args(False)
    check_attention_args(False, model="hl_dgn", feature_dtype="bf16")        # nothing asked for: nothing to refuse
    check_attention_args(True, "a.json", "t.npz", 4, model="l_dgn", feature_dtype="f32a")
    for kw in (dict(attention_curves_out="a.json"), dict(attention_trace_out="t.npz")):
        with pytest.raises(ValueError, match="spread"):
            check_attention_args(False, **kw)
        with pytest.raises(ValueError, match="HL-DGN"):
            check_attention_args(True, model="hl_dgn", **kw)
        with pytest.raises(ValueError, match="bf16"):
            check_attention_args(True, model="dgn_r", feature_dtype="bf16", **kw)
    with pytest.raises(ValueError, match="trace_envs"):
        check_attention_args(True, attention_trace_out="t.npz", trace_envs=17)


def test_watch_flags_need_spread(capsys):
    from melissa_amd import watch
    for flags in (["--attention-curves-out", "a.json"], ["--attention-trace-out", "t.npz"]):
        with pytest.raises(SystemExit):
            watch.parse_args(flags)
        assert "spread" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        watch.parse_args(["--spread", "--model", "hl_dgn", "--attention-curves-out", "a.json"])
    assert "HL-DGN" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        watch.parse_args(["--spread", "--dtype", "bf16", "--attention-curves-out", "a.json"])
    assert "bf16" in capsys.readouterr().err
    a = watch.parse_args(["--spread", "--attention-curves-out", "a.json", "--attention-trace-out", "t.npz", "--trace-envs", "2"])
    assert (a.attention_curves_out, a.attention_trace_out, a.trace_envs) == ("a.json", "t.npz", 2)
    assert not hasattr(watch.parse_args(["--spread"]), "attention_curves_out")     # a plain call's namespace is what it was
    # the function refuses at argument time too: before a network or an env is built
    with pytest.raises(ValueError, match="spread"):
        watch.watch(model="l_dgn", n_nodes=20, envs=1, episodes=2, attention_curves_out="a.json", device="no-such-device")
    with pytest.raises(ValueError, match="HL-DGN"):
        watch.watch(model="hl_dgn", n_nodes=20, envs=1, episodes=2, spread=True, attention_trace_out="t.npz", device="no-such-device")


def test_abi_sizeof_and_argument_errors():
    """``mel_abi_sizeof`` id 17 against the ctypes twin, and every argument error of the three entry points: all of them are
    returned before anything is launched, so made-up (never dereferenced) pointers do."""
    import ctypes as C
    lib = _lib.load()
    assert C.sizeof(_lib.MelAttentionRecord) == lib.mel_abi_sizeof(17) == 176 and lib.mel_abi_sizeof(18) == 0
    for name in ("mel_forward_attention", "mel_attention_record_round", "mel_attention_record_read"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    fake = 0x10000
    pointers = [name for name, kind in _lib.MelAttentionRecord._fields_ if kind is C.c_void_p and name != "quota"]

    def record(**kw):
        r = _lib.MelAttentionRecord()
        for name in pointers:
            setattr(r, name, fake)
        r.n_envs, r.n_nodes, r.max_rounds, r.n_degrees, r.n_heads, r.n_trace, r.trace_capacity = 4, 20, 8, 20, 4, 0, 0
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
    read = lib.mel_attention_record_read

    def round_(ref, env_ref, alpha=fake, sources=fake, offsets=fake, live=fake, heads=4):
        return lib.mel_attention_record_round(ref, env_ref, alpha, sources, offsets, live, heads, None)

    def refused(r, word):
        ref = C.byref(r) if r is not None else None
        for st in (round_(ref, C.byref(env)), read(ref, fake, fake, fake, fake, None)):
            assert st == _lib.ERR_INVALID_ARG and word.encode() in lib.mel_last_error(), (word, lib.mel_last_error())

    refused(None, "null")
    for name in ("by_round", "by_degree", "by_head", "overflow", "skipped"):
        refused(record(**{name: None}), "null buffer")
    refused(record(max_rounds=0), "max_rounds")
    refused(record(max_rounds=_lib.DR_MAX_ROUNDS + 1), "max_rounds")
    refused(record(n_degrees=0), "n_degrees")
    refused(record(n_degrees=_lib.DR_MAX_DEGREES + 1), "n_degrees")
    refused(record(n_heads=0), "n_heads")
    refused(record(n_heads=_lib.AR_MAX_HEADS + 1), "n_heads")
    refused(record(n_trace=-1), "n_trace")
    refused(record(n_trace=_lib.DR_MAX_TRACE + 1), "n_trace")
    refused(record(n_trace=1, trace_capacity=0, trace_env=[0]), "trace_capacity")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[0, 4]), "outside")
    refused(record(n_trace=2, trace_capacity=4, trace_env=[1, 1]), "twice")
    for name in ("trace_cursor", "trace_meta", "trace_sets", "trace_fields"):
        refused(record(n_trace=1, trace_capacity=4, trace_env=[0], **{name: None}), "trace sink")
    ok = C.byref(record())
    assert round_(ok, None) == _lib.ERR_INVALID_ARG and b"env is null" in lib.mel_last_error()
    assert round_(ok, C.byref(_lib.MelEnvBatch())) == _lib.ERR_INVALID_ARG and b"not bound" in lib.mel_last_error()
    assert round_(C.byref(record(n_envs=5)), C.byref(env)) == _lib.ERR_INVALID_ARG and b"envs" in lib.mel_last_error()
    assert round_(C.byref(record(n_nodes=21)), C.byref(env)) == _lib.ERR_INVALID_ARG
    for kw in (dict(alpha=None), dict(sources=None), dict(offsets=None), dict(live=None)):
        assert round_(ok, C.byref(env), **kw) == _lib.ERR_INVALID_ARG and b"null input" in lib.mel_last_error()
    assert round_(ok, C.byref(env), heads=2) == _lib.ERR_INVALID_ARG and b"heads" in lib.mel_last_error()
    for outs in ((None, fake, fake, fake), (fake, None, fake, fake), (fake, fake, None, fake), (fake, fake, fake, None)):
        assert read(ok, *outs, None) == _lib.ERR_INVALID_ARG and b"null output" in lib.mel_last_error()
    # mel_forward_attention: null arguments, sizes, HL-DGN weights, bf16 rows
    fwd = lib.mel_forward_attention
    w = _lib.MelWeights()
    w.model, w.precision = _lib.MODEL_LDGN, _lib.PREC_F32
    w.conv2.heads, w.conv2.channels, w.conv2.kind = 4, 128, _lib.CONV_GATV2
    for args in ((None, 4, 20, 80, fake, fake, fake), (C.byref(w), 4, 20, 80, None, fake, fake),
                 (C.byref(w), 4, 20, 80, fake, None, fake), (C.byref(w), 4, 20, 80, fake, fake, None)):
        assert fwd(*args, None) == _lib.ERR_INVALID_ARG and b"null argument" in lib.mel_last_error()
    for bs, n, cap in ((0, 20, 80), (4, 0, 80), (4, _lib.MAX_NODES + 1, 80), (4, 20, 0), (4, 20, 81)):
        assert fwd(C.byref(w), bs, n, cap, fake, fake, fake, None) == _lib.ERR_INVALID_ARG and b"rows_cap" in lib.mel_last_error()
    w.model = _lib.MODEL_HLDGN
    assert fwd(C.byref(w), 4, 20, 80, fake, fake, fake, None) == _lib.ERR_UNSUPPORTED and b"second convolution" in lib.mel_last_error()
    w.model, w.precision = _lib.MODEL_DGNR, _lib.PREC_BF16
    assert fwd(C.byref(w), 4, 20, 80, fake, fake, fake, None) == _lib.ERR_UNSUPPORTED and b"bf16" in lib.mel_last_error()
