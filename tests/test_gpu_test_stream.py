"""GPU parity of the evaluation schedule on the device (csrc/episode_stream.hpp's testing mode,
melissa_amd/env/stream.py ``TestEpisodeStream``, ``melissa_amd.collect.evaluate_spread``): the device reads the seed list
and draws, bit for bit, what World.reset draws with ``is_testing`` (core.py:182-187,348-370) - checked against
``EpisodeSampler``, the numpy restatement the golden env traces pin to the real reference - for a list walked whole and a list
spread over the envs; and an evaluation spread over several envs and replayed from a HIP graph reports, position by
position, the episodes the one-env evaluation plays one after another."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.trace_replay import set_int      # node sets (uint64 scalar, or words beyond 64 nodes) -> int
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


# (n, graphs, T, dynamic, spread, discard, scripted ratio)
DRAW_CASES = [(20, 5, 7, True, False, 0, 0.0),          # T neither divides nor is divided by the ring; wraps several times
              (20, 5, 7, True, True, 0, 0.0),
              (20, 5, 7, True, False, 2, 0.0),
              (20, 5, 7, True, False, 0, 0.3),
              (12, 1, 10, True, False, 0, 0.0),         # a pool of one graph: no graph draw
              (70, 3, 5, False, False, 0, 0.0),         # static, two-word node sets
              (100, 4, 12, True, False, 0, 0.0),
              (100, 4, 12, True, True, 0, 0.0)]


@pytest.mark.parametrize("n,n_graphs,T,dynamic,spread,discard,ratio", DRAW_CASES)
def test_device_schedule_matches_numpy_protocol(n, n_graphs, T, dynamic, spread, discard, ratio):
    from melissa_amd import _lib as L
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.env.episodes import movement_offsets
    from melissa_amd.env.stream import TestEpisodeStream
    B, K, seed, max_moves = 9, 5, 123, 7
    graphs = synthetic_graph_pool(n, n_graphs, first_seed=3)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=dynamic, device="cuda", max_moves=max_moves,
                             construct_like_reference=False, is_testing=True, num_test_episodes=T,
                             scripted_agents_ratio=ratio, spread_test_episodes=spread)
    total = 4 * K + 3
    want = []
    for b in range(B):
        sampler = venv.make_sampler(seed + b, env=b)
        want.append([sampler.sample() for _ in range(total + discard)])
    st = TestEpisodeStream(venv, seed, ring=K, discard=discard)
    assert (int(st.struct.test_env_step), int(st.struct.test_episode_step)) == ((1, B) if spread else (0, 1))
    cursor = venv.scalars()[:, L.S_EP_CURSOR]
    checked = 0
    for cur in range(0, total - K + 2):
        cursor.fill_(cur)                      # pretend every env has started `cur` episodes
        st.refill()
        torch.cuda.synchronize()
        produced = st.produced.cpu().numpy()
        assert (produced == cur + K - 1).all()
        t = {k: v.cpu().numpy() for k, v in st.pool.tensors.items()}
        for b in range(B):
            for j in range(max(0, cur - 1), cur + K - 1):          # every live slot of the ring
                slot = b * K + j % K
                ep = want[b][j + discard]
                g = graphs[ep.graph_index]
                assert t["origin"][slot] == ep.origin and set_int(t["interested"][slot]) == ep.interested, (b, j)
                assert set_int(t["scripted"][slot]) == ep.scripted, (b, j)
                np.testing.assert_array_equal(t["pos"][slot], g.pos)
                np.testing.assert_array_equal(t["one_hop"][slot].view(np.uint64), g.one_hop)
                if dynamic:
                    np.testing.assert_array_equal(t["moves"][slot], movement_offsets(ep.movement_seed, n, max_moves))
                checked += 1
    assert checked > 100
    assert (st.test_discarded.cpu().numpy() == discard).all()
    # the envs' generators: only the scripted sets were drawn from them - no episode seed, no graph
    pcg = st.pcg.cpu().numpy().view(np.uint64)
    half = st.pcg_half.cpu().numpy().view(np.uint32)
    k_scripted = int(round(ratio * n))
    for b in range(B):
        gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b)))
        sampler = venv.make_sampler(seed + b, env=b)
        for _ in range(int(st.produced[b]) + discard):
            sampler.sample()
            if k_scripted:
                gen.choice(n, size=k_scripted, replace=False)
        ref = sampler.np_random.bit_generator.state
        assert ref == gen.bit_generator.state
        assert (int(pcg[b, 1]) << 64 | int(pcg[b, 0])) == ref["state"]["state"]
        assert int(half[b, 0]) == ref["has_uint32"] and (not ref["has_uint32"] or int(half[b, 1]) == ref["uinteger"])


@pytest.mark.parametrize("T", [1, 10, 700])          # 700 crosses a regeneration of the 624-word key
def test_seed_list_is_randomstate_17(T):
    from melissa_amd import _lib as L
    out = torch.zeros(T, dtype=torch.int32, device="cuda")
    L.check(L.load().mel_episode_test_seeds(out.data_ptr(), T, L.current_stream_ptr(out.device)), "mel_episode_test_seeds")
    gen = np.random.RandomState(17)
    want = [gen.randint(0, 1e9) for _ in range(T)]
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), np.asarray(want, dtype=np.uint32))


# ---- a spread evaluation against the one-env evaluation ------------------------------------------------------------------
SEED = 9


@functools.lru_cache(maxsize=None)
def _policy(model, n):
    from melissa_amd.networks import HLDGNNetwork, LDGNNetwork
    from melissa_amd.policy import DQNPolicy
    torch.manual_seed(5)
    if model == "l_dgn":
        net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip")
    else:
        net = HLDGNNetwork(5, 128, 2, 4, n, aggregator="max", dueling_param=DUEL(), device="cuda", backend="hip")
    net.eval()
    net.set_feature_dtype("f32")
    return DQNPolicy(net)


def _venv(n, envs, T, spread):
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    return HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 3, first_seed=0), dynamic_graph=True, device="cuda",
                             max_moves=64, seed=SEED, construct_like_reference=False, is_testing=True, num_test_episodes=T,
                             spread_test_episodes=spread)


@functools.lru_cache(maxsize=None)
def _one_env_reference(model, n, T):
    """The existing path: one env, a host-drawn static table, eager rounds; the first T rows are list positions 0 .. T-1."""
    from melissa_amd.collect import Collector
    from melissa_amd.env.stream import StaticSupply
    col = Collector(_policy(model, n), _venv(n, 1, T, False), episodes_per_env=T + 2, seed=SEED, eps=0.0, chunk=4,
                    use_graph=False)
    res = col.collect(n_episode=T)
    assert isinstance(col.loop.supply, StaticSupply)
    assert len(res.returns) >= T
    info = {k: v[:T].copy() for k, v in res.episode_info.items()}
    return res.returns[:T].copy(), res.lens[:T].copy(), info


def _assert_same_episodes(res, positions, ref, T):
    from melissa_amd import _lib as L
    returns, lens, info = ref
    np.testing.assert_array_equal(positions, np.arange(T))
    assert res.n_collected_episodes == T and len(res.returns) == len(res.lens) == T
    assert set(res.episode_info) == set(L.LOGGER_KEYS) and len(L.LOGGER_KEYS) == 10
    for k in L.LOGGER_KEYS:
        np.testing.assert_array_equal(res.episode_info[k], info[k], err_msg=k)
    np.testing.assert_array_equal(res.lens, lens)
    np.testing.assert_array_equal(res.returns, returns)


@pytest.mark.parametrize("model,n,T,B", [("l_dgn", 12, 10, 4), ("hl_dgn", 12, 10, 4), ("l_dgn", 70, 5, 2)])
def test_spread_evaluation_equals_one_env_evaluation(model, n, T, B):
    from melissa_amd.collect import evaluate_spread, test_shares
    from melissa_amd.env.stream import TestEpisodeStream
    ref = _one_env_reference(model, n, T)
    assert len(set(ref[1].tolist())) > 1 or len(set(ref[0].tolist())) > 1          # the positions are told apart
    if (T, B) == (10, 4):
        assert test_shares(T, B) == [3, 3, 2, 2]
    venv = _venv(n, B, T, True)
    res, positions = evaluate_spread(_policy(model, n), venv, T, eps=0.0, seed=SEED, use_graph=True)
    _assert_same_episodes(res, positions, ref, T)
    assert venv.scalars()[:, 11].cpu().numpy().max() == 0                          # MEL_S_ERROR


def test_spread_evaluation_clamps_to_the_list_and_repeats():
    """More envs than list positions: the envs beyond the list own nothing.  A second call on the same envs starts from the
    top of the list again and reports the same rows."""
    from melissa_amd.collect import evaluate_spread, test_shares
    model, n, T, B = "l_dgn", 12, 10, 16
    assert test_shares(T, B) == [1] * 10 + [0] * 6
    ref = _one_env_reference(model, n, T)
    venv = _venv(n, B, T, True)
    for _ in range(2):
        res, positions = evaluate_spread(_policy(model, n), venv, T, eps=0.0, seed=SEED, use_graph=True)
        _assert_same_episodes(res, positions, ref, T)


def test_spread_evaluation_refuses_a_full_log_and_other_envs():
    from melissa_amd.collect import evaluate_spread
    policy = _policy("l_dgn", 12)
    with pytest.raises(RuntimeError, match="episode log"):
        evaluate_spread(policy, _venv(12, 4, 10, True), 10, eps=0.0, seed=SEED, log_capacity=3)
    with pytest.raises(ValueError, match="spread_test_episodes"):
        evaluate_spread(policy, _venv(12, 4, 10, False), 10)
    with pytest.raises(ValueError, match="num_test_episodes"):
        evaluate_spread(policy, _venv(12, 4, 10, True), 8)


def test_train_evaluates_with_several_envs(tmp_path):
    """epochs[0] is evaluated before any update, from the same seed: three spread envs report what one env reports."""
    from melissa_amd import _lib as L
    from melissa_amd.train import train
    kw = dict(model="l_dgn", n_nodes=12, envs=8, epoch=1, step_per_epoch=300, test_num=6, eps_test=0.0, model_name="run",
              log=lambda line: None)
    spread = train(test_envs=3, logdir=str(tmp_path / "spread"), **kw)
    single = train(test_envs=1, logdir=str(tmp_path / "single"), **kw)
    a, b = spread["epochs"][0], single["epochs"][0]
    assert (a["test_envs"], b["test_envs"]) == (3, 1) and a["episodes"] == b["episodes"] == 6
    for k in ("test_rew", "test_len", *L.LOGGER_KEYS):
        assert a[k] == b[k], k
    assert all(e["test_envs"] == 3 for e in spread["epochs"]) and len(spread["epochs"]) == 2
    assert spread["errors"] == 0 and single["errors"] == 0


def test_watch_spread_plays_every_position_once():
    """``watch --envs E --spread`` reports the list itself, each position once: what one env reports that plays it in order."""
    from melissa_amd.watch import watch
    spread = watch(model="l_dgn", n_nodes=12, envs=4, episodes=6, seed=SEED, spread=True)
    walk = watch(model="l_dgn", n_nodes=12, envs=1, episodes=6, seed=SEED, spread=True)      # one env: the list in order
    assert spread["n/ep"] == walk["n/ep"] == 6
    for k in ("rew", "len", "coverage"):
        assert spread[k] == walk[k], k


def test_error_handling():
    from melissa_amd import _lib as L
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.env.stream import EpisodeStream, StaticSupply, TestEpisodeStream, make_supply
    graphs = synthetic_graph_pool(12, 3, first_seed=0)
    kw = dict(graph_pool=graphs, dynamic_graph=True, device="cuda", construct_like_reference=False)
    venv = HipGraphVectorEnv(4, 12, is_testing=True, num_test_episodes=7, **kw)
    with pytest.raises(ValueError, match="device sampler"):
        EpisodeStream(venv, 0)                                                   # the training stream still refuses the mode
    assert isinstance(make_supply(venv, 0, episodes_per_env=7), StaticSupply)    # and nobody gets the new one unasked
    with pytest.raises(ValueError, match="is_testing"):
        TestEpisodeStream(HipGraphVectorEnv(4, 12, **kw), 0)
    st = make_supply(venv, 0, stream="test", ring=5)
    assert isinstance(st, TestEpisodeStream) and st.describe()["walk"] == (0, 1)
    lib = L.load()
    call = lambda discard: lib.mel_episode_refill(C.byref(st.struct), C.byref(st.graphs), C.byref(st.pool.struct),
                                                  C.byref(venv.env), 5, discard, L.current_stream_ptr(venv.device))
    n_test = st.struct.n_test
    st.struct.n_test = 0
    assert call(0) == L.ERR_UNSUPPORTED                                          # testing mode without a schedule
    st.struct.n_test = n_test
    st.struct.test_env_step, st.struct.test_episode_step = 1, 4
    assert call(1) == L.ERR_INVALID_ARG and b"discard" in lib.mel_last_error()   # a spread list does not discard
    assert call(0) == L.OK
    torch.cuda.synchronize()
    spread = HipGraphVectorEnv(4, 12, is_testing=True, num_test_episodes=7, spread_test_episodes=True, **kw)
    with pytest.raises(ValueError, match="discard"):
        TestEpisodeStream(spread, 0, discard=1)
    with pytest.raises(ValueError, match="is_testing"):
        HipGraphVectorEnv(4, 12, spread_test_episodes=True, **kw)
