"""CPU side of the evaluation schedule on the device: where ``EpisodeSampler`` puts an env on the list of test seeds (the
oracle of ``mel_episode_refill``'s testing mode), how a spread list is shared out, the ABI fields, the argument checks that
need no GPU, and the command lines."""
import ctypes as C

import numpy as np
import pytest

N = 20


def _sampler(T, pool=5, n=N, ratio=0.0, seed=3, **kw):
    from melissa_amd.env.episodes import EpisodeSampler
    return EpisodeSampler(n, np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed))), pool, False, is_testing=True,
                          num_test_episodes=T, scripted_agents_ratio=ratio, **kw)


def _key(ep):
    return (ep.graph_index, ep.origin, ep.interested, ep.movement_seed)


def _density_count(t, T, n=N):
    """core.py:365-366: the density list is indexed with the list index AFTER it was bumped."""
    return int(((((t + 1) % T) % 10) + 1) / 10.0 * n)


@pytest.mark.parametrize("T", [7, 10, 13])
@pytest.mark.parametrize("B", [1, 4, 7])
def test_spread_sampler_plays_the_plain_samplers_positions(T, B):
    plain = [_key(ep) for ep in (lambda s: [s.sample() for _ in range(T)])(_sampler(T))]
    assert len(set(plain)) == T                                  # the positions are told apart by what is compared
    for b in range(B):
        s = _sampler(T, test_env=b, test_env_step=1, test_episode_step=B)
        for e in range(2 * T + 3):                               # past the end of the list: the walk wraps
            t = (b + e * B) % T
            assert s.test_position(e) == t
            ep = s.sample()
            assert _key(ep) == plain[t], (b, e, t)
            assert bin(ep.interested).count("1") == _density_count(t, T), (b, e, t)      # the density follows the position


def test_seven_episodes_cycle_the_density_from_the_second_entry():
    s = _sampler(7)
    assert [bin(s.sample().interested).count("1") for _ in range(7)] == [4, 6, 8, 10, 12, 14, 2]


@pytest.mark.parametrize("T", [1, 5, 7, 10, 13, 100])
@pytest.mark.parametrize("B", [1, 2, 4, 7, 10, 16])
def test_shares_cover_the_list_exactly_once(T, B):
    from melissa_amd.collect import test_shares
    shares = test_shares(T, B)
    assert len(shares) == B and sum(shares) == T
    played = []
    for b in range(B):
        assert shares[b] == (-(-(T - b) // B) if b < T else 0)
        s = _sampler(T, test_env=b, test_env_step=1, test_episode_step=B)
        played += [s.test_position(e) for e in range(shares[b])]
        assert played[len(played) - shares[b]:] == list(range(b, T, B))          # below T: no wrap inside a share
    assert sorted(played) == list(range(T))


def test_discarded_episodes_shift_the_walk():
    T, discard = 7, 2
    plain = [_key(_s) for _s in (lambda s: [s.sample() for _ in range(T)])(_sampler(T))]
    s = _sampler(T)
    for _ in range(discard):
        s.sample()
    for e in range(T + 2):
        assert _key(s.sample()) == plain[(e + discard) % T]


@pytest.mark.parametrize("ratio", [0.0, 0.3])
def test_defaults_reproduce_the_reference_walk(ratio):
    """The sampler's default placement against World.reset's own statement (core.py:351-366, 393-395): one index that is
    bumped modulo T before the density is read, the scripted set from the env's generator."""
    T, pool, seed = 7, 5, 11
    s = _sampler(T, pool=pool, ratio=ratio, seed=seed)
    gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
    rs17 = np.random.RandomState(17)
    seeds = [rs17.randint(0, 1e9) for _ in range(T)]
    index = 0
    for _ in range(2 * T + 1):
        ep_rng = np.random.RandomState(seeds[index])
        index = (index + 1) % T
        graph = int(ep_rng.randint(0, pool))
        movement_seed = int(ep_rng.randint(0, 1e9))
        origin = int(ep_rng.randint(0, N))
        density = [i / 10.0 for i in range(1, 11)][index % 10]
        interested = sum(1 << int(i) for i in ep_rng.choice(N, size=int(density * N), replace=False))
        scripted = sum(1 << int(i) for i in gen.choice(N, size=int(round(ratio * N)), replace=False)) & ~(1 << origin)
        ep = s.sample()
        assert (ep.graph_index, ep.movement_seed, ep.origin, ep.interested, ep.scripted) == \
            (graph, movement_seed, origin, interested, scripted)
    assert s.np_random.bit_generator.state == gen.bit_generator.state


def test_sampler_rejects_negative_placement():
    with pytest.raises(ValueError):
        _sampler(7, test_env_step=-1)


def test_episode_stream_abi_has_the_schedule_fields():
    from melissa_amd import _lib
    names = [f[0] for f in _lib.MelEpisodeStream._fields_]
    assert names.index("draw_scripted") < names.index("n_test") < names.index("test_env_step") \
        < names.index("test_episode_step") < names.index("test_seeds") < names.index("test_discarded")      # appended
    assert _lib.MelEpisodeStream.test_seeds.offset % 8 == 0
    assert C.sizeof(_lib.MelEpisodeStream) == _lib.load().mel_abi_sizeof(10)
    assert "mel_episode_test_seeds" in _lib.EXPORTS


def test_refill_validates_the_schedule_arguments_without_a_gpu():
    from melissa_amd import _lib
    lib = _lib.load()
    st, graphs, pool, env = _lib.MelEpisodeStream(), _lib.MelGraphPool(), _lib.MelEpisodePool(), _lib.MelEnvBatch()
    host = (C.c_uint64 * 8)()
    p = C.addressof(host)                       # never dereferenced: every case below fails validation first
    st.n_envs, st.ring = 2, 3
    st.pcg = st.pcg_half = st.produced = st.draw_seed = st.draw_graph = st.work = st.new_count = p
    env.n_envs, env.n_nodes = 2, 20
    graphs.n_graphs, graphs.n_nodes, graphs.pos, graphs.one_hop = 3, 20, p, p
    call = lambda discard=0: lib.mel_episode_refill(C.byref(st), C.byref(graphs), C.byref(pool), C.byref(env), 1, discard, None)
    env.is_testing = 1
    assert call() == _lib.ERR_UNSUPPORTED                                    # testing mode without a schedule
    st.n_test, env.is_testing = 7, 0
    assert call() == _lib.ERR_INVALID_ARG and b"testing mode" in lib.mel_last_error()
    env.is_testing = 1
    assert call() == _lib.ERR_INVALID_ARG and b"test_seeds" in lib.mel_last_error()
    st.test_seeds = st.test_discarded = p
    st.test_env_step, st.test_episode_step = 1, 2
    assert call(discard=1) == _lib.ERR_INVALID_ARG and b"discard" in lib.mel_last_error()
    st.test_env_step = -1
    assert call() == _lib.ERR_INVALID_ARG and b"test_env_step" in lib.mel_last_error()
    st.test_env_step, st.test_episode_step, st.fixed_graph = 0, 1, 1
    graphs.n_graphs = 1
    assert call() == _lib.ERR_UNSUPPORTED                                    # a fixed graph in testing mode
    assert lib.mel_episode_test_seeds(None, 4, None) == _lib.ERR_INVALID_ARG
    assert lib.mel_episode_test_seeds(p, 0, None) == _lib.ERR_INVALID_ARG


def test_command_lines_take_test_envs_and_spread():
    from melissa_amd import train, watch
    a = train.parse_args(["--epoch", "1", "--test-envs", "10"])
    assert a.test_envs == 10 and train.train_kwargs(a)["test_envs"] == 10
    assert train.train_kwargs(train.parse_args([]))["test_envs"] == 1        # the default: one env, the path as it was
    w = watch.arg_parser().parse_args(["--envs", "4", "--episodes", "10", "--spread"])
    assert w.spread is True and w.envs == 4
    assert watch.arg_parser().parse_args([]).spread is False


def test_train_rejects_a_test_envs_below_one():
    from melissa_amd import train
    with pytest.raises(ValueError, match="test_envs"):
        train.train(epoch=1, test_envs=0)
