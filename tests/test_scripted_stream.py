"""CPU side of the scripted-agent episode stream: the derivation the device draw rests on (numpy's
``Generator.choice(n, k, replace=False)`` as a set-valued Floyd draw plus the shuffle's draws), the ABI fields, the host
predicate and the training CLI."""
import ctypes as C
import types

import numpy as np
import pytest

from tests.scripted_draw import Pcg64Mirror

RATIOS = (0.1, 0.25, 0.5, 0.9, 1.0)


@pytest.mark.parametrize("n", [12, 20, 50, 70, 100, 128])
def test_mask_form_draw_equals_numpy_choice(n):
    """Per episode, in World.reset's order on the env generator (core.py:372,378,395): integers(0, 1e9), choice(37),
    choice(n, k, replace=False).  Sets AND the generator's final state (half-word buffer included) must agree."""
    episodes = 6
    for ratio in RATIOS:
        k = int(round(ratio * n))
        for seed in range(8):
            gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed)))
            mir = Pcg64Mirror(seed)
            for ep in range(episodes):
                assert mir.bounded(999999999) == gen.integers(0, 1e9), (ratio, seed, ep)
                assert mir.bounded(36) == gen.choice(37), (ratio, seed, ep)
                want = 0
                for i in gen.choice(n, size=k, replace=False):
                    want |= 1 << int(i)
                got = mir.choice_set(n, k)
                assert got == want and bin(got).count("1") == k, (ratio, seed, ep)
            ref = gen.bit_generator.state
            state, has32, half = mir.state()
            assert state == ref["state"]["state"] and has32 == ref["has_uint32"], (ratio, seed)
            assert not has32 or half == ref["uinteger"], (ratio, seed)


def test_mask_form_draw_is_the_episode_sampler_protocol():
    """The same mirror against EpisodeSampler.sample() (the restatement the golden env traces pin to the reference): fixed
    graph (no graph draw) and a pool, the source cleared from the set."""
    from melissa_amd.env.episodes import EpisodeSampler
    for n, ratio, pool, fixed in [(20, 0.5, 5, False), (100, 0.4, 3, False), (50, 0.25, 1, True)]:
        k = int(round(ratio * n))
        for seed in (3, 11):
            sampler = EpisodeSampler(n, np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed))), pool, fixed,
                                     scripted_agents_ratio=ratio)
            mir = Pcg64Mirror(seed)
            for _ in range(7):
                ep = sampler.sample()
                mir.bounded(999999999)
                if not fixed:
                    assert mir.bounded(pool - 1) == ep.graph_index
                assert mir.choice_set(n, k) & ~(1 << ep.origin) == ep.scripted
            assert mir.state()[0] == sampler.np_random.bit_generator.state["state"]["state"]


def test_train_cli_takes_the_reference_flags():
    from melissa_amd import train
    a = train.arg_parser().parse_args(["--heuristic", "mpr", "--scripted-agents-ratio", "0.5"])
    assert a.heuristic == "mpr" and a.scripted_agents_ratio == 0.5
    d = train.arg_parser().parse_args([])
    assert d.heuristic is None and d.scripted_agents_ratio == 0.0            # common.py:67,69
    with pytest.raises(SystemExit):
        train.arg_parser().parse_args(["--heuristic", "probabilistic_gossip"])


def test_episode_stream_abi_has_the_scripted_fields():
    from melissa_amd import _lib
    names = [f[0] for f in _lib.MelEpisodeStream._fields_]
    assert names.index("new_count") < names.index("n_scripted") < names.index("draw_scripted")      # appended
    assert _lib.MelEpisodeStream.n_scripted.size == 4 and _lib.MelEpisodeStream.draw_scripted.offset % 8 == 0
    assert C.sizeof(_lib.MelEpisodeStream) == _lib.load().mel_abi_sizeof(10)


def test_refill_validates_the_scripted_arguments_without_a_gpu():
    """n_scripted out of range / without its buffers is an argument error, not a launch."""
    from melissa_amd import _lib
    lib = _lib.load()
    st, graphs, pool, env, snap = (_lib.MelEpisodeStream(), _lib.MelGraphPool(), _lib.MelEpisodePool(), _lib.MelEnvBatch(),
                                   _lib.MelEnvBatch())
    host = (C.c_uint64 * 8)()
    p = C.addressof(host)                       # never dereferenced: every case below fails validation first
    st.n_envs, st.ring = 2, 3
    st.pcg = st.pcg_half = st.produced = st.draw_seed = st.draw_graph = st.work = st.new_count = p
    env.n_envs, env.n_nodes = 2, 20
    graphs.n_graphs, graphs.n_nodes, graphs.pos, graphs.one_hop = 1, 20, p, p
    call = lambda: lib.mel_episode_refill(C.byref(st), C.byref(graphs), C.byref(pool), C.byref(env), 1, 0, None)
    for bad in (-1, 21):
        st.n_scripted = bad
        assert call() == _lib.ERR_INVALID_ARG and b"n_scripted" in lib.mel_last_error()
    st.n_scripted = 10                          # no draw_scripted
    assert call() == _lib.ERR_INVALID_ARG and b"draw_scripted" in lib.mel_last_error()
    st.draw_scripted = p                        # no pool->scripted
    assert call() == _lib.ERR_INVALID_ARG and b"draw_scripted" in lib.mel_last_error()
    env.is_testing = 1
    assert call() == _lib.ERR_UNSUPPORTED


def test_stream_supported_covers_scripted_training():
    from melissa_amd.env.stream import stream_supported

    def venv(ratio=0.0, is_testing=False, fixed=False, dynamic=True):
        return types.SimpleNamespace(_sampler_kw=dict(is_testing=is_testing, scripted_agents_ratio=ratio),
                                     fixed_graph=fixed, dynamic_graph=dynamic)
    assert stream_supported(venv(0.5)) and stream_supported(venv(0.0)) and stream_supported(venv(0.5, fixed=True, dynamic=False))
    assert not stream_supported(venv(0.5, is_testing=True)) and not stream_supported(venv(0.0, is_testing=True))
    assert not stream_supported(venv(1.0))                   # training mode, every node scripted: not playable
    assert not stream_supported(venv(0.5, fixed=True))       # a fixed graph that moves
