"""GPU parity of the forms an episode refill takes (csrc/episode_stream.hpp): generators seeded one lane per episode into the
key scratch (``episode_keys_kernel``) or inside the episode's own wavefront (work items past ``key_capacity``, and episodes
whose movement seed lies beyond the outputs the keys launch looks at), the movement table by a four-wave workgroup, the reset
snapshot in a launch of its own.  Every ring array, ``produced``, the PCG state and the snapshot scalars are checked against
the numpy protocol (``EpisodeSampler``: ``Generator(PCG64)``, ``RandomState`` randint / uniform / permutation) at the smallest
shapes where each part can go wrong: one- and two-word node sets, refills that cross a 64-lane seeding wave, movement tables
below and beyond one regeneration of the 624-word key, an empty refill, a single new episode, the first fill."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.trace_replay import set_int      # node sets (uint64 scalar, or words beyond 64 nodes) -> int


def _graphs(n, count):
    """`count` graphs over a few distinct ones (the graph draw's range matters to the sampler, not the graphs)."""
    from melissa_amd.env import synthetic_graph_pool
    base = synthetic_graph_pool(n, min(count, 3), first_seed=3, radius=0.7 if n < 12 else 0.45 if n < 50 else 0.2)
    return [base[g % len(base)] for g in range(count)]


def _snapshot_scalars(st):
    from melissa_amd import _lib as L
    pool = st.pool
    off = pool.snapshot_env.scalars - pool.snapshot_state.data_ptr()
    e = int(pool.struct.n_episodes)
    return pool.snapshot_state[off: off + e * L.ENV_SCALARS * 4].view(torch.int32).view(e, -1).cpu().numpy()


def _check_ring(st, venv, graphs, want, cursors, discard=0):
    """Every live slot of every env's ring - the episode being played (cursor - 1) up to the newest one - against `want`."""
    from melissa_amd import _lib as L
    from melissa_amd.env.episodes import movement_offsets
    K, n = st.ring, venv.n
    torch.cuda.synchronize()
    produced = st.produced.cpu().numpy()
    t = {k: v.cpu().numpy() for k, v in st.pool.tensors.items()}
    sc = _snapshot_scalars(st)
    checked = 0
    for b in range(venv.env_num):
        for j in range(max(0, int(cursors[b]) - 1), int(produced[b])):
            slot = b * K + j % K
            ep = want[b][j + discard]
            g = graphs[ep.graph_index]
            assert t["origin"][slot] == ep.origin, (b, j)
            assert set_int(t["interested"][slot]) == ep.interested, (b, j)
            assert set_int(t["scripted"][slot]) == ep.scripted, (b, j)
            np.testing.assert_array_equal(t["pos"][slot], g.pos)
            np.testing.assert_array_equal(t["one_hop"][slot].view(np.uint64), g.one_hop)
            if venv.dynamic_graph:
                np.testing.assert_array_equal(t["moves"][slot], movement_offsets(ep.movement_seed, n, venv.max_moves))
            assert sc[slot, L.S_ORIGIN] == ep.origin and sc[slot, L.S_EPISODE] == slot, (b, j)
            # (World.reset ends with one world step: a moving graph has consumed its first movement offsets)
            assert sc[slot, L.S_MOVE_CURSOR] == int(venv.dynamic_graph), (b, j)
            assert sc[slot, L.S_NUM_MOVES] == 0 and sc[slot, L.S_EP_CURSOR] == 0, (b, j)
            assert sc[slot, L.S_ERROR] == 0 and sc[slot, L.S_EPISODES_DONE] == 0, (b, j)
            checked += 1
    return checked


def _check_pcg(st, venv, seed, discard=0, env_arg=False):
    """The envs' generators: numpy's PCG64 state after the same number of samplings."""
    pcg = st.pcg.cpu().numpy().view(np.uint64)
    half = st.pcg_half.cpu().numpy().view(np.uint32)
    for b in range(venv.env_num):
        sampler = venv.make_sampler(seed + b, env=b) if env_arg else venv.make_sampler(seed + b)
        for _ in range(int(st.produced[b]) + discard):
            sampler.sample()
        ref = sampler.np_random.bit_generator.state
        assert (int(pcg[b, 1]) << 64 | int(pcg[b, 0])) == ref["state"]["state"]
        assert int(half[b, 0]) == ref["has_uint32"] and (not ref["has_uint32"] or int(half[b, 1]) == ref["uinteger"])


def _walk(st, venv, graphs, want, seed, discard=0, env_arg=False):
    """The first fill (ring - 1 episodes per env), a refill with no free slot, one with a single new episode, then two
    consecutive refills that together replace the whole ring (the key scratch must carry nothing over)."""
    from melissa_amd import _lib as L
    B, K = venv.env_num, st.ring
    cursor = venv.scalars()[:, L.S_EP_CURSOR]
    cur = np.zeros(B, dtype=np.int64)
    assert (st.produced.cpu().numpy() == K - 1).all()
    checked = _check_ring(st, venv, graphs, want, cur, discard)
    # ---- no free slot: nothing is drawn, nothing is written
    before = {k: v.clone() for k, v in st.pool.tensors.items()}
    pcg_before, snap_before = st.pcg.clone(), st.pool.snapshot_state.clone()
    st.refill()
    torch.cuda.synchronize()
    assert (st.produced.cpu().numpy() == K - 1).all() and torch.equal(st.pcg, pcg_before)
    assert all(torch.equal(v, before[k]) for k, v in st.pool.tensors.items()) and torch.equal(st.pool.snapshot_state, snap_before)
    # ---- a single new episode: only env B - 1 has started its second one
    cur[B - 1] = 1
    cursor.copy_(torch.from_numpy(cur.astype(np.int32)))
    st.refill()
    torch.cuda.synchronize()
    produced = st.produced.cpu().numpy()
    assert produced[B - 1] == K and (produced[:B - 1] == K - 1).all()
    checked += _check_ring(st, venv, graphs, want, cur, discard)
    # ---- two consecutive refills on one stream: 3 or 4 new episodes per env, then ring - 1
    for step in (3, K - 1):
        cur = np.maximum(cur, 1) + step
        cursor.copy_(torch.from_numpy(cur.astype(np.int32)))
        st.refill()
        torch.cuda.synchronize()
        assert (st.produced.cpu().numpy() == cur + K - 1).all()
        checked += _check_ring(st, venv, graphs, want, cur, discard)
    _check_pcg(st, venv, seed, discard, env_arg)
    return checked


def _want(venv, seed, count, env_arg=False):
    out = []
    for b in range(venv.env_num):
        sampler = venv.make_sampler(seed + b, env=b) if env_arg else venv.make_sampler(seed + b)
        out.append([sampler.sample() for _ in range(count)])
    return out


# n = 7 / 50 / 100: a partial word, the headline, two-word sets.  70 envs: the new episodes of a refill cross a 64-lane seeding
# wave (first fill 70 * (ring - 1) episodes; the later refills 1, 279 and 70 * (ring - 1)); 3 envs stay inside one.
# max_moves 4 at n = 50: 400 doubles, beyond the 312 of one regeneration of the movement key; max_moves 1: within one.
@pytest.mark.parametrize("n,B,K,max_moves", [(7, 3, 6, 1), (7, 70, 6, 4), (50, 3, 16, 4), (50, 70, 16, 1), (50, 70, 6, 4),
                                             (100, 3, 6, 1), (100, 70, 16, 4)])
def test_refill_matches_numpy_protocol(n, B, K, max_moves):
    from melissa_amd.env import HipGraphVectorEnv
    from melissa_amd.env.stream import EpisodeStream
    seed, discard = 123, 1
    graphs = _graphs(n, 5)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=max_moves,
                             construct_like_reference=False)
    want = _want(venv, seed, 3 * K + 6 + discard)
    st = EpisodeStream(venv, seed, ring=K, discard=discard)
    assert int(st.struct.key_capacity) == B * (K - 1)          # the scratch holds the first fill
    assert _walk(st, venv, graphs, want, seed, discard) > 3 * B * (K - 1)


# ---- env seeds chosen on the CPU for the rejections their episodes' generators meet -------------------------------------------
def _raw_outputs(episode_seed, count=400):
    return [int(x) for x in np.random.RandomState(episode_seed)._bit_generator.random_raw(count)]


def _rejections(episode_seed, n, pool=None, density=True):
    """numpy's masked rejection sampling replayed on the raw MT19937 outputs of RandomState(episode_seed): (outputs consumed up
    to and including the accepted movement seed, rejections of randint(0, 1e9), longest run of rejections inside one draw of
    permutation(n), outputs consumed in all)."""
    r, p = _raw_outputs(episode_seed), 0

    def masked(rng):
        nonlocal p
        mask, rejected = (1 << int(rng).bit_length()) - 1, 0
        while rng:
            v = r[p] & mask
            p += 1
            if v <= rng:
                break
            rejected += 1
        return rejected

    if pool is not None:
        masked(pool - 1)
    first = masked(999999999)
    used = p
    masked(n - 1)
    p += 2 if density else 0
    run = max(masked(i) for i in range(n - 1, 0, -1))
    return used, first, run, p


# seed 51, env 2, episode 4 (the last one of a first fill of ring 6): randint(0, 1e9) rejects its first TWO outputs, and one
# draw of permutation(50) rejects eleven times in a row.
# The same seed at 92 nodes: the fill wavefront draws its first 128 outputs from registers (mt_head) and the later ones from the
# regenerated key in LDS; the 15 episodes of the first fill consume fewer than 128 outputs, exactly 128 (the head is used up
# and nothing more is asked), 129 (one output past it) and more.  At 50 nodes every episode stays inside the head.
REJECTING_SEED = 51


@pytest.mark.parametrize("n", [50, 92])
def test_refill_on_seeds_whose_draws_reject(n):
    from melissa_amd.env import HipGraphVectorEnv
    from melissa_amd.env.stream import EpisodeStream
    B, K, seed = 3, 6, REJECTING_SEED
    graphs = _graphs(n, 5)
    # the property itself, from numpy: episode seed and graph come from the env's generator, in this order
    traces = []
    for b in range(B):
        gen = np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b)))
        for _ in range(K - 1):
            episode_seed = int(gen.integers(0, 1e9))
            gen.choice(len(graphs), replace=True)
            traces.append(_rejections(episode_seed, n))
            accepted = [v & 0x3FFFFFFF for v in _raw_outputs(episode_seed, 40) if (v & 0x3FFFFFFF) <= 999999999][0]
            assert np.random.RandomState(episode_seed).randint(0, 1e9) == accepted       # (the replay is numpy's algorithm)
    last = traces[2 * (K - 1) + 4]                                                        # env 2, episode 4
    consumed = [t[3] for t in traces]
    if n == 50:
        assert last[1] == 2 and last[2] >= 2 and max(consumed) < 128, traces
    else:
        assert last[1] == 2 and min(consumed) < 128 and 128 in consumed and 129 in consumed and max(consumed) > 129, consumed
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=2,
                             construct_like_reference=False)
    want = _want(venv, seed, 3 * K + 6)
    assert _walk(EpisodeStream(venv, seed, ring=K), venv, graphs, want, seed) > 3 * B * (K - 1)


# ---- the evaluation schedule, scripted sets, fixed density, static graphs ------------------------------------------------------
@pytest.mark.parametrize("n,n_graphs,T,K,dynamic,density,ratio", [(50, 4, 3, 6, True, None, 0.5),     # n_test = 3, half scripted
                                                                  (100, 4, 3, 6, False, 0.6, 0.5),    # static pool, two words
                                                                  (20, 17, 30, 16, True, None, 0.0)])
def test_refill_of_the_evaluation_schedule(n, n_graphs, T, K, dynamic, density, ratio):
    """(20, 17, 30, 16): with 17 graphs the graph draw rejects 15 of 32 masked values, and list position 24 accepts its
    movement seed only as the generator's 9th output - one more than ``episode_keys_kernel`` looks at (MEL_KEY_DRAWS = 8),
    so that episode seeds its movement generator inside its wavefronts while its neighbours read the scratch.  Every env
    walks the list from the top and reaches position 24 in its second refill."""
    from melissa_amd.env import HipGraphVectorEnv
    from melissa_amd.env.stream import TestEpisodeStream
    B, seed = 5, 77
    graphs = _graphs(n, n_graphs)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=dynamic, device="cuda", max_moves=4,
                             construct_like_reference=False, is_testing=True, num_test_episodes=T,
                             scripted_agents_ratio=ratio, fixed_interest_density=density)
    if n_graphs == 17:
        lst = venv.make_sampler(0).test_seeds_list
        used = [_rejections(int(s), n, pool=n_graphs, density=False)[0] for s in lst]
        assert used[24] == 9 and max(used) == 9, used            # just past what the keys launch reaches
    want = _want(venv, seed, 3 * K + 6, env_arg=True)
    st = TestEpisodeStream(venv, seed, ring=K)
    assert _walk(st, venv, graphs, want, seed, env_arg=True) > 3 * B * (K - 1)


@pytest.mark.parametrize("n,dynamic,density,ratio,fixed", [(50, True, 0.35, 0.5, False), (100, False, 0.6, 0.5, False),
                                                           (20, False, None, 0.0, True)])
def test_refill_with_scripted_sets_fixed_density_and_static_graphs(n, dynamic, density, ratio, fixed):
    from melissa_amd.env import HipGraphVectorEnv
    from melissa_amd.env.stream import EpisodeStream
    B, K, seed = 5, 6, 9
    graphs = _graphs(n, 1 if fixed else 4)
    kw = dict(graph=graphs[0]) if fixed else dict(graph_pool=graphs)
    venv = HipGraphVectorEnv(B, n, dynamic_graph=dynamic, device="cuda", max_moves=4, construct_like_reference=False,
                             fixed_interest_density=density, scripted_agents_ratio=ratio, **kw)
    want = _want(venv, seed, 3 * K + 6)
    assert _walk(EpisodeStream(venv, seed, ring=K), venv, graphs, want, seed) > 3 * B * (K - 1)


# ---- the capacity of the key scratch -------------------------------------------------------------------------------------------
# 13 envs x ring 6: the first fill draws 65 episodes (one past a seeding wave).  Capacities just below, at and just above it,
# one that ends inside the first seeding wave, and none at all (every episode seeds in-wave).
@pytest.mark.parametrize("capacity", [0, 40, 64, 65, 66])
def test_refill_around_the_key_capacity(capacity):
    from melissa_amd.env import HipGraphVectorEnv
    from melissa_amd.env.stream import EpisodeStream
    n, B, K, seed = 50, 13, 6, 5
    graphs = _graphs(n, 5)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=4,
                             construct_like_reference=False)
    want = _want(venv, seed, 3 * K + 6)
    st = EpisodeStream(venv, seed, ring=K, key_capacity=capacity)
    assert int(st.struct.key_capacity) == capacity and (st.key_scratch is None) == (capacity == 0)
    assert _walk(st, venv, graphs, want, seed) > 3 * B * (K - 1)
    # and byte for byte the stream that seeds everything through the scratch, snapshots included
    venv2 = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=4,
                              construct_like_reference=False)
    st2 = EpisodeStream(venv2, seed, ring=K)
    _walk(st2, venv2, graphs, want, seed)
    assert all(torch.equal(v, st2.pool.tensors[k]) for k, v in st.pool.tensors.items())
    assert torch.equal(st.pool.snapshot_state, st2.pool.snapshot_state)
