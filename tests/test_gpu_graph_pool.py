"""GPU parity of the device graph-pool generator (csrc/graph_pool.hpp, ``mel_graph_pool_generate``,
``melissa_amd.env.device_graph_pool``) with the host loop ``packed_graph_pool``: positions, node sets and seeds bit for bit,
in the same order, whatever the chunk size; then the pool through a file into the env and into ``train``.

Every host expectation is computed once per module."""
import functools

import numpy as np
import pytest

from melissa_amd.env import (Graph, HipGraphVectorEnv, device_graph_pool, load_graph_pool, packed_graph_pool, save_graph_pool,
                             synthetic_graph_pool)

pytestmark = pytest.mark.gpu

# (n, count, first_seed, radius, last accepted seed)
CASES = [
    (20, 5, 0, 0.2, 15081),                     # rare acceptance: thousands of rejects between accepts
    (20, 3, 1000, 0.2, 4098),                   # first_seed != 0, the first accept is not the first candidate
    (50, 200, 0, 0.2, 783),                     # the benchmark size
    (64, 100, 0, 0.2, 183),                     # last one-word size
    (65, 100, 0, 0.2, 168),                     # first two-word size
    (100, 100, 0, 0.2, 106),                    # two nodes per lane
    (128, 64, 0, 0.2, 64),                      # all 512 words of one regeneration
    (100, 64, 2 ** 31 - 40, 0.2, 2147483677),   # seeds across 2^31
    (128, 40, 2 ** 32 - 64, 0.2, 4294967272),   # the top of the key range
    (12, 20, 0, 0.4, 39),                       # another radius, few lanes active
]


@functools.lru_cache(maxsize=None)
def host(n, count, first_seed, radius):
    out = packed_graph_pool(n, count, first_seed, radius)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def device(n, count, first_seed, radius, chunk=None):
    return device_graph_pool(n, count, first_seed, radius, device="cuda:0", chunk=chunk)


def assert_same_pool(got, want):
    for g, w, name in zip(got, want, ("pos", "one_hop", "seeds")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("n,count,first_seed,radius,last", CASES)
def test_device_pool_is_the_host_pool(n, count, first_seed, radius, last):
    want = host(n, count, first_seed, radius)
    assert int(want[2][-1]) == last                            # the inputs are the ones the cases were chosen on
    assert_same_pool(device(n, count, first_seed, radius), want)


@pytest.mark.parametrize("chunk", [64, 1000, None])
def test_chunk_size_does_not_matter(chunk):
    assert_same_pool(device(50, 200, 0, 0.2, chunk), host(50, 200, 0, 0.2))


def test_seeds_run_out():
    with pytest.raises(ValueError, match="2\\^32"):
        device_graph_pool(20, 1, first_seed=2 ** 32 - 8, device="cuda:0")       # none of the last eight seeds is connected


def test_nothing_asked_for():
    pos, hop, seeds = device_graph_pool(20, 0, device="cuda:0")
    assert pos.shape == (0, 20, 2) and hop.shape == (0, 20) and seeds.shape == (0,)


@pytest.mark.parametrize("n,count,first_seed,radius", [c[:4] for c in CASES])
def test_device_graphs_are_what_they_claim(n, count, first_seed, radius):
    """Properties of the device result itself: every graph is connected, and its node sets are the radius rule on its
    positions."""
    pos, hop, seeds = device(n, count, first_seed, radius)
    assert np.all(np.diff(seeds) > 0) and seeds[0] >= first_seed
    for g in range(count):
        assert Graph(pos[g], hop[g]).is_connected(), g
        np.testing.assert_array_equal(Graph.from_positions(pos[g], radius).one_hop, hop[g])


def test_pool_file_drives_the_env_like_the_host_pool(tmp_path):
    path = str(tmp_path / "pool.npz")
    save_graph_pool(path, *device(50, 4, 0, 0.2))
    venvs = [HipGraphVectorEnv(8, 50, graph_pool=pool, dynamic_graph=True, device="cuda:0", seed=7)
             for pool in (load_graph_pool(path), synthetic_graph_pool(50, 4, 0))]
    obs = [v.reset()[0] for v in venvs]
    tape = np.random.RandomState(3).randint(0, 2, size=(12, 8))
    for t in range(12):
        for o, p in zip(*obs):
            np.testing.assert_array_equal(o["obs"], p["obs"], err_msg=f"round {t}")
            assert o["agent_id"] == p["agent_id"]
        out = [v.step(tape[t]) for v in venvs]
        obs = [list(o[0]) for o in out]
        np.testing.assert_array_equal(out[0][1], out[1][1])
        np.testing.assert_array_equal(out[0][2], out[1][2])
        for k in range(8):
            if out[0][2][k] and out[0][4][k].get("explicit_reset"):
                for i, v in enumerate(venvs):
                    obs[i][k] = v.reset([k])[0][0]


def test_train_from_a_pool_file_matches_train_from_a_count(tmp_path):
    from melissa_amd.train import train
    pos, hop, seeds = host(20, 5, 0, 0.2)                       # its first four graphs are the pool of --graphs 4
    path = str(tmp_path / "pool.npz")
    save_graph_pool(path, pos[:4], hop[:4], seeds[:4])
    kw = dict(model="l_dgn", n_nodes=20, envs=8, updates=2, capture_updates=False, log=lambda line: None)
    from_file = train(graph_pool=path, graphs=999, **kw)        # graphs is not used beside a file
    from_count = train(graphs=4, **kw)
    assert from_file["updates"] == from_count["updates"] == 2
    assert from_file["param_checksum"] == from_count["param_checksum"]
