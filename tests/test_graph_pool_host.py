"""The graph-pool plumbing that needs no GPU: the ``python -m melissa_amd.env.episodes`` writer, ``--graph-pool`` on both command
lines, ``cached_graph_pool``'s host path, and the argument checks ``device_graph_pool`` makes before it touches a device."""
import os

import numpy as np
import pytest

from melissa_amd import _lib, train, watch
from melissa_amd.env import episodes
from melissa_amd.env.episodes import (cached_graph_pool, default_pool_chunk, device_graph_pool, load_graph_pool, packed_graph_pool)


@pytest.fixture(scope="module")
def host_50_4():
    return packed_graph_pool(50, 4, 0)


@pytest.fixture()
def no_gpu(monkeypatch):
    """A process without a GPU: the generator must not be reached."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def refuse(*a, **k):
        raise AssertionError("device_graph_pool called without a GPU")
    monkeypatch.setattr(episodes, "device_graph_pool", refuse)


def test_cli_writer_round_trips(tmp_path, host_50_4, no_gpu, capsys):
    path = str(tmp_path / "pool.npz")
    episodes.main(["--nodes", "50", "--graphs", "4", "--out", path])
    assert "4 connected 50-node graphs" in capsys.readouterr().out
    pos, hop, seeds = host_50_4
    graphs = load_graph_pool(path)
    assert len(graphs) == 4
    for g, graph in enumerate(graphs):
        np.testing.assert_array_equal(graph.pos, pos[g])
        np.testing.assert_array_equal(graph.one_hop, hop[g])
        assert graph.one_hop.dtype == np.uint64 and graph.pos.dtype == np.float64
    with np.load(path) as z:
        np.testing.assert_array_equal(z["seeds"], seeds)
    # --first-seed: starting at the second accepted seed drops the first graph
    episodes.main(["--nodes", "50", "--graphs", "3", "--first-seed", str(int(seeds[1])), "--out", path])
    np.testing.assert_array_equal(np.stack([g.pos for g in load_graph_pool(path)]), pos[1:])


def test_parsers_accept_graph_pool(capsys):
    a = train.parse_args(["--graph-pool", "pool.npz"])
    assert a.graph_pool == "pool.npz" and train.train_kwargs(a)["graph_pool"] == "pool.npz"
    assert capsys.readouterr().err == ""
    assert train.train_kwargs(train.parse_args([]))["graph_pool"] is None
    a = train.parse_args(["--graph-pool", "pool.npz", "--graphs", "64"])           # both: --graphs is ignored, with a message
    assert a.graph_pool == "pool.npz"
    assert "--graphs 64 is ignored" in capsys.readouterr().err
    w = watch.arg_parser().parse_args(["--graph-pool", "pool.npz"])
    assert w.graph_pool == "pool.npz" and w.graphs == 16
    assert watch.arg_parser().parse_args([]).graph_pool is None


def test_cached_graph_pool_takes_the_host_path_without_a_gpu(tmp_path, host_50_4, no_gpu):
    pos, hop, seeds = host_50_4
    graphs = cached_graph_pool(50, 4, 0, cache_dir=str(tmp_path))
    assert os.listdir(str(tmp_path)) == ["graph_pool_n50_4_0.npz"]                 # the file name it always had
    np.testing.assert_array_equal(np.stack([g.pos for g in graphs]), pos)
    np.testing.assert_array_equal(np.stack([g.one_hop for g in graphs]), hop)
    with np.load(str(tmp_path / "graph_pool_n50_4_0.npz")) as z:
        assert sorted(z.files) == ["adj", "pos", "seeds"]
        np.testing.assert_array_equal(z["seeds"], seeds)
    again = cached_graph_pool(50, 4, 0, cache_dir=str(tmp_path))                   # second call: read from the file
    np.testing.assert_array_equal(np.stack([g.pos for g in again]), pos)


def test_device_graph_pool_checks_its_arguments_first(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded for arguments that are out of range")
    monkeypatch.setattr(_lib, "load", refuse)
    with pytest.raises(ValueError, match="200 nodes"):
        device_graph_pool(200, 1)
    with pytest.raises(ValueError):
        device_graph_pool(20, 1, first_seed=2 ** 32)
    with pytest.raises(ValueError):
        device_graph_pool(20, 1, first_seed=-1)
    with pytest.raises(ValueError):
        device_graph_pool(20, 1, chunk=0)


def test_default_chunk_fits_the_budget():
    for n in (2, 20, 50, 64, 65, 100, 128):
        c = default_pool_chunk(n)
        assert c * (n * (16 + 8 * episodes.set_words(n)) + 4) <= episodes.POOL_CHUNK_BYTES < (c + 1) * (n * (16 + 8 * episodes.set_words(n)) + 4)


def test_generate_entry_point_refuses_bad_arguments():
    """mel_graph_pool_generate's own checks (no launch happens: every call fails before it)."""
    lib = _lib.load()
    import ctypes as C
    buf = (C.c_char * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 256
    call = lambda n=20, first=0, m=4, pos=p, ws=p: lib.mel_graph_pool_generate(n, 0.04, first, m, 4, pos, p, p, p, ws, 0, None)
    assert call(n=1) == _lib.ERR_INVALID_ARG and call(n=129) == _lib.ERR_INVALID_ARG
    assert call(pos=None) == _lib.ERR_INVALID_ARG and call(ws=None) == _lib.ERR_INVALID_ARG
    assert call(first=-1) == _lib.ERR_INVALID_ARG
    assert call(first=2 ** 32 - 3) == _lib.ERR_INVALID_ARG                         # 4 candidates from 2^32 - 3 leave the key range
    assert "2^32" in _lib.last_error()
    assert call(m=-1) == _lib.ERR_INVALID_ARG
    assert call() == _lib.ERR_WORKSPACE                                            # ws_bytes = 0
    assert call(m=0) == _lib.OK                                                    # nothing to examine: no launch
    assert lib.mel_graph_pool_workspace_bytes(200, 4) == 0 and lib.mel_graph_pool_workspace_bytes(1, 4) == 0
    assert lib.mel_graph_pool_workspace_bytes(20, 1000) >= 1000 * (4 + 20 * 24)
    assert lib.mel_graph_pool_workspace_bytes(128, 1000) >= 1000 * (4 + 128 * 32)
