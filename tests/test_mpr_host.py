"""The "mpr" scripted-agent heuristic on the CPU: the restatement (tests/mpr_oracle.py) against the reference's recorded
MPR sets and GraphEnv traces (tests/golden/make_mpr_golden.py), the argument checks, and the watch flags."""
import glob
import os
import re

import numpy as np
import pytest

from oracle import env_oracle as eo
from tests.mpr_oracle import MprOracleGraphEnv, mpr_set
from tests.trace_replay import replay, set_int, set_ints

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SETS = sorted(glob.glob(os.path.join(GOLDEN, "mpr_sets_*.npz")))
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mpr_trace_*.npz")))


def test_fixtures_present():
    assert len(SETS) >= 7 and len(TRACES) >= 4


@pytest.mark.parametrize("path", SETS, ids=[os.path.basename(p)[9:-4] for p in SETS])
def test_restatement_equals_reference_sets(path):
    f = np.load(path)
    checked = 0
    for g in range(f["adj"].shape[0]):
        adj = set_ints(f["adj"][g])
        want = set_ints(f["mpr"][g])
        got = [mpr_set(adj, v) for v in range(len(adj))]
        assert got == want, f"{f['names'][g]}"
        checked += len(adj)
    assert checked >= 12


def test_fixture_graph_sets_by_hand():
    """The reference's 12-node test graph (test_core.py:23-31): node 0 reaches 5, 6 only through 2, 7 only through 3 and
    11 through 4; 10 hangs off 3, so it relays for no one and has no two-hop neighbours."""
    f = np.load(os.path.join(GOLDEN, "mpr_sets_n12_fixture.npz"))
    mpr = set_ints(f["mpr"][0])
    assert mpr[0] == (1 << 2) | (1 << 3) | (1 << 4)
    assert mpr[10] == 1 << 3 and mpr[5] == 1 << 2


def build_oracle(tr):
    n = int(tr["n"])
    pool = [eo.GraphSpec(tr["pool_pos"][k], set_ints(tr["pool_adj"][k])) for k in range(tr["pool_pos"].shape[0])]
    kw = dict(number_of_agents=n, dynamic_graph=bool(tr["dynamic"]), graph_pool=pool,
              scripted_agents_ratio=float(tr["scripted_agents_ratio"]), heuristic=str(tr["heuristic"]),
              np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(tr["env_seed"])))))
    if bool(tr["is_testing"]):
        kw.update(is_testing=True, num_test_episodes=int(tr["num_test_episodes"]))
    env = MprOracleGraphEnv(**kw)
    env.forwards = 0                    # the generator counts from the first recorded reset on
    return env


@pytest.mark.parametrize("path", TRACES, ids=[os.path.basename(p)[10:-4] for p in TRACES])
def test_oracle_replays_mpr_trace(path):
    tr = np.load(path)
    env = build_oracle(tr)
    pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
    pz.env, pz.n, pz.rewards = env, env.n, [0] * env.n
    row = [0]

    def state():
        r = row[0]
        row[0] += 1
        assert env.received_from == set_ints(tr["received_from"][r]), f"row {r} received_from"
        return dict(agents_mask=env.agents, alive_mask=env.alive, terminated_mask=env.terminated,
                    has_message_mask=env.has_message, interested_mask=env.interested, scripted_mask=env.scripted,
                    origin=env.origin_agent, pos=env.pos, one_hop=env.adj, two_hop=env.two_hop)

    rows = replay(tr, pz, state)
    assert rows >= 300 and row[0] == rows
    assert env.forwards == int(tr["forwards"])
    if bool(tr["is_testing"]):
        assert env.forwards >= 5


def test_oracle_argument_checks():
    pool = [eo.GraphSpec(np.random.RandomState(0).uniform(size=(10, 2)))]
    with pytest.raises(ValueError, match="no heuristic can be set"):
        MprOracleGraphEnv(10, graph_pool=pool, scripted_agents_ratio=0.0)
    with pytest.raises(ValueError, match=r"must be in \[0.0, 1.0\]"):
        MprOracleGraphEnv(10, graph_pool=pool, scripted_agents_ratio=1.5)


def test_env_argument_checks_for_mpr():
    """core.py:143-152: the reference's argument errors, raised before the env touches the GPU."""
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    pool = synthetic_graph_pool(20, 2, 10)
    with pytest.raises(ValueError, match="no heuristic can be set"):
        HipGraphVectorEnv(2, 20, graph_pool=pool, heuristic="mpr")
    with pytest.raises(ValueError, match=r"must be in \[0.0, 1.0\]"):
        HipGraphVectorEnv(2, 20, graph_pool=pool, scripted_agents_ratio=-0.5, heuristic="mpr")


def test_abi_constants():
    from melissa_amd import _lib
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "melissa_hip.h")).read()
    assert int(re.search(r"#define MEL_HEURISTIC_MPR\s+(\d+)", header).group(1)) == _lib.HEURISTICS["mpr"] == 4
    assert _lib.MelEnvBatch._fields_[-1][0] == "received_from"


def test_mpr_sets_rejects_bad_adjacency():
    import torch
    from melissa_amd.env import mpr_sets
    ok = torch.tensor([[0b10, 0b01]], dtype=torch.int64)
    with pytest.raises(ValueError, match="not symmetric"):
        mpr_sets(torch.tensor([[0b10, 0b00]], dtype=torch.int64))
    with pytest.raises(ValueError, match="self loops"):
        mpr_sets(torch.tensor([[0b11, 0b01]], dtype=torch.int64))
    with pytest.raises(ValueError, match="beyond"):
        mpr_sets(torch.tensor([[0b110, 0b001]], dtype=torch.int64))
    with pytest.raises(ValueError, match="shape"):
        mpr_sets(ok.reshape(1, 2, 1))
    with pytest.raises(ValueError, match="device tensor"):
        mpr_sets(ok)                     # valid, but a host tensor


def test_watch_flags_parse_and_reach_the_env(monkeypatch):
    import melissa_amd.watch as w
    seen = {}
    monkeypatch.setattr(w, "watch", lambda *a, **k: seen.update(args=a, kwargs=k) or {})
    w.main(["--nodes", "20", "--heuristic", "mpr", "--scripted-agents-ratio", "0.5"])
    assert seen["kwargs"]["heuristic"] == "mpr" and seen["kwargs"]["scripted_agents_ratio"] == 0.5
    w.main([])
    assert seen["kwargs"]["heuristic"] is None and seen["kwargs"]["scripted_agents_ratio"] == 0.0
    with pytest.raises(SystemExit):
        w.main(["--heuristic", "probabilistic_gossip"])
    monkeypatch.undo()

    class Stop(Exception):
        pass

    class Net:
        def eval(self):
            pass

        def set_feature_dtype(self, dtype):
            pass

    def env(*a, **k):
        seen["env"] = k
        raise Stop

    monkeypatch.setattr(w, "build_network", lambda *a, **k: Net())
    monkeypatch.setattr(w, "DQNPolicy", lambda *a, **k: None)
    monkeypatch.setattr(w, "HipGraphVectorEnv", env)
    with pytest.raises(Stop):
        w.watch(n_nodes=20, envs=2, episodes=2, heuristic="silent", scripted_agents_ratio=0.25, device="cpu")
    assert seen["env"]["heuristic"] == "silent" and seen["env"]["scripted_agents_ratio"] == 0.25
    assert seen["env"]["is_testing"] is True


def test_batch_restatement_equals_the_pinned_one():
    """mpr_sets_batch (the GPU tests' bulk expectation) against mpr_set on the golden graphs and on random graphs with
    isolated nodes and dense parts."""
    from tests.mpr_oracle import mpr_sets_batch
    for path in SETS:
        f = np.load(path)
        n = int(f["n"])
        adj = np.array([[[(set_int(r) >> j) & 1 for j in range(n)] for r in g] for g in f["adj"]], dtype=bool)
        got = mpr_sets_batch(adj)
        want = [[set_int(m) for m in g] for g in f["mpr"]]
        assert [[sum(1 << int(j) for j in np.nonzero(row)[0]) for row in g] for g in got] == want
    rng = np.random.RandomState(3)
    for n in (7, 33, 70):
        adj = np.triu(rng.uniform(size=(20, n, n)) < rng.uniform(0.02, 0.5, size=(20, 1, 1)), 1)
        adj = adj | adj.transpose(0, 2, 1)
        adj[:, : n // 5] = adj[:, :, : n // 5] = False                  # isolated nodes
        got = mpr_sets_batch(adj)
        for g in range(20):
            rows = [sum(1 << int(j) for j in np.nonzero(r)[0]) for r in adj[g]]
            assert [sum(1 << int(j) for j in np.nonzero(r)[0]) for r in got[g]] == [mpr_set(rows, v) for v in range(n)]
