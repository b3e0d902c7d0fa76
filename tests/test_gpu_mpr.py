"""GPU parity of the "mpr" scripted-agent heuristic: mel_mpr_sets against the reference's recorded sets and the
restatement (tests/mpr_oracle.py), the env kernels against the reference's GraphEnv traces, and the round loop against
MprOracleGraphEnv."""
import glob
import os

import numpy as np
import pytest
import torch

from tests.mpr_oracle import MprOracleGraphEnv, mpr_sets_batch
from tests.test_gpu_env import OneEnvAdapter, build_venv
from tests.trace_replay import replay, set_int, set_ints

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SETS = sorted(glob.glob(os.path.join(GOLDEN, "mpr_sets_*.npz")))
TRACES = sorted(glob.glob(os.path.join(GOLDEN, "mpr_trace_*.npz")))
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


def to_words(adj: np.ndarray) -> np.ndarray:
    """bool [G, N, N] -> uint64 node sets [G, N] ([G, N, W] beyond 64 nodes)."""
    g, n, _ = adj.shape
    w = (n + 63) // 64
    padded = np.zeros((g, n, 64 * w), dtype=np.uint64)
    padded[:, :, :n] = adj
    words = (padded.reshape(g, n, w, 64) << np.arange(64, dtype=np.uint64)).sum(axis=3, dtype=np.uint64)
    return words[:, :, 0] if n <= 64 else words


def to_bool(words: np.ndarray, n: int) -> np.ndarray:
    w = words.reshape(words.shape[0], n, -1).astype(np.uint64)
    return ((w[:, :, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).reshape(w.shape[0], n, -1)[:, :, :n].astype(bool)


def device_sets(words: np.ndarray) -> np.ndarray:
    from melissa_amd.env import mpr_sets
    out = mpr_sets(torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("path", SETS, ids=[os.path.basename(p)[9:-4] for p in SETS])
def test_mpr_sets_kernel_equals_reference(path):
    f = np.load(path)
    got = device_sets(f["adj"])
    np.testing.assert_array_equal(got, f["mpr"])


def random_graphs(n, count, rng):
    """Half connected random geometric graphs (radius 0.2 from 50 nodes up, wider below so that they connect), half
    Erdos-Renyi graphs of mixed density with a few isolated nodes."""
    out = []
    radius = 0.2 * max(1.0, (50.0 / n) ** 0.5)
    while len(out) < count // 2:
        p = rng.uniform(size=(n, 2))
        d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2)
        adj = d <= radius * radius
        np.fill_diagonal(adj, False)
        seen, frontier = {0}, [0]
        while frontier:
            frontier = [j for i in frontier for j in np.nonzero(adj[i])[0] if j not in seen and not seen.add(j)]
        if len(seen) == n:
            out.append(adj)
    while len(out) < count:
        adj = np.triu(rng.uniform(size=(n, n)) < rng.choice([0.02, 0.05, 0.1, 0.25, 0.6]), 1)
        adj = adj | adj.T
        iso = rng.choice(n, size=rng.randint(0, max(2, n // 8)), replace=False)
        adj[iso] = False
        adj[:, iso] = False
        out.append(adj)
    return np.stack(out)


@pytest.mark.parametrize("n", [7, 20, 50, 63, 64, 65, 100, 128])
def test_mpr_sets_kernel_equals_restatement_on_random_graphs(n):
    adj = random_graphs(n, 500, np.random.RandomState(n))
    got = device_sets(to_words(adj))
    want = to_words(mpr_sets_batch(adj))
    np.testing.assert_array_equal(got, want)
    assert to_bool(got, n).any()


def trace_state(pz, tr, venv, k):
    row = [0]

    def state():
        r = row[0]
        row[0] += 1
        rf = venv.received_from()[k].cpu().numpy().view(np.uint64)
        assert set_ints(rf) == set_ints(tr["received_from"][r]), f"row {r} received_from"
        return pz.state()
    return state, row


@pytest.mark.parametrize("path", TRACES, ids=[os.path.basename(p)[10:-4] for p in TRACES])
def test_hip_env_matches_reference_mpr_trace(path):
    tr = np.load(path)
    venv = build_venv(tr)
    pz = OneEnvAdapter(venv, 0)
    state, row = trace_state(pz, tr, venv, 0)
    rows = replay(tr, pz, state)
    assert rows >= 300 and row[0] == rows
    assert int(venv.scalars()[0, 11]) == 0


def test_hip_env_mpr_trace_in_a_busy_batch():
    """The traced env (testing mode, every node scripted: relay forwards) in slot 5 of 9 envs stepped in the same launches."""
    tr = np.load(os.path.join(GOLDEN, "mpr_trace_n20_testing_dynamic.npz"))
    venv = build_venv(tr, env_num=9, slot=5)
    rng = np.random.RandomState(0)
    venv.reset([i for i in range(9) if i != 5])

    class Busy(OneEnvAdapter):
        def step(self, a):
            others = [i for i in range(9) if i != 5]
            obs, rew, term, trunc, info = self.venv.step(rng.randint(0, 2, size=8), others)
            for i, t, inf in zip(others, term, info):
                if t and inf.get("explicit_reset"):
                    self.venv.reset([i])
            return super().step(a)

    busy = Busy(venv, 5)
    state, _ = trace_state(busy, tr, venv, 5)
    assert replay(tr, busy, state) >= 300
    assert int(venv.scalars()[:, 11].abs().sum()) == 0


@pytest.mark.parametrize("n,ratio,testing", [(20, 0.4, False), (50, 0.4, False), (100, 0.4, False), (20, 1.0, True),
                                             (100, 1.0, True)])
def test_hldgn_round_loop_with_mpr_matches_oracle(n, ratio, testing):
    """HL-DGN round loop (reset snapshots, as RoundLoop builds them for a table) with mpr scripted agents: env state and
    received_from after every round equal MprOracleGraphEnv replaying the same actions.  In training mode the scripted
    nodes only get relay duties (the source is never scripted, so no scripted node ever forwards); in testing mode with
    every node scripted the source starts the chain and relays forward."""
    from melissa_amd import _lib as L
    from melissa_amd.collect import RoundLoop, sample_episode_table
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.networks import HLDGNNetwork
    from melissa_amd.policy import DQNPolicy
    from oracle import env_oracle as eo
    from oracle import net_oracle as no
    from tests.test_gpu_round import TOL, oracle_round
    B, seed, K = 5, 41, 30
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    skw = dict(scripted_agents_ratio=ratio, heuristic="mpr")
    tkw = dict(is_testing=True, num_test_episodes=8) if testing else {}
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=48,
                             construct_like_reference=False, **skw, **tkw)
    sd = no.init_weights("hl_dgn", seed=9, random_conv_bias=True)
    net = HLDGNNetwork(5, 128, 2, 4, n, aggregator="max", dueling_param=DUEL(), device="cuda", backend="hip")
    net.load_state_dict(sd)
    packed, table = sample_episode_table(venv, 12, seed)
    loop = RoundLoop(venv, DQNPolicy(net), eps=0.0, seed=seed, episodes=(packed, np.ascontiguousarray(table[:, 1:])))
    assert loop.pool.struct.snapshot                     # episode ends load the reset snapshots
    refs = []
    for b in range(B):
        env = MprOracleGraphEnv(n, graph_pool=[eo.GraphSpec(g.pos.copy(), set_ints(g.one_hop)) for g in graphs],
                                dynamic_graph=True,
                                np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b))), **skw, **tkw)
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count = env, n, [0] * n, 0
        env.last()
        env.forwards = env.relay_duties = 0
        refs.append(pz)
    for it in range(K):
        live = loop.live.cpu().numpy().view(np.uint64).copy()
        mat = venv.obs_matrix().cpu().numpy().copy()
        loop.step()
        torch.cuda.synchronize()
        logits = loop.logits.cpu().numpy()
        act = loop.act.cpu().numpy().reshape(B, n)
        obs_rows = np.concatenate([mat, np.zeros((B, 1), np.float32)], axis=1)
        np.testing.assert_allclose(logits, no.hldgn_forward(sd, obs_rows, n, aggregator="max").numpy(), atol=TOL, rtol=0)
        for b, pz in enumerate(refs):
            oracle_round(pz, {a: act[b, a] for a in range(n) if (set_int(live[b]) >> a) & 1})
        s = venv.node_sets().cpu().numpy().view(np.uint64)
        rf = venv.received_from().cpu().numpy().view(np.uint64)
        mat = venv.obs_matrix().cpu().numpy()
        for b, pz in enumerate(refs):
            assert set_int(s[b, L.SET_HAS_MESSAGE]) == pz.env.has_message, (it, b)
            assert set_int(s[b, L.SET_AGENTS]) == pz.env.agents and set_int(s[b, L.SET_SCRIPTED]) == pz.env.scripted
            assert set_ints(rf[b]) == pz.env.received_from, (it, b)
            np.testing.assert_array_equal(mat[b].reshape(n, 8), pz.env.obs_matrix)
            np.testing.assert_array_equal(venv.positions()[b].cpu().numpy(), pz.env.pos)
    assert loop.counters()["errors"] == 0
    assert sum(pz.env.relay_duties for pz in refs) > 0
    if testing:
        assert sum(pz.env.forwards for pz in refs) > 0
    assert sum(len(getattr(pz, "finished", [])) for pz in refs) > 0      # episodes ended: snapshots were loaded


def test_venv_mpr_sets_follow_the_current_graphs():
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    n = 50
    venv = HipGraphVectorEnv(6, n, graph_pool=synthetic_graph_pool(n, 4, 3), dynamic_graph=True, device="cuda", seed=1,
                             scripted_agents_ratio=0.5, heuristic="mpr")
    venv.reset()
    rng = np.random.RandomState(1)
    for _ in range(12):
        venv.step(rng.randint(0, 2, size=6))
    hop = venv.one_hop().cpu().numpy().view(np.uint64)
    got = venv.mpr_sets().cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got, to_words(mpr_sets_batch(to_bool(hop, n))))


def test_watch_with_mpr_scripted_agents():
    from melissa_amd.watch import watch
    out = watch(model="hl_dgn", n_nodes=20, envs=64, episodes=64, heuristic="mpr", scripted_agents_ratio=1.0)
    assert out["n/ep"] >= 64 and 0.0 < out["coverage"] <= 1.0 and out["total_messages_transmitted"] >= 1
