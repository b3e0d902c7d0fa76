"""GPU parity of the episode stream WITH scripted agents: the device sampler also draws World._sample_scripted_agents'
``np_random.choice(N, k, replace=False)`` (core.py:197-215,395), bit for bit with ``EpisodeSampler`` (the numpy
restatement the golden env traces pin to the reference), so the loops, collectors and the training CLI run mixed
populations for as long as they like instead of stopping when a 16-episode host table is used up."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.trace_replay import set_int, set_ints
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


@pytest.mark.parametrize("n,ratio,heuristic,fixed", [(20, 0.5, "mpr", False), (50, 0.25, "simple_broadcast", False),
                                                     (64, 0.9, "silent", False), (100, 0.4, "mpr", False),
                                                     (70, 0.5, None, False), (20, 0.5, "broadcast_if_any_interested", True)])
def test_device_sampler_draws_the_scripted_sets(n, ratio, heuristic, fixed):
    from melissa_amd import _lib as L
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.env.episodes import movement_offsets
    from melissa_amd.env.stream import EpisodeStream
    B, K, seed, max_moves, discard = 9, 5, 123, 7, 2
    dynamic = not fixed                         # (a fixed graph streams only when it is static)
    graphs = synthetic_graph_pool(n, 4, first_seed=3)
    kw = dict(graph=graphs[0]) if fixed else dict(graph_pool=graphs)
    venv = HipGraphVectorEnv(B, n, dynamic_graph=dynamic, device="cuda", max_moves=max_moves, construct_like_reference=False,
                             scripted_agents_ratio=ratio, heuristic=heuristic, **kw)
    total = 4 * K + 3
    want = []
    for b in range(B):
        sampler = venv.make_sampler(seed + b)
        want.append([sampler.sample() for _ in range(total + discard)])
    st = EpisodeStream(venv, seed, ring=K, discard=discard)
    assert st.n_scripted == int(round(ratio * n))
    cursor = venv.scalars()[:, L.S_EP_CURSOR]
    checked, sizes = 0, set()
    for cur in range(0, total - K + 2):
        cursor.fill_(cur)                      # pretend every env has started `cur` episodes
        st.refill()
        torch.cuda.synchronize()
        assert (st.produced.cpu().numpy() == cur + K - 1).all()
        t = {k: v.cpu().numpy() for k, v in st.pool.tensors.items()}
        for b in range(B):
            for j in range(max(0, cur - 1), cur + K - 1):          # every live slot of the ring
                slot = b * K + j % K
                ep = want[b][j + discard]
                g = graphs[ep.graph_index]
                assert set_int(t["scripted"][slot]) == ep.scripted, (b, j)
                assert t["origin"][slot] == ep.origin and set_int(t["interested"][slot]) == ep.interested, (b, j)
                assert not (ep.scripted >> ep.origin) & 1
                sizes.add(bin(ep.scripted).count("1"))
                np.testing.assert_array_equal(t["pos"][slot], g.pos)
                np.testing.assert_array_equal(t["one_hop"][slot].view(np.uint64), g.one_hop)
                if dynamic:
                    np.testing.assert_array_equal(t["moves"][slot], movement_offsets(ep.movement_seed, n, max_moves))
                checked += 1
    assert checked > 100 and sizes <= {st.n_scripted, st.n_scripted - 1} and len(sizes) == 2    # the source was drawn sometimes
    # the generators themselves: numpy's PCG64 state after the same number of samplings
    pcg = st.pcg.cpu().numpy().view(np.uint64)
    half = st.pcg_half.cpu().numpy().view(np.uint32)
    for b in range(B):
        sampler = venv.make_sampler(seed + b)
        for _ in range(int(st.produced[b]) + discard):
            sampler.sample()
        ref = sampler.np_random.bit_generator.state
        assert (int(pcg[b, 1]) << 64 | int(pcg[b, 0])) == ref["state"]["state"]
        assert int(half[b, 0]) == ref["has_uint32"] and (not ref["has_uint32"] or int(half[b, 1]) == ref["uinteger"])


@pytest.mark.parametrize("n", [20, 50, 100])
@pytest.mark.parametrize("heuristic", ["mpr", "simple_broadcast", "broadcast_if_any_interested", "silent"])
def test_round_loop_on_the_scripted_stream_matches_oracle(heuristic, n):
    """RoundLoop with its default supply (the device stream) against the CPU oracle env that draws its own episodes from
    the same generator: identical state after every one of 120 rounds, far beyond the first ring."""
    from melissa_amd import _lib as L
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.networks import HLDGNNetwork
    from melissa_amd.policy import DQNPolicy
    from oracle import env_oracle as eo
    from oracle import net_oracle as no
    from tests.mpr_oracle import MprOracleGraphEnv
    from tests.test_gpu_round import oracle_round
    B = 4 if n <= 50 else 3                     # (the Python oracles set the price of this test)
    seed, rounds, ring = 41, 120, 5
    ratio = 0.5 if heuristic == "mpr" else 0.4
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    skw = dict(scripted_agents_ratio=ratio, heuristic=heuristic)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=48,
                             construct_like_reference=False, **skw)
    net = HLDGNNetwork(5, 128, 2, 4, n, aggregator="max", dueling_param=DUEL(), device="cuda", backend="hip")
    net.load_state_dict(no.init_weights("hl_dgn", seed=9, random_conv_bias=True))
    loop = RoundLoop(venv, DQNPolicy(net), eps=0.0, seed=seed, ring=ring, discard=1)
    assert loop.supply.kind == "device stream" and loop.pool.struct.snapshot
    oracle_cls = MprOracleGraphEnv if heuristic == "mpr" else eo.OracleGraphEnv
    refs = []
    for b in range(B):
        env = oracle_cls(n, graph_pool=[eo.GraphSpec(g.pos.copy(), set_ints(g.one_hop)) for g in graphs], dynamic_graph=True,
                         np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b))), **skw)
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count = env, n, [0] * n, 0
        env.last()
        refs.append(pz)
    scripted_sets = set()
    for it in range(rounds):
        live = loop.live.cpu().numpy().view(np.uint64).copy()
        sets = venv.node_sets().cpu().numpy().view(np.uint64)
        for b, pz in enumerate(refs):
            assert set_int(sets[b, L.SET_SCRIPTED]) == pz.env.scripted, (it, b)
            assert set_int(live[b]) & pz.env.scripted == 0, (it, b)
            scripted_sets.add((b, pz.env.scripted))
        loop.step()
        torch.cuda.synchronize()
        act = loop.act.cpu().numpy().reshape(B, n)
        for b, pz in enumerate(refs):
            oracle_round(pz, {a: act[b, a] for a in range(n) if (set_int(live[b]) >> a) & 1})
        s = venv.node_sets().cpu().numpy().view(np.uint64)
        mat = venv.obs_matrix().cpu().numpy()
        pos = venv.positions().cpu().numpy()
        rf = venv.received_from().cpu().numpy().view(np.uint64) if heuristic == "mpr" else None
        for b, pz in enumerate(refs):
            e = pz.env
            assert set_int(s[b, L.SET_HAS_MESSAGE]) == e.has_message and set_int(s[b, L.SET_AGENTS]) == e.agents, (it, b)
            assert set_int(s[b, L.SET_SCRIPTED]) == e.scripted, (it, b)
            np.testing.assert_array_equal(pos[b], e.pos)
            np.testing.assert_array_equal(mat[b].reshape(n, 8), e.obs_matrix)
            if rf is not None:
                assert set_ints(rf[b]) == e.received_from, (it, b)
    assert loop.counters()["errors"] == 0
    cursors = venv.scalars()[:, L.S_EP_CURSOR].cpu().numpy()
    print(f"episodes started per env: {cursors.tolist()}")
    assert int(cursors.min()) > ring                       # every env left its first ring: the refills supplied the rest
    assert len(scripted_sets) > B * ring                   # ... each with a scripted set of its own


def test_collector_runs_past_the_old_sixteen_episode_table():
    """64 envs x 40 episodes with mpr scripted agents through the reference's collector surface: the default supply is the
    device stream, so nothing runs out (a 16-episode host table raised MEL_ENV_ERR_EPISODE_UNDERRUN here)."""
    from melissa_amd.collect import MultiAgentCollector
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy, MultiAgentSharedPolicy
    from tests.test_gpu_round import make_ldgn
    n, B = 20, 64
    net, _ = make_ldgn(n)
    venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 4, first_seed=50), dynamic_graph=True, device="cuda",
                             max_moves=48, seed=5, construct_like_reference=False, scripted_agents_ratio=0.5, heuristic="mpr")
    col = MultiAgentCollector(n, policy=MultiAgentSharedPolicy(DQNPolicy(net), venv), env=venv)
    res = col.collect(n_episode=B * 40)
    assert res.n_collected_episodes >= 2560
    assert col.loop.supply.kind == "device stream" and col.loop.counters()["errors"] == 0


@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn"])
def test_long_scripted_run_never_replays_an_episode(model):
    """The scripted twin of test_gpu_stream.test_long_run_never_replays_an_episode: thousands of resets through a 7-slot
    ring, no error flag, and at the end every checked env's ring holds the protocol's episodes for its last ordinals -
    scripted sets included (a skipped or extra draw anywhere would leave the sequential generator somewhere else)."""
    from melissa_amd import _lib as L
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.env.episodes import movement_offsets
    from melissa_amd.networks import HLDGNNetwork, LDGNNetwork
    from melissa_amd.policy import DQNPolicy
    n, B, K, seed, rounds, max_moves = 20, 96, 7, 31, 700, 48
    graphs = synthetic_graph_pool(n, 9, first_seed=1)
    torch.manual_seed(1)
    if model == "l_dgn":
        net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip")
    else:
        net = HLDGNNetwork(5, 128, 2, 4, n, aggregator="max", dueling_param=DUEL(), device="cuda", backend="hip")
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=True, device="cuda", max_moves=max_moves,
                             construct_like_reference=False, scripted_agents_ratio=0.5, heuristic="simple_broadcast")
    loop = RoundLoop(venv, DQNPolicy(net), seed=seed, eps=0.2, ring=K, use_graph=True)
    loop.run(rounds)
    torch.cuda.synchronize()
    c = loop.counters()
    sc = venv.scalars().cpu().numpy()
    assert c["errors"] == 0 and (sc[:, L.S_ERROR] == 0).all() and c["episodes"] > 20 * B
    produced = loop.supply.produced.cpu().numpy()
    assert (sc[:, L.S_EP_CURSOR] == sc[:, L.S_EPISODES_DONE] + 1).all()
    assert (produced > sc[:, L.S_EP_CURSOR]).all() and (produced <= sc[:, L.S_EP_CURSOR] + K - 1).all()
    t = {k: v.cpu().numpy() for k, v in loop.supply.pool.tensors.items()}
    for b in range(0, B, 7):
        sampler = venv.make_sampler(seed + b)
        eps = [sampler.sample() for _ in range(int(produced[b]))]
        for j in range(int(sc[b, L.S_EP_CURSOR]) - 1, int(produced[b])):          # the running episode and the ones ahead
            slot = b * K + j % K
            assert set_int(t["scripted"][slot]) == eps[j].scripted and eps[j].scripted != 0
            assert t["origin"][slot] == eps[j].origin and set_int(t["interested"][slot]) == eps[j].interested
            np.testing.assert_array_equal(t["moves"][slot], movement_offsets(eps[j].movement_seed, n, max_moves))
    assert loop.supply.describe()["refills"] >= rounds // loop.supply.period


@pytest.mark.parametrize("model", ["hl_dgn", "dgn_r"])
def test_training_with_scripted_agents(model):
    from melissa_amd.train import train
    out = train(model=model, n_nodes=12, envs=48, updates=4, rounds_per_update=3, batch_size=32, log=lambda *_: None,
                heuristic="mpr", scripted_agents_ratio=0.5)
    assert out["errors"] == 0 and out["replicas_identical"]
    assert np.isfinite(out["loss_first"]) and np.isfinite(out["loss_last"])
    assert out["episode_supply"]["mode"] == "device stream"
    assert out["heuristic"] == "mpr" and out["scripted_agents_ratio"] == 0.5
