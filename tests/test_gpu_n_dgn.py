"""N-DGN on the MI355X: the neighbour masks mel_env_round records (mel_round_replay.active_nb) against the oracle env's
``info['active_one_hop_neighbors']`` at each acting agent's next observation, the sampler's ``nb_sibling``, the first N-DGN update
against oracle autograd, the captured update against the eager one, and the three new ``train`` models end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_round import DUEL, TOL, make_ldgn
from tests.trace_replay import set_int


def _bool_to_int(mask) -> int:
    return sum(1 << j for j, v in enumerate(np.asarray(mask).tolist()) if v)


def _oracle_round_waiting(pz, act_of_agent, acting, waiting, seen):
    """One env round on the oracle in mel_env_round's order (dead steps, then each active agent), with the collective
    collector's bookkeeping (collective_experience_collector.py:270-290): the agents that acted wait for their NEXT
    observation, whose info['active_one_hop_neighbors'] is stored with their transition.  ``waiting``: agent -> record key;
    ``seen[key][agent]`` receives the mask as a Python int.  Returns the world step's outcome (None if none ran)."""
    n = pz.env.n
    outcome = None
    for _ in range(3 * n + 4):
        env = pz.env
        sel = env.agent_selection
        dead = (env.terminated >> sel) & 1
        moves = env.num_moves
        obs, rew, term, trunc, info = pz.step(0 if dead else int(act_of_agent[sel]))
        if pz.env.num_moves != moves:
            outcome = dict(obs_next=pz.env.obs_matrix.copy(), rew=list(pz.env.rewards), terminated=pz.env.terminated)
            for a in acting:                                  # their transitions now wait for the next observation
                assert a not in waiting
                waiting[a] = acting[a]
        a = int(obs["agent_id"])
        if a in waiting:
            seen[waiting.pop(a)][a] = _bool_to_int(info["active_one_hop_neighbors"])
        if term:
            pz.done_count += 1
            if info.get("explicit_reset") or pz.done_count == n:
                # every acting agent has been observed again before the episode ends: the record is complete
                assert not waiting, ("agents reach the episode end unobserved", sorted(waiting))
                pz.reset()
                pz.done_count = 0
                return outcome
        if info.get("environment_step"):
            return outcome
    raise AssertionError("round did not terminate")


def _masks_vs_oracle(n, dynamic, supply, B=6):
    from melissa_amd.collect import RoundLoop, sample_episode_table
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.replay import RoundReplay
    from oracle import env_oracle as eo
    from oracle import net_oracle as no
    seed = 77
    graphs = synthetic_graph_pool(n, 3, first_seed=50)
    venv = HipGraphVectorEnv(B, n, graph_pool=graphs, dynamic_graph=dynamic, device="cuda", max_moves=48,
                             construct_like_reference=False)
    net, sd = make_ldgn(n)
    packed, table = sample_episode_table(venv, 14, seed)
    replay = RoundReplay(B, n, 8, "cuda", neighbours=True)
    K = 40
    if supply == "stream":
        ring = 5 if n <= 20 else 3
        loop = RoundLoop(venv, DQNPolicy(net), eps=0.0, seed=seed, replay=replay, ring=ring, discard=1)
        K = 70 if n <= 50 else 110
    else:
        loop = RoundLoop(venv, DQNPolicy(net), eps=0.0, seed=seed, replay=replay,
                         episodes=({k: v for k, v in packed.items()}, np.ascontiguousarray(table[:, 1:])))
    refs = []
    for b in range(B):
        env = eo.OracleGraphEnv(n, graph_pool=[eo.GraphSpec(g.pos.copy(), [set_int(x) for x in g.one_hop]) for g in graphs],
                                dynamic_graph=dynamic,
                                np_random=np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed + b))))
        pz = eo.OraclePettingZooEnv.__new__(eo.OraclePettingZooEnv)
        pz.env, pz.n, pz.rewards, pz.done_count = env, n, [0] * n, 0
        env.last()
        refs.append(pz)
    waiting = [dict() for _ in range(B)]
    seen, recorded = {}, {}                                  # record key -> {agent: oracle mask} / device row
    checked = 0
    for it in range(K):
        live = loop.live.cpu().numpy().view(np.uint64).copy()
        mat = venv.obs_matrix().cpu().numpy().copy()
        loop.step()
        torch.cuda.synchronize()
        offsets, act = loop.offsets.cpu().numpy(), loop.act.cpu().numpy()
        logits = loop.logits.cpu().numpy()
        rows = [(b, a) for b in range(B) for a in range(n) if (set_int(live[b]) >> a) & 1]
        if rows:                                             # the actions the oracle replays are the oracle network's choices
            obs_rows = np.concatenate([mat[[b for b, _ in rows]], np.array([[a] for _, a in rows], np.float32)], axis=1)
            np.testing.assert_allclose(logits[:len(rows)], no.ldgn_forward(sd, obs_rows, n).numpy(), atol=TOL, rtol=0)
        cursor = replay.cursor.cpu().numpy()
        nb_dev = replay.active_nb.cpu().numpy()
        for b, pz in enumerate(refs):
            lv = set_int(live[b])
            acts = {a: act[offsets[b] + j] for j, a in enumerate(a for a in range(n) if (lv >> a) & 1)}
            key = (b, it)
            if lv:
                seen[key] = {}
            outcome = _oracle_round_waiting(pz, acts, {a: key for a in acts} if lv else {}, waiting[b], seen)
            if lv:
                slot = (int(cursor[b]) - 1) % replay.K
                assert outcome is not None
                # the existing fields of the record, with neighbours on
                np.testing.assert_array_equal(replay.obs[b, slot].cpu().numpy(), mat[b])
                np.testing.assert_array_equal(replay.obs_next[b, slot].cpu().numpy(), outcome["obs_next"].reshape(-1))
                assert set_int(replay.acted[b, slot].cpu().numpy().view(np.uint64)) == lv
                assert set_int(replay.done[b, slot].cpu().numpy().view(np.uint64)) == outcome["terminated"] & lv
                rec_act, rec_rew = replay.act[b, slot].cpu().numpy(), replay.rew[b, slot].cpu().numpy()
                for a_id, a_val in acts.items():
                    assert rec_act[a_id] == a_val and rec_rew[a_id] == np.float32(outcome["rew"][a_id])
                recorded[key] = [set_int(nb_dev[b, slot, j]) for j in range(n)]
        # compare every record whose acting agents have all been observed again
        for key in [k for k in seen if not any(v == k for v in waiting[k[0]].values())]:
            want, got = seen.pop(key), recorded.pop(key)
            for j in range(n):
                assert got[j] == want.get(j, 0), (key, j, hex(got[j]), hex(want.get(j, 0)))
            checked += len(want)
    c = loop.counters()
    assert c["errors"] == 0 and c["episodes"] >= 3 and checked > 100, (c, checked)
    assert len(seen) <= B                                    # only the last round's records may still wait


@pytest.mark.parametrize("n,dynamic,supply", [(12, False, "table"), (20, True, "stream"), (50, True, "table"),
                                               (70, False, "stream"), (100, True, "table")])
def test_recorded_neighbour_masks_match_the_oracle(n, dynamic, supply):
    _masks_vs_oracle(n, dynamic, supply)


def _filled_device_replay(n, envs=32, rounds=24, neighbours=True):
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.replay import RoundReplay
    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 8, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5, construct_like_reference=False)
    net, _ = make_ldgn(n)
    replay = RoundReplay(envs, n, 16, "cuda", neighbours=neighbours)
    loop = RoundLoop(venv, DQNPolicy(net), seed=5, eps=0.2, replay=replay)
    with torch.no_grad():
        loop.run(rounds)
    torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0
    return replay


@pytest.mark.parametrize("n", [20, 70])
def test_device_sampler_nb_sibling(n):
    from melissa_amd import _lib
    replay = _filled_device_replay(n)
    g = torch.Generator(device="cuda").manual_seed(7)
    b = replay.sample(256, 4, 0.99, g)
    torch.cuda.synchronize()
    e, k, a = (b[key].cpu().numpy() for key in ("env", "slot", "agent"))
    acted, nb = replay.acted.cpu().numpy(), replay.active_nb.cpu().numpy()
    got = b["nb_sibling"].cpu().numpy()
    assert got.shape == ((256,) if n <= 64 else (256, 2))
    nonempty = 0
    for i in range(256):
        s, ac = set_int(got[i]), set_int(acted[e[i], k[i]])
        assert s == ac & (set_int(nb[e[i], k[i], a[i]]) | (1 << int(a[i])))
        assert (s >> int(a[i])) & 1 and s & ~ac == 0
        nonempty += s != (1 << int(a[i]))
    assert nonempty > 0                                      # some experiences do have neighbour siblings
    # the host formulation of the same draw agrees too (RoundReplay.sample's CPU path on copies of the ring)
    host = replay.__class__(replay.B, n, replay.K, "cpu", neighbours=True)
    for name in ("obs", "obs_next", "acted", "done", "act", "rew", "episode", "cursor", "active_nb"):
        getattr(host, name).copy_(getattr(replay, name).cpu())
    hb = host.sample(64, 4, 0.99, torch.Generator().manual_seed(1))
    for i in range(64):
        ee, kk, aa = int(hb["env"][i]), int(hb["slot"][i]), int(hb["agent"][i])
        assert set_int(hb["nb_sibling"][i].numpy()) == set_int(acted[ee, kk]) & (set_int(nb[ee, kk, aa]) | (1 << aa))
    # without active_nb the launch is refused cleanly, and the replay keeps running
    plain = _filled_device_replay(n, rounds=6, neighbours=False)
    assert "nb_sibling" not in plain.sample(8, 2, 0.9)
    out = {name: torch.empty(8, 8 * n + 1, device="cuda") for name in ("obs", "boot_obs")}
    out.update({name: torch.empty(8, device="cuda") for name in ("ret", "boot_w")})
    out.update({name: torch.empty(8, dtype=torch.int64, device="cuda") for name in ("act", "env", "slot", "agent")})
    out["nb_sibling"] = torch.empty(8, *plain.acted.shape[2:], dtype=torch.int64, device="cuda")
    bt = _lib.MelReplayBatch()
    for name, t in out.items():
        setattr(bt, name, t.data_ptr())
    lib = _lib.load()
    draws = torch.zeros(1, dtype=torch.int64, device="cuda")
    scratch = torch.empty(plain.B * plain.K + 1, dtype=torch.int32, device="cuda")
    disc = (C.c_float * 3)(1.0, 0.9, 0.81)
    st = lib.mel_replay_sample(C.byref(plain.struct), plain.B, n, 8, 2, disc, 1, draws.data_ptr(), scratch.data_ptr(),
                               C.byref(bt), _lib.current_stream_ptr(torch.device("cuda")))
    assert st == _lib.ERR_INVALID_ARG and b"active_nb" in lib.mel_last_error()
    assert "nb_sibling" not in plain.sample(8, 2, 0.9)
    torch.cuda.synchronize()


@pytest.mark.parametrize("model", ["n_dgn_r", "l_n_dgn_r", "hl_n_dgn_r"])
def test_first_n_dgn_update_matches_oracle_autograd(model):
    """N = 50: the training loop's first N-DGN update re-derived by the oracle - the loss of policies/n_dgn.py:31-64 over the
    oracle forward of every restricted sibling of the sampled batch, with the pre-update weights - and its autograd gradient
    against what the HIP learn path left in .grad (each tensor within 2e-4 of its scale)."""
    from melissa_amd.train import train
    from oracle import net_oracle as no
    n = 50
    cap = {}

    def probe(k, net, learner, phase):
        if k != 0:
            return
        if phase == "before":
            cap["sd"] = {key: v.detach().cpu().clone() for key, v in net.state_dict().items()}
        else:
            cap["batch"] = {key: v.detach().cpu() for key, v in learner.last_batch.items()}
            cap["grad"] = {key: p.grad.detach().cpu().clone() for key, p in net.named_parameters() if p.grad is not None}

    out = train(model=model, n_nodes=n, envs=64, updates=2, rounds_per_update=3, batch_size=32, log=lambda *_: None, probe=probe)
    assert out["errors"] == 0 and out["decisions"] > 500
    b = cap["batch"]
    sib = b["sibling"]
    assert bool(sib[torch.arange(32), b["agent"]].all())     # every experience is its own sibling
    sd = {k: v.clone().requires_grad_(True) for k, v in cap["sd"].items()}
    torch.set_num_threads(8)
    seg, agent = torch.nonzero(sib, as_tuple=True)
    rows = torch.cat([b["obs_matrix"][seg], agent.float()[:, None]], dim=1).numpy()
    fwd = {"l_n_dgn_r": no.ldgn_forward, "n_dgn_r": no.dgnr_forward, "hl_n_dgn_r": no.hldgn_forward}[model]
    logits = fwd(sd, rows, n)
    q = logits[torch.arange(len(seg)), b["act_all"][seg, agent]]
    batch_q = torch.zeros_like(b["returns"]).index_add(0, seg, q)
    loss = (b["returns"] - batch_q).pow(2).mean()
    loss.backward()
    assert abs(float(loss.detach()) - out["loss_first"]) <= 1e-4 * max(1.0, abs(float(loss.detach()))), (float(loss), out["loss_first"])
    overall = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    compared = 0
    for k, g in ((k, v.grad) for k, v in sd.items()):
        if g is None:
            continue
        assert k in cap["grad"], k
        scale = max(float(g.abs().max()), 1e-3 * overall)
        assert float((cap["grad"][k] - g).abs().max()) <= 2e-4 * scale, (k, float((cap["grad"][k] - g).abs().max()), scale)
        compared += g.numel()
    assert compared > 100000


@pytest.mark.parametrize("model", ["n_dgn_r", "hl_n_dgn_r"])
def test_captured_n_dgn_update_equals_the_eager_update(model):
    import copy
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import NDGNPolicy
    from melissa_amd.replay import NDGNLearner, RoundReplay
    from melissa_amd.train import build_network
    n, envs = 20, 64

    def make_policy():
        torch.manual_seed(3)
        net = build_network(model, n, "cuda")
        return net, NDGNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=3)

    net, policy = make_policy()
    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 8, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=11, construct_like_reference=False)
    replay = RoundReplay(envs, n, 16, "cuda", neighbours=True)
    loop = RoundLoop(venv, policy, seed=11, eps=0.1, replay=replay)
    with torch.no_grad():
        loop.run(20)
    learner = NDGNLearner(policy, replay, batch_size=32, n_step=4, gamma=0.99, seed=2)
    learner.capture()
    twin_net, twin = make_policy()
    for k in range(5):                                       # two target syncs (every 3 updates; 2 warm-up updates ran)
        twin_net.load_state_dict(net.state_dict())
        twin.model_old.load_state_dict(policy.model_old.state_dict())
        twin.optim.load_state_dict(copy.deepcopy(policy.optim.state_dict()))
        twin._iter = policy._iter
        out = learner.step()
        batch = {key: v.clone() for key, v in learner.last_batch.items()}
        want = twin.learn(batch)
        assert abs(float(out["loss"]) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"]))
        for (name, p), q in zip(net.named_parameters(), twin_net.parameters()):
            diff = float((p.detach() - q.detach()).abs().max())
            assert diff <= 2e-6, (k, name, diff)
        with torch.no_grad():
            loop.run(2)                                      # the collect loop keeps running on the new weights
    assert loop.counters()["errors"] == 0


@pytest.mark.parametrize("model", ["n_dgn_r", "l_n_dgn_r", "hl_n_dgn_r"])
def test_training_loop_n_dgn_models(model):
    from melissa_amd.train import train
    out = train(model=model, n_nodes=12, envs=48, updates=4, rounds_per_update=3, batch_size=32, log=lambda *_: None)
    assert out["errors"] == 0 and out["decisions"] > 200 and out["replicas_identical"] and out["updates_from_hip_graphs"]
    assert np.isfinite(out["loss_first"]) and np.isfinite(out["loss_last"])


def test_collective_experience_collector_records_neighbours():
    from melissa_amd.collect import CollectiveExperienceCollector
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import MultiAgentCollaborativeSharedPolicy, NDGNPolicy
    n = 20
    venv = HipGraphVectorEnv(16, n, graph_pool=synthetic_graph_pool(n, 4, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=3, construct_like_reference=False)
    net, _ = make_ldgn(n)
    masp = MultiAgentCollaborativeSharedPolicy(NDGNPolicy(net, None), venv)
    col = CollectiveExperienceCollector(n, policy=masp, env=venv, buffer=None, exploration_noise=True, buffer_rounds=8)
    assert col.buffer.active_nb is not None and col.buffer.K == 8
    res = col.collect(n_step=200)
    assert res.n_collected_steps >= 200
    ex = col.buffer.export_transitions()
    assert ex["active_one_hop_neighbors"].shape == ex["indices"].shape and len(ex["act"]) > 0
    # a neighbour mask never names an agent outside the graph, and some transitions have neighbours
    assert ex["active_one_hop_neighbors"].any()
