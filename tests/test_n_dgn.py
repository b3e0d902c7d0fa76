"""N-DGN training on the host (policies/n_dgn.py): the neighbour-restricted sibling loss against a restatement of the reference's
loop, the replay's ``nb_sibling`` / ``active_one_hop_neighbors`` outputs, HL-DGN's all-agents form and the reference-named
constructors of the collective scripts.  No GPU."""
import inspect

import numpy as np
import pytest
import torch

from melissa_amd.env.episodes import int_to_set, set_to_int, sets_to_bool
from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork

HEADS = lambda: ({"hidden_sizes": [64]}, {"hidden_sizes": [64]})


def _words(m: int, n: int) -> torch.Tensor:
    w = torch.from_numpy(np.atleast_1d(int_to_set(m, n)).view(np.int64).copy())
    return w if n > 64 else w[0]


def _neighbour_replay(n_envs=3, n=6, cap=5, rounds=7, seed=0):
    """A RoundReplay(neighbours=True) filled on the CPU the way mel_env_round fills it, with random neighbour masks (acting
    agents only, never containing the agent itself - the env's one_hop sets exclude self)."""
    from melissa_amd.replay import RoundReplay
    rng = np.random.RandomState(seed)
    rp = RoundReplay(n_envs, n, cap, "cpu", neighbours=True)
    for r in range(rounds):
        for e in range(n_envs):
            k = r % cap
            acted = 0
            for a in rng.choice(n, size=rng.randint(1, n), replace=False):
                acted |= 1 << int(a)
            rp.acted[e, k] = _words(acted, n)
            rp.done[e, k] = _words(acted, n) if r % 4 == 3 else 0
            rp.obs[e, k] = torch.from_numpy(rng.uniform(0, 1, 8 * n).astype(np.float32))
            rp.obs_next[e, k] = torch.from_numpy(rng.uniform(0, 1, 8 * n).astype(np.float32))
            rp.act[e, k] = torch.from_numpy(rng.randint(0, 2, n).astype(np.int8))
            rp.rew[e, k] = torch.from_numpy(rng.uniform(-1, 1, n).astype(np.float32))
            rp.episode[e, k] = r // 4
            rp.cursor[e] = r + 1
            rp.active_nb[e, k] = 0
            for a in range(n):
                if (acted >> a) & 1:
                    nb = int(sum(1 << j for j in range(n) if j != a and rng.rand() < 0.4))
                    rp.active_nb[e, k, a] = _words(nb, n)
    return rp


def _make(model, n):
    torch.manual_seed(4)
    if model == "hl_dgn":
        return HLDGNNetwork(5, 32, 2, 2, n, aggregator="max", dueling_param=HEADS(), device="cpu", backend="torch")
    cls = DGNRNetwork if model == "dgn_r" else LDGNNetwork
    return cls(5, 32, 2, 2, n, dueling_param=HEADS(), device="cpu", backend="torch")


def _reference_loop(net, ex, pick, returns, huber=False):
    """policies/n_dgn.py:31-64 restated: for every experience, its siblings (info.indices >= 0) restricted to the info's
    active_one_hop_neighbors plus the agent itself, each sibling's Q from its own buffer row (first match of its index among the
    batch's active_obs.index), summed; MSE or Huber against the returns."""
    indices = ex["indices"][pick]
    active_index = indices[indices >= 0]                     # collaborative_shared_policy.py:55-59
    active_obs, active_act = ex["obs"][active_index], ex["act"][active_index]
    batch_q = []
    for i, t in enumerate(pick):
        nb = ex["active_one_hop_neighbors"][t].copy()
        nb[int(ex["obs"][t, -1])] = True
        keep = (indices[i] >= 0) & nb
        rows = [int(np.where(active_index == idx)[0][0]) for idx in indices[i][keep]]
        q = net(torch.from_numpy(active_obs[rows]))[0]
        batch_q.append(q[torch.arange(len(rows)), torch.from_numpy(active_act[rows])].sum())
    batch_q = torch.stack(batch_q)
    ret = torch.from_numpy(returns)
    if huber:
        return torch.nn.functional.huber_loss(batch_q.reshape(-1, 1), ret.reshape(-1, 1))
    return (ret - batch_q).pow(2).mean()


def _grads_match(net_a, net_b):
    for (name, pa), pb in zip(net_a.named_parameters(), net_b.parameters()):
        if pa.grad is None:
            assert pb.grad is None or float(pb.grad.abs().max()) == 0.0, name      # (dgn_r.py: lin_skip unused)
            continue
        torch.testing.assert_close(pb.grad, pa.grad, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("model", ["dgn_r", "l_dgn", "hl_dgn"])
@pytest.mark.parametrize("huber", [False, True])
def test_n_dgn_learn_equals_the_reference_loop(model, huber):
    from melissa_amd.policy import NDGNPolicy
    n = 6
    rp = _neighbour_replay(n=n)
    ex = rp.export_transitions()
    assert ex["active_one_hop_neighbors"].shape == ex["indices"].shape and ex["active_one_hop_neighbors"].dtype == np.bool_
    rng = np.random.RandomState(1)
    pick = rng.choice(len(ex["act"]), size=8, replace=False)
    returns = rng.uniform(-1, 1, size=8).astype(np.float32)
    net_a = _make(model, n)
    loss_a = _reference_loop(net_a, ex, pick, returns, huber)
    loss_a.backward()
    indices = ex["indices"][pick]
    # (b) the row form, in the reference's own layout
    net_b = _make(model, n)
    pol = NDGNPolicy(net_b, torch.optim.SGD(net_b.parameters(), lr=0.0), clip_loss_grad=huber)
    active_index = indices[indices >= 0]
    batch = dict(indices=indices, active_one_hop_neighbors=ex["active_one_hop_neighbors"][pick], agent_id=ex["agent_id"][pick],
                 active_obs=ex["obs"][active_index], active_index=active_index, active_act=ex["act"][active_index], returns=returns)
    out = pol.learn(batch)
    assert abs(out["loss"] - float(loss_a.detach())) < 1e-6
    assert batch["weight"].shape == (8,)                     # prio-buffer hook (n_dgn.py:67)
    _grads_match(net_a, net_b)
    # (c) the dense form: one graph per experience, the restricted siblings as a [B, N] mask
    net_c = _make(model, n)
    pol_c = NDGNPolicy(net_c, torch.optim.SGD(net_c.parameters(), lr=0.0), clip_loss_grad=huber)
    e, k, agent = (torch.from_numpy(ex[key][pick]) for key in ("env_id", "record_slot", "agent_id"))
    bits = torch.from_numpy(sets_to_bool(rp.acted[e, k].numpy(), n))
    nb = torch.from_numpy(ex["active_one_hop_neighbors"][pick]).clone()
    nb[torch.arange(8), agent] = True
    out_c = pol_c.learn(dict(obs_matrix=rp.obs[e, k], act_all=rp.act[e, k].long(), sibling=bits & nb,
                             returns=torch.from_numpy(returns)))
    assert abs(out_c["loss"] - float(loss_a.detach())) < 1e-6
    _grads_match(net_a, net_c)


def test_the_restriction_changes_the_loss():
    """N-DGN is not DGN-R: with neighbour masks that drop siblings, the two losses differ on the same batch."""
    from melissa_amd.policy import DGNPolicy, NDGNPolicy
    n = 6
    ex = _neighbour_replay(n=n).export_transitions()
    pick = np.arange(8)
    indices = ex["indices"][pick]
    assert (NDGNPolicy.neighbour_indices(indices, ex["active_one_hop_neighbors"][pick], ex["agent_id"][pick]) >= 0).sum() < \
        (indices >= 0).sum()
    active_index = indices[indices >= 0]
    g_dgn = DGNPolicy.segments_from_indices(indices, active_index)
    g_ndgn = NDGNPolicy.segments_from_indices(indices, active_index, ex["active_one_hop_neighbors"][pick], ex["agent_id"][pick])
    assert len(g_ndgn[0]) < len(g_dgn[0])
    assert NDGNPolicy.segments_from_indices(indices, active_index)[0].tolist() == g_dgn[0].tolist()


@pytest.mark.parametrize("n", [6, 70])
def test_host_sampler_nb_sibling(n):
    from melissa_amd.replay import RoundReplay
    rp = _neighbour_replay(n=n)
    g = torch.Generator().manual_seed(3)
    b = rp.sample(64, n_step=2, gamma=0.9, generator=g)
    assert b["nb_sibling"].shape == ((64,) if n <= 64 else (64, 2)) and b["nb_sibling"].dtype == torch.int64
    for i in range(64):
        e, k, a = int(b["env"][i]), int(b["slot"][i]), int(b["agent"][i])
        acted, nb = set_to_int(rp.acted[e, k].numpy()), set_to_int(rp.active_nb[e, k, a].numpy())
        s = set_to_int(b["nb_sibling"][i].numpy())
        assert (s >> a) & 1                                  # the experience is its own sibling
        assert s & ~acted == 0                               # only agents that acted in the round
        assert s == acted & (nb | (1 << a))
    # without neighbours the sampler keeps its old outputs
    plain = RoundReplay(2, n, 4, "cpu")
    assert plain.active_nb is None
    plain.acted[:, 0], plain.cursor[:] = _words(1, n), 1
    assert "nb_sibling" not in plain.sample(4, 1, 0.9)


def test_n_dgn_learner_on_host_tensors():
    from melissa_amd.policy import NDGNPolicy
    from melissa_amd.replay import NDGNLearner, RoundReplay
    n = 6
    rp = _neighbour_replay(n=n)
    net = _make("dgn_r", n)
    pol = NDGNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), target_update_freq=2)
    with pytest.raises(ValueError, match="neighbours=True"):
        NDGNLearner(pol, RoundReplay(3, n, 5, "cpu"))
    learner = NDGNLearner(pol, rp, batch_size=8, n_step=2, gamma=0.9, seed=1)
    batch = learner.sample_batch()
    assert batch["sibling"].shape == (8, n) and batch["sibling"].dtype == torch.bool
    for i in range(8):
        e, k, a = int(batch["env"][i]), int(batch["slot"][i]), int(batch["agent"][i])
        want = set_to_int(rp.acted[e, k].numpy()) & (set_to_int(rp.active_nb[e, k, a].numpy()) | (1 << a))
        assert [bool((want >> j) & 1) for j in range(n)] == batch["sibling"][i].tolist()
    rows = learner.row_form(batch)                           # on request only
    assert rows["segment"].numel() == int(batch["sibling"].sum())
    before = [p.detach().clone() for p in net.parameters()]
    losses = [learner.step()["loss"] for _ in range(3)]
    assert all(np.isfinite(losses)) and "segment" not in learner.last_batch
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))


@pytest.mark.parametrize("aggregator", ["max", "mean", "add"])
def test_hldgn_all_agents_form(aggregator):
    n, G = 9, 4
    torch.manual_seed(0)
    net = HLDGNNetwork(5, 32, 2, 2, n, aggregator=aggregator, dueling_param=HEADS(), device="cpu", backend="torch")
    rng = np.random.RandomState(0)
    mat = torch.from_numpy(rng.uniform(0, 1, (G, 8 * n)).astype(np.float32))
    mat.view(G, n, 8)[:, :, 7] = torch.from_numpy((rng.rand(G, n) < 0.5).astype(np.float32))      # decision-maker flags
    q_all = net.torch_forward_all_agents(mat)
    assert q_all.shape == (G, n, 2)
    for j in range(n):
        rows = torch.cat([mat, torch.full((G, 1), float(j))], dim=1)
        torch.testing.assert_close(q_all[:, j], net.torch_forward(rows), atol=1e-6, rtol=1e-6)
    q_all.sum().backward()                                   # differentiable
    assert net.encoder.model[0].weight.grad is not None


def test_train_models_and_reference_named_constructors():
    from melissa_amd import train as T
    from melissa_amd.collect import CollectiveExperienceCollector, MultiAgentCollector
    from melissa_amd.policy import (DGNPolicy, DQNPolicy, MultiAgentCollaborativeSharedPolicy, MultiAgentSharedPolicy,
                                    NDGNPolicy)
    from melissa_amd.replay import DGNLearner, DQNLearner, NDGNLearner, RoundReplay
    for name, cls in (("n_dgn_r", DGNRNetwork), ("l_n_dgn_r", LDGNNetwork), ("hl_n_dgn_r", HLDGNNetwork)):
        assert type(T.build_network(name, 12, "cpu")) is cls
        assert T.policy_and_learner(name) == (NDGNPolicy, NDGNLearner, True)
    assert T.policy_and_learner("dgn_r") == (DGNPolicy, DGNLearner, False)
    assert T.policy_and_learner("l_dgn") == T.policy_and_learner("hl_dgn") == (DQNPolicy, DQNLearner, False)
    with pytest.raises(ValueError):
        T.policy_and_learner("n_dgn")
    assert set(T.MODELS) == {"l_dgn", "hl_dgn", "dgn_r", "n_dgn_r", "l_n_dgn_r", "hl_n_dgn_r"}
    # collective_experience_collector.py:20: CollectiveExperienceCollector(agents_num, **kwargs)
    assert issubclass(CollectiveExperienceCollector, MultiAgentCollector)
    params = inspect.signature(CollectiveExperienceCollector).parameters
    assert list(params)[0] == "agents_num" and "buffer" in params
    with pytest.raises(ValueError, match="neighbours=True"):
        CollectiveExperienceCollector(12, policy=object(), env=None, buffer=RoundReplay(2, 12, 4, "cpu"))
    # collaborative_shared_policy.py:15 / n_dgn_r.py:80: MultiAgentCollaborativeSharedPolicy(policy, env)
    pol = NDGNPolicy(_make("dgn_r", 12), None)
    masp = MultiAgentCollaborativeSharedPolicy(pol, [str(i) for i in range(12)])
    assert isinstance(masp, MultiAgentSharedPolicy) and masp.policy is pol and masp.agents == [str(i) for i in range(12)]
    assert masp.agent_idx["3"] == 3
