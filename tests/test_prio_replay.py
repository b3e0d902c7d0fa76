"""Prioritized experience replay on the host (the reference's ``--prio-buffer``: [3P] tianshou PrioritizedVectorReplayBuffer,
l_dgn.py:169-176; parity unpinned): ``PrioritizedRoundReplay``'s torch formulation against the NumPy restatement
(tests/prio_oracle.py), the weighted losses of the three policies, the learners' write-back, ``reset_buffer`` and the training
script's flags.  No GPU."""
import numpy as np
import pytest
import torch

from melissa_amd.env.episodes import int_to_set
from melissa_amd.networks import DGNRNetwork, LDGNNetwork
from melissa_amd.policy import DGNPolicy, DQNPolicy, NDGNPolicy
from melissa_amd.replay import DGNLearner, DQNLearner, NDGNLearner, PrioritizedRoundReplay, RoundReplay
from tests.prio_oracle import EPS, PrioOracle

HEADS = lambda: ({"hidden_sizes": [64]}, {"hidden_sizes": [64]})


def _words(m: int, n: int) -> torch.Tensor:
    w = torch.from_numpy(np.atleast_1d(int_to_set(m, n)).view(np.int64).copy())
    return w if n > 64 else w[0]


def _write_round(rp, rng, r):
    """One more round for every env, the way mel_env_round fills the ring (tests/test_host_logic.py::_filled_round_replay)."""
    n = rp.n
    for e in range(rp.B):
        k = r % rp.K
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
        if rp.active_nb is not None:
            rp.active_nb[e, k] = 0
            for a in range(n):
                if (acted >> a) & 1:
                    rp.active_nb[e, k, a] = _words(int(sum(1 << j for j in range(n) if j != a and rng.rand() < 0.4)), n)


def _filled(n=6, n_envs=3, cap=5, rounds=7, seed=0, neighbours=False, **kw):
    rng = np.random.RandomState(seed)
    rp = PrioritizedRoundReplay(n_envs, n, cap, "cpu", neighbours=neighbours, **kw)
    for r in range(rounds):
        _write_round(rp, rng, r)
    return rp, rng


def _acted(rp) -> np.ndarray:
    return rp._members(rp.acted).numpy()                                           # [B, K, N] bool


def _key(rp, b):
    return ((b["env"] * rp.K + b["slot"]) * rp.n + b["agent"]).numpy()


@pytest.mark.parametrize("n", [6, 70])
def test_fresh_buffer_every_transition_is_one_and_weights_are_one(n):
    rp, _ = _filled(n)
    assert float(rp.max_prio) == 1.0 and float(rp.min_prio) == 1.0
    b = rp.sample(64, 4, 0.99, torch.Generator().manual_seed(1))
    acted = _acted(rp)
    np.testing.assert_array_equal(rp.prio.numpy(), acted.astype(np.float32))       # 1.0 ** alpha where an agent acted, 0 elsewhere
    np.testing.assert_array_equal(b["weight"].numpy(), np.ones(64, np.float32))
    assert b["weight"].dtype == torch.float32
    assert acted[b["env"], b["slot"], b["agent"]].all()
    assert set(b) >= {"obs", "act", "ret", "boot_obs", "boot_w", "env", "slot", "agent", "weight"}
    assert torch.equal(rp.seen, rp.cursor)


@pytest.mark.parametrize("n", [6, 70])
def test_update_weight_and_sample_follow_the_restatement(n):
    rp, rng = _filled(n, alpha=0.7, beta=0.5)
    acted = _acted(rp)
    ref = PrioOracle((rp.B, rp.K, rp.n), alpha=0.7, beta=0.5)
    ref.add_records(acted, [(e, k) for e in range(rp.B) for k in range(rp.K)])
    gen = torch.Generator().manual_seed(3)
    for it in range(6):
        b = rp.sample(48, 4, 0.99, gen)
        idx = _key(rp, b)
        assert acted[b["env"], b["slot"], b["agent"]].all()                        # acting agents in filled slots only
        np.testing.assert_allclose(b["weight"].numpy(), ref.get_weight(idx), rtol=1e-6)
        td = torch.from_numpy((rng.uniform(0.01, 30.0, 48) * rng.choice([-1.0, 1.0], 48)).astype(np.float32))
        if it == 2:
            td[5] = 0.0                                                            # p = eps exactly: the smallest priority there is
        rp.update_weight(b, td)
        ref.update_weight(idx, td.numpy())
        np.testing.assert_allclose(rp.prio.numpy().reshape(-1), ref.tree, rtol=1e-6)
        assert float(rp.max_prio) == np.float32(ref.max_prio) and float(rp.min_prio) == np.float32(ref.min_prio)
        assert (rp.prio.numpy()[~acted] == 0).all()
    assert float(rp.min_prio) == EPS and float(rp.max_prio) > 20.0
    # sampling follows the priorities: the empirical distribution of 40 000 draws against the priority mass per env
    draws = torch.cat([rp.sample(1000, 4, 0.99, gen)["env"] for _ in range(40)]).numpy()
    mass = rp.prio.double().sum((1, 2)).numpy()
    expect = mass / mass.sum() * draws.size
    chi2 = float(((np.bincount(draws, minlength=rp.B) - expect) ** 2 / expect).sum())
    assert chi2 < 2.0 * rp.B + 10.0, chi2                                          # B - 1 degrees of freedom (B = 3: 99.9 % < 13.8)


def test_duplicate_indices_keep_the_last_and_extremes_follow():
    rp, _ = _filled(6)
    rp.refresh()
    e, k = 1, 2
    a = int(np.nonzero(_acted(rp)[e, k])[0][0])
    batch = dict(env=torch.tensor([e, e, 0, e]), slot=torch.tensor([k, k, 0, k]),
                 agent=torch.tensor([a, a, int(np.nonzero(_acted(rp)[0, 0])[0][0]), a]))
    td = torch.tensor([5.0, -0.25, 2.0, 0.5])
    rp.update_weight(batch, td)
    np.testing.assert_allclose(float(rp.prio[e, k, a]), (np.float32(0.5) + EPS) ** np.float32(0.6), rtol=1e-6)    # the LAST of the three
    assert abs(float(rp.prio[e, k, a]) - 5.0 ** 0.6) > 1.0 and abs(float(rp.prio[e, k, a]) - 0.25 ** 0.6) > 0.1
    assert float(rp.max_prio) == float(np.float32(5.0) + EPS) and float(rp.min_prio) == float(np.float32(0.25) + EPS)
    rp.update_weight(batch, torch.tensor([0.3, 0.3, 0.3, 0.3]))
    assert float(rp.max_prio) == float(np.float32(5.0) + EPS)                      # max_prio / min_prio never move back
    with pytest.raises(ValueError):
        rp.update_weight(batch, torch.zeros(3))


def test_a_record_overwritten_by_the_ring_is_back_at_max_prio():
    rp, rng = _filled(6, rounds=5)                                                 # ring exactly full, cursor = 5
    gen = torch.Generator().manual_seed(0)
    b = rp.sample(32, 4, 0.99, gen)
    rp.update_weight(b, torch.full((32,), 9.0))
    before = rp.prio.clone()
    _write_round(rp, rng, 5)                                                       # overwrites slot 0 of every env
    _write_round(rp, rng, 6)                                                       # ... and slot 1
    rp.sample(8, 4, 0.99, gen)
    acted = _acted(rp)
    assert float(rp.max_prio) == float(np.float32(9.0) + EPS)
    init = (np.float32(9.0) + EPS) ** np.float32(0.6)                              # max_prio ** alpha, float32
    for k in (0, 1):
        np.testing.assert_allclose(rp.prio[:, k].numpy(), np.where(acted[:, k], init, np.float32(0)), rtol=1e-6)
        assert (rp.prio[:, k].numpy()[~acted[:, k]] == 0).all()
    assert torch.equal(rp.prio[:, 2:], before[:, 2:])                              # untouched records keep what was written back
    # a partially filled ring: unfilled slots hold no priority and are never sampled
    part, _ = _filled(6, cap=8, rounds=3)
    s = part.sample(200, 4, 0.99, gen)
    assert int(s["slot"].max()) <= 2 and (part.prio[:, 3:] == 0).all()


def _net(cls, n):
    torch.manual_seed(4)
    return cls(5, 32, 2, 2, n, dueling_param=HEADS(), device="cpu", backend="torch")


def _grads(net):
    return torch.cat([p.grad.flatten() for p in net.parameters()])


def test_policies_weighted_loss_is_mean_of_td_squared_times_weight():
    n, bs = 6, 7
    rng = np.random.RandomState(2)
    w = torch.from_numpy(rng.uniform(0.1, 1.0, bs).astype(np.float32))
    returns = torch.from_numpy(rng.uniform(-1, 1, bs).astype(np.float32))
    # DQNPolicy
    net = _net(LDGNNetwork, n)
    policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3))
    obs = torch.from_numpy(np.concatenate([rng.rand(bs, 8 * n), rng.randint(0, n, (bs, 1))], 1).astype(np.float32))
    act = torch.from_numpy(rng.randint(0, 2, bs))
    plain = dict(obs=obs, act=act, returns=returns)
    loss0 = policy.loss_backward(plain)
    g0 = _grads(net).clone()
    td = plain["td_error"]
    q = net(obs)[0].detach()[torch.arange(bs), act]
    torch.testing.assert_close(td, returns - q)
    torch.testing.assert_close(loss0, td.pow(2).mean())                            # without a weight: today's value
    assert "weight" not in plain
    weighted = dict(plain, weight=w)
    loss1 = policy.loss_backward(weighted)
    torch.testing.assert_close(loss1, (td.pow(2) * w).mean())
    assert not torch.allclose(_grads(net), g0)
    ones = policy.loss_backward(dict(plain, weight=torch.ones(bs)))
    assert torch.equal(ones, loss0) and torch.equal(_grads(net), g0)               # weight 1 = no weight, bit for bit
    huber = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), clip_loss_grad=True)
    assert torch.equal(huber.loss_backward(dict(plain, weight=w)), huber.loss_backward(dict(plain)))    # weight unused
    # DGNPolicy / NDGNPolicy, dense form
    for cls in (DGNPolicy, NDGNPolicy):
        net = _net(DGNRNetwork, n)
        policy = cls(net, torch.optim.Adam(net.parameters(), lr=1e-3))
        dense = dict(obs_matrix=torch.from_numpy(rng.rand(bs, 8 * n).astype(np.float32)),
                     act_all=torch.from_numpy(rng.randint(0, 2, (bs, n))), sibling=torch.from_numpy(rng.rand(bs, n) < 0.5),
                     returns=returns)
        loss0 = policy.loss_backward(dense)
        td = dense["td_error"]                                                     # the dense form hands the TD error back too
        assert td.shape == (bs,) and "weight" not in dense
        torch.testing.assert_close(loss0, td.pow(2).mean())
        torch.testing.assert_close(policy.loss_backward(dict(dense, weight=w)), (td.pow(2) * w).mean())


def _learner_case(kind, n):
    neighbours = kind == "n_dgn"
    rp, rng = _filled(n, n_envs=4, cap=6, rounds=9, neighbours=neighbours)
    net = _net(LDGNNetwork if kind == "dqn" else DGNRNetwork, n)
    policy_cls, learner_cls = {"dqn": (DQNPolicy, DQNLearner), "dgn": (DGNPolicy, DGNLearner), "n_dgn": (NDGNPolicy, NDGNLearner)}[kind]
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=2)
    return rp, learner_cls(policy, rp, batch_size=16, n_step=4, gamma=0.99, seed=5)


@pytest.mark.parametrize("kind", ["dqn", "dgn", "n_dgn"])
def test_three_learner_steps_move_exactly_the_sampled_priorities(kind):
    rp, learner = _learner_case(kind, 6)
    ref = PrioOracle((rp.B, rp.K, rp.n))
    ref.add_records(_acted(rp), [(e, k) for e in range(rp.B) for k in range(rp.K)])
    for _ in range(3):
        out = learner.step()
        b = learner.last_batch
        assert np.isfinite(out["loss"]) and b["weight"].shape == (16,) and b["td_error"].shape == (16,)
        idx = _key(rp, b)
        np.testing.assert_allclose(b["weight"].numpy(), ref.get_weight(idx), rtol=1e-6)
        ref.update_weight(idx, b["td_error"].numpy())
        np.testing.assert_allclose(rp.prio.numpy().reshape(-1), ref.tree, rtol=1e-6)       # the sampled ones moved, nothing else
        assert float(rp.max_prio) == np.float32(ref.max_prio) and float(rp.min_prio) == np.float32(ref.min_prio)
    assert (rp.prio[rp.prio > 0] != 1).any()


def test_uniform_replay_learners_are_unchanged():
    """Without a prioritized replay no batch carries a weight and nothing is written anywhere."""
    from tests.test_host_logic import _filled_round_replay
    rp = _filled_round_replay()
    net = _net(LDGNNetwork, 6)
    learner = DQNLearner(DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4), rp, batch_size=8, seed=1)
    learner.step()
    assert "weight" not in learner.last_batch and "env" not in learner.last_batch and not hasattr(rp, "prio")
    assert type(rp) is RoundReplay


def test_collectors_reset_buffer_returns_priorities_to_their_initial_state():
    from melissa_amd.collect import MultiAgentCollector
    rp, _ = _filled(6)
    b = rp.sample(16, 4, 0.99, torch.Generator().manual_seed(0))
    rp.update_weight(b, torch.linspace(0.01, 30, 16))
    assert float(rp.max_prio) > 1 and float(rp.min_prio) < 1 and int(rp.seen.min()) > 0
    col = MultiAgentCollector.__new__(MultiAgentCollector)                         # (reset_buffer only touches the buffer)
    col.buffer = rp
    col.reset_buffer()
    assert int(rp.cursor.max()) == 0 and int(rp.seen.max()) == 0 and float(rp.prio.abs().max()) == 0
    assert float(rp.max_prio) == 1.0 and float(rp.min_prio) == 1.0
    with pytest.raises(ValueError):
        rp.sample(4, 4, 0.99)                                                      # empty again
    with pytest.raises(ValueError):
        PrioritizedRoundReplay(2, 6, 4, "cpu", alpha=-0.1)


def test_train_argument_parser_has_the_references_flags():
    import inspect
    from melissa_amd import train
    a = train.arg_parser().parse_args([])
    assert (a.prio_buffer, a.alpha, a.beta) == (False, 0.6, 0.4)                   # common.py:52,64-65
    a = train.arg_parser().parse_args(["--prio-buffer", "--alpha", "0.5", "--beta", "1", "--model", "hl_n_dgn_r"])
    assert (a.prio_buffer, a.alpha, a.beta, a.model) == (True, 0.5, 1.0, "hl_n_dgn_r")
    sig = inspect.signature(train.train).parameters
    assert (sig["prio_buffer"].default, sig["alpha"].default, sig["beta"].default) == (False, 0.6, 0.4)


def test_abi_errors_touch_no_device_data():
    """mel_replay_sample_prio / mel_replay_update_priority refuse bad arguments before any launch (the pointers here are host
    memory that a launch would fault on; nothing reads them)."""
    import ctypes as C
    from melissa_amd import _lib
    lib = _lib.load()
    host = (C.c_double * 64)()
    ptr = C.addressof(host)

    def filled(cls, **over):
        s = cls()
        for name, typ in cls._fields_:
            if typ is C.c_void_p:
                setattr(s, name, ptr)
        for name, v in over.items():
            setattr(s, name, v)
        return s

    replay = filled(_lib.MelRoundReplay, capacity=4, active_nb=None)
    out = filled(_lib.MelReplayBatch, nb_sibling=None)
    disc = (C.c_float * 5)(1, 1, 1, 1, 1)
    good = dict(alpha=0.6, beta=0.4, weight_norm=1)

    def sample(pr, batch=8, replay=replay, out=out, weight=ptr, n_step=4):
        return lib.mel_replay_sample_prio(C.byref(replay) if replay is not None else None, C.byref(pr) if pr is not None else None,
                                          2, 6, batch, n_step, disc, 1, ptr, C.byref(out), weight, None)

    def update(pr, batch=8, env=ptr, td=ptr):
        return lib.mel_replay_update_priority(C.byref(pr) if pr is not None else None, 2, 4, 6, batch, env, ptr, ptr, td, None)

    for call in (sample, update):
        assert call(None) == _lib.ERR_INVALID_ARG and b"null" in lib.mel_last_error()
        assert call(filled(_lib.MelReplayPriority, seen=None, **good)) == _lib.ERR_INVALID_ARG
        assert b"incomplete priority block" in lib.mel_last_error()
        assert call(filled(_lib.MelReplayPriority, alpha=-0.1, beta=0.4)) == _lib.ERR_INVALID_ARG and b"alpha" in lib.mel_last_error()
        assert call(filled(_lib.MelReplayPriority, alpha=0.6, beta=-1.0)) == _lib.ERR_INVALID_ARG and b"beta" in lib.mel_last_error()
        for batch in (0, 1025):
            assert call(filled(_lib.MelReplayPriority, **good), batch=batch) == _lib.ERR_INVALID_ARG
            assert b"batch in [1, 1024]" in lib.mel_last_error()
    pr = filled(_lib.MelReplayPriority, **good)
    assert sample(pr, replay=None) == _lib.ERR_INVALID_ARG and sample(pr, weight=None) == _lib.ERR_INVALID_ARG
    assert sample(pr, replay=filled(_lib.MelRoundReplay, capacity=4, rew=None)) == _lib.ERR_INVALID_ARG
    assert sample(pr, out=filled(_lib.MelReplayBatch, agent=None)) == _lib.ERR_INVALID_ARG
    assert sample(pr, out=filled(_lib.MelReplayBatch)) == _lib.ERR_INVALID_ARG and b"active_nb" in lib.mel_last_error()
    assert sample(pr, n_step=17) == _lib.ERR_INVALID_ARG
    assert update(pr, env=None) == _lib.ERR_INVALID_ARG and b"missing" in lib.mel_last_error()
    assert update(pr, td=None) == _lib.ERR_INVALID_ARG
    assert C.sizeof(_lib.MelReplayPriority) == lib.mel_abi_sizeof(13) == 72
    assert all(v == 0 for v in host)
