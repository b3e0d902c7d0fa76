"""Prioritized experience replay on the MI355X (the reference's ``--prio-buffer``; parity unpinned): the three launches -
refresh, sample, write-back - against the NumPy restatement (tests/prio_oracle.py), the draws re-derived from splitmix64, the
captured update against the eager one, and ``train(prio_buffer=True)`` for the six models."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.prio_oracle import EPS, PrioOracle, draw_u
from tests.test_gpu_round import DUEL
from tests.test_prio_replay import test_abi_errors_touch_no_device_data  # noqa: F401  (check 6 runs here too)

N_STEP, GAMMA = 4, 0.99


def _filled(n, B, K=16, rounds=40, neighbours=False, **kw):
    """A PrioritizedRoundReplay filled by the round loop as in tests/test_gpu_round.py::test_replay_sampling_and_dqn_learner
    (ring full)."""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.networks import LDGNNetwork
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.replay import PrioritizedRoundReplay
    torch.manual_seed(0)
    net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="auto")
    policy = DQNPolicy(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=N_STEP, target_update_freq=2)
    venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 4, first_seed=5), dynamic_graph=True, device="cuda",
                             max_moves=48, construct_like_reference=False)
    replay = PrioritizedRoundReplay(B, n, K, "cuda", neighbours=neighbours, **kw)
    loop = RoundLoop(venv, policy, episodes_per_env=10, seed=3, eps=0.3, replay=replay)
    with torch.no_grad():
        loop.run(rounds)
    torch.cuda.synchronize()
    assert int(replay.cursor.min()) >= K
    return replay, loop, policy


def _key(rp, b):
    return ((b["env"] * rp.K + b["slot"]) * rp.n + b["agent"]).cpu().numpy()


def _acted(rp) -> np.ndarray:
    return rp._members(rp.acted).cpu().numpy()                                     # [B, K, N] bool


def _written(c0, c1, K):
    """(env, slot) of the records written while the cursors went from c0 to c1."""
    return [(e, int(c % K)) for e, (a, b) in enumerate(zip(c0.tolist(), c1.tolist())) for c in range(max(a, b - K), b)]


def _uneven_td(b, B, rng):
    """TD errors spanning 0.01 - 30, large in the first quarter of the envs: their priority mass ends up far above the others'."""
    env = b["env"].cpu().numpy()
    mag = np.where(env < B // 4, rng.uniform(10.0, 30.0, env.size), rng.uniform(0.01, 0.3, env.size))
    return torch.from_numpy((mag * rng.choice([-1.0, 1.0], env.size)).astype(np.float32)).cuda()


def _assert_draws_exact(prio, seed, draw, rp, b):
    """Check 1: every sampled transition satisfies excl[idx] - tol <= u * total < incl[idx] + tol on the float64 cumsum of the
    priorities, tol = T * 2^-52 * total (the reordering error of a float64 sum of T non-negative terms: all the device scan may do
    differently from np.cumsum).  Returns the closest distance to a boundary, in units of total."""
    flat = np.asarray(prio, np.float32).astype(np.float64).reshape(-1)
    incl = np.cumsum(flat)
    excl, total = incl - flat, incl[-1]
    tol = flat.size * 2.0 ** -52 * total
    idx = _key(rp, b)
    t = draw_u(seed, draw, idx.size) * total
    assert (flat[idx] > 0).all()
    lo, hi = t - excl[idx], incl[idx] - t
    print(f"draws: closest to a boundary {min(lo.min(), hi.min()) / total:.3e} of total, tol {tol / total:.3e}")
    assert (lo >= -tol).all() and (hi > -tol).all(), (lo.min(), hi.min(), tol)
    return min(lo.min(), hi.min()) / total


def _assert_slow_walk(rp, s):
    """ret / boot_w / obs / boot_obs / act of every sample against a slow walk over the records (the uniform sampler's checks)."""
    K = rp.K
    acted, done = _acted(rp), rp._members(rp.done).cpu().numpy()
    rew, epi, cur = rp.rew.cpu().numpy(), rp.episode.cpu().numpy(), rp.cursor.cpu().numpy()
    act_all, obs_next = rp.act.cpu().numpy(), rp.obs_next.cpu().numpy()
    cols = [s[x].cpu().numpy() for x in ("env", "slot", "agent", "ret", "boot_w", "obs", "act", "boot_obs")]
    for e, k, a, ret, bw, obs, act, boot_obs in zip(*cols):
        assert acted[e, k, a] and obs[-1] == a and act == act_all[e, k, a] and boot_obs[-1] == a
        want, w, kk, newest, boot = 0.0, 1.0, k, (cur[e] - 1) % K, k
        for j in range(N_STEP):
            if epi[e, kk] != epi[e, k] or not acted[e, kk, a]:
                break
            want += GAMMA ** j * rew[e, kk, a]
            w, boot = GAMMA ** (j + 1), kk
            if done[e, kk, a]:
                w = 0.0
                break
            if kk == newest:
                break
            kk = (kk + 1) % K
        assert abs(ret - want) < 1e-5 and abs(bw - w) < 1e-6
        np.testing.assert_array_equal(boot_obs[:-1], obs_next[e, boot])
    np.testing.assert_array_equal(s["obs"][:, :-1].cpu().numpy(), rp.obs[s["env"], s["slot"]].cpu().numpy())


@pytest.mark.parametrize("n,B", [(20, 32), (70, 8)])
def test_draws_are_exact_and_follow_the_priority_mass(n, B):
    """Checks 1 and 2."""
    rp, _, _ = _filled(n, B, neighbours=True)
    rng = np.random.RandomState(1)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for _ in range(8):                                       # several write-backs, TD errors 0.01 - 30, uneven over the envs
        b = rp.sample(1024, N_STEP, GAMMA, gen)
        rp.update_weight(b, _uneven_td(b, B, rng))
    for bs in (256, 1024, 1):
        draw = int(rp._draws)
        s = rp.sample(bs, N_STEP, GAMMA, gen)
        assert int(rp._draws) == draw + 1
        _assert_draws_exact(rp.prio.cpu().numpy(), 7, draw, rp, s)
        _assert_slow_walk(rp, s)
        acted = torch.from_numpy(_acted(rp)).cuda()
        sib = rp._members(s["nb_sibling"])
        assert bool((sib & ~acted[s["env"], s["slot"]]).sum() == 0) and bool(sib[torch.arange(bs), s["agent"]].all())
    # distribution: 64 batches of 1 024 against the per-env priority mass; the same draws must FAIL the uniform expectation
    draws = torch.cat([rp.sample(1024, N_STEP, GAMMA, gen)["env"] for _ in range(64)]).cpu().numpy()
    freq = np.bincount(draws, minlength=B).astype(np.float64)
    mass = rp.prio.double().sum((1, 2)).cpu().numpy()
    pairs = _acted(rp).sum((1, 2)).astype(np.float64)
    chi2 = lambda w: float(((freq - w / w.sum() * freq.sum()) ** 2 / (w / w.sum() * freq.sum())).sum())
    print(f"chi2 against the priority mass {chi2(mass):.1f}, against the pair counts {chi2(pairs):.1f}, bound {2.0 * B}")
    assert chi2(mass) < 2.0 * B, (chi2(mass), B)             # B - 1 degrees of freedom: mean B - 1, sd ~ sqrt(2 B)
    assert chi2(pairs) >= 2.0 * B, (chi2(pairs), B)          # ... and it is not the uniform sampler


@pytest.mark.parametrize("n,B", [(20, 32), (70, 8)])
def test_weights_and_write_back_follow_the_restatement(n, B):
    """Check 3."""
    rp, loop, _ = _filled(n, B, alpha=0.6, beta=0.4)
    K = rp.K
    ref = PrioOracle((B, K, n), alpha=0.6, beta=0.4)
    ref.add_records(_acted(rp), [(e, k) for e in range(B) for k in range(K)])
    rng = np.random.RandomState(2)
    gen = torch.Generator(device="cuda").manual_seed(11)
    worst_p = worst_w = 0.0

    def compare():
        nonlocal worst_p
        got = rp.prio.cpu().numpy().reshape(-1).astype(np.float64)
        assert ((got == 0) == (ref.tree == 0)).all()
        nz = ref.tree != 0
        worst_p = max(worst_p, float(np.abs(got[nz] / ref.tree[nz] - 1).max()))
        np.testing.assert_allclose(got, ref.tree, rtol=1e-6)
        assert float(rp.max_prio) == np.float32(ref.max_prio) and float(rp.min_prio) == np.float32(ref.min_prio)

    for it in range(6):
        if it == 3:                                          # the loop overwrites ring slots: lazily back at max_prio ** alpha
            c0 = rp.cursor.cpu().numpy()
            with torch.no_grad():
                loop.run(3)
            ref.add_records(_acted(rp), _written(c0, rp.cursor.cpu().numpy(), K))
        b = rp.sample(256, N_STEP, GAMMA, gen)
        assert torch.equal(rp.seen, rp.cursor)
        compare()
        idx = _key(rp, b)
        assert len(np.unique(idx)) < idx.size                # duplicates: with replacement, 256 of a few thousand
        want = ref.get_weight(idx)
        worst_w = max(worst_w, float(np.abs(b["weight"].cpu().numpy() / want - 1).max()))
        np.testing.assert_allclose(b["weight"].cpu().numpy(), want, rtol=1e-6)
        td = _uneven_td(b, B, rng)
        if it == 1:
            td[7] = 0.0                                      # p = eps
        rp.update_weight(b, td)
        ref.update_weight(idx, td.cpu().numpy())             # (numpy keeps the last of a repeated index)
        compare()
    print(f"max relative deviation: priorities {worst_p:.3e}, weights {worst_w:.3e}")
    assert float(rp.min_prio) == EPS and float(rp.max_prio) > 20
    # a hand-made batch that names one transition three times: the last wins
    e, k = 1, 2
    a = int(np.nonzero(_acted(rp)[e, k])[0][0])
    dup = dict(env=torch.tensor([e, e, e], device="cuda"), slot=torch.tensor([k, k, k], device="cuda"),
               agent=torch.tensor([a, a, a], device="cuda"))
    rp.update_weight(dup, torch.tensor([5.0, 0.25, -0.5], device="cuda"))
    np.testing.assert_allclose(float(rp.prio[e, k, a]), (np.float32(0.5) + EPS) ** np.float32(0.6), rtol=1e-6)
    # determinism: the same state and seed twice -> the same bits in batch and priorities
    state = [t.clone() for t in (rp.prio, rp.seen, rp.max_prio, rp.min_prio, rp._draws)]
    runs = []
    for _ in range(2):
        for t, s in zip((rp.prio, rp.seen, rp.max_prio, rp.min_prio, rp._draws), state):
            t.copy_(s)
        b = rp.sample(512, N_STEP, GAMMA, gen)
        rp.update_weight(b, (b["ret"] * 3.0 + 0.01))
        runs.append({**{key: v.clone() for key, v in b.items()}, "prio": rp.prio.clone(), "max": rp.max_prio.clone(),
                     "min": rp.min_prio.clone()})
    for key in runs[0]:
        assert torch.equal(runs[0][key], runs[1][key]), key


@pytest.mark.parametrize("model", ["l_dgn", "dgn_r", "n_dgn_r"])
def test_captured_prioritized_update_equals_the_eager_update(model):
    """Check 4: tests/test_gpu_round.py::test_captured_update_equals_the_eager_update with a prioritized replay - the twin learns on
    ``last_batch`` including ``weight``; the priorities after every replay are the restatement's write-back of the twin's TD
    error, and every replay's draw is consistent with the priorities the previous one wrote."""
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.replay import PrioritizedRoundReplay
    from melissa_amd.train import build_network, policy_and_learner
    n, envs, K = 20, 64, 16
    policy_cls, learner_cls, neighbours = policy_and_learner(model)

    def make_policy():
        torch.manual_seed(3)
        net = build_network(model, n, "cuda")
        return net, policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=3)

    net, policy = make_policy()
    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 8, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=11, construct_like_reference=False)
    replay = PrioritizedRoundReplay(envs, n, K, "cuda", neighbours=neighbours)
    loop = RoundLoop(venv, policy, seed=11, eps=0.1, replay=replay)
    with torch.no_grad():
        loop.run(20)
    learner = learner_cls(policy, replay, batch_size=32, n_step=4, gamma=0.99, seed=2)
    learner.capture()
    assert bool((replay.prio[replay.prio > 0] != 1).any())   # the warm-up updates wrote priorities back
    twin_net, twin = make_policy()
    for k in range(5):                                       # covers two target syncs (every 3 updates; 2 warm-up updates ran)
        twin_net.load_state_dict(net.state_dict())
        twin.model_old.load_state_dict(policy.model_old.state_dict())
        twin.optim.load_state_dict(copy.deepcopy(policy.optim.state_dict()))
        twin._iter = policy._iter
        # the restatement starts from the device's state: what the previous replay wrote + what the loop recorded since
        ref = PrioOracle((envs, K, n))
        ref.tree = replay.prio.cpu().numpy().reshape(-1).astype(np.float64)
        ref.max_prio, ref.min_prio = float(replay.max_prio), float(replay.min_prio)
        ref.add_records(_acted(replay), _written(replay.seen.cpu().numpy(), replay.cursor.cpu().numpy(), K))
        draw = int(replay._draws)
        out = learner.step()
        batch = {key: v.clone() for key, v in learner.last_batch.items()}
        assert {"weight", "td_error", "env", "slot", "agent"} <= set(batch)
        _assert_draws_exact(ref.tree, 2, draw, replay, batch)
        idx = _key(replay, batch)
        np.testing.assert_allclose(batch["weight"].cpu().numpy(), ref.get_weight(idx), rtol=1e-6)
        graph_td = batch["td_error"].clone()
        want = twin.learn(batch)                             # (leaves the twin's TD error in batch["td_error"])
        assert abs(float(out["loss"]) - want["loss"]) <= 1e-5 * max(1.0, abs(want["loss"]))
        for (name, p), q in zip(net.named_parameters(), twin_net.parameters()):
            diff = float((p.detach() - q.detach()).abs().max())
            assert diff <= 2e-6, (k, name, diff)
        for p, q in zip(policy.model_old.parameters(), twin.model_old.parameters()):
            assert torch.equal(p, q)
        ref.update_weight(idx, batch["td_error"].cpu().numpy())
        np.testing.assert_allclose(replay.prio.cpu().numpy().reshape(-1), ref.tree, rtol=1e-6)
        torch.testing.assert_close(graph_td, batch["td_error"], rtol=1e-5, atol=1e-6)
        if k in (1, 3):
            with torch.no_grad():
                loop.run(2)                                  # new records between two replays: the graph's refresh initialises them
    assert loop.counters()["errors"] == 0


# param_checksum of train(model, n_nodes=20, envs=64, updates=4, rounds_per_update=4, batch_size=32) on the commit before the
# prioritized replay existed, recorded with a one-off run on an MI355X: (captured, eager; the capture takes two more updates)
PARENT_CHECKSUM = {
    "l_dgn": (-87.3504633918744, 33.241879931551566),
    "hl_dgn": (28.90502093091203, 24.2058172304466),
    "dgn_r": (-349.09570708085437, -58.15954297284638),
    "n_dgn_r": (-205.8777324138115, -90.96784158303505),
    "l_n_dgn_r": (-294.96322977960034, -160.2990136535694),
    "hl_n_dgn_r": (-47.24773013998373, -46.25309754480378),
}


@pytest.mark.parametrize("captured", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn", "dgn_r", "n_dgn_r", "l_n_dgn_r", "hl_n_dgn_r"])
def test_train_with_and_without_the_prioritized_buffer(model, captured):
    """Check 5."""
    from melissa_amd.replay import PrioritizedRoundReplay
    from melissa_amd.train import train
    seen = {}

    def probe(k, net, learner, phase):
        seen["replay"] = learner.replay

    kw = dict(model=model, n_nodes=20, envs=64, updates=4, rounds_per_update=4, batch_size=32, log=lambda *_: None,
              capture_updates=captured)
    out = train(prio_buffer=True, probe=probe, **kw)
    assert out["prio_buffer"] and out["errors"] == 0 and out["updates_from_hip_graphs"] == captured
    assert np.isfinite(out["loss_first"]) and np.isfinite(out["loss_last"]) and np.isfinite(out["param_checksum"])
    rp = seen["replay"]
    assert isinstance(rp, PrioritizedRoundReplay)
    p = rp.prio[rp.prio > 0]
    assert p.numel() > 1000 and bool((p != 1).any()) and bool(torch.isfinite(p).all())
    assert float(rp.max_prio) >= 1.0 >= float(rp.min_prio) > 0 and float(rp.min_prio) < float(rp.max_prio)
    out = train(prio_buffer=False, **kw)
    print(f"{model} {'captured' if captured else 'eager'}: param_checksum {out['param_checksum']!r}, "
          f"parent {PARENT_CHECKSUM[model][0 if captured else 1]!r}")
    assert not out["prio_buffer"]
    assert out["param_checksum"] == PARENT_CHECKSUM[model][0 if captured else 1]
