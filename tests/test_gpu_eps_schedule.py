"""The exploration schedule on the device: mel_exploration_schedule against the host formula, the fused selections reading
eps from device memory, a replayed round graph that follows the schedule, and ``train(epoch=...)`` - evaluation, checkpoints,
resume - on top of them."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from melissa_amd.collect import EpsSchedule, exploration_eps

# eps is evaluated in double and rounded ONCE to float, as np.float32(exploration_eps(...)) is; the device's exp() form and the
# reference's pow() form of the expression differ by < 1e-9 (tests/test_train_epochs.py), so the two roundings can land on
# neighbouring floats at most: one float ulp at 1.0, the largest value eps takes
EPS_TOL = 1.2e-7
DEFAULTS = (1.0, 0.05, 0.6, 10, 100000)                          # the reference's command-line defaults: horizon 600 000
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


def launch_schedule(decisions, n_envs, scale=1, sched=DEFAULTS, rounds=None, trace=None):
    """decisions: CUDA int32 [n_envs, 16] (the counters in column MEL_S_DECISIONS, like mel_env_batch.scalars) -> status,
    env_step, eps.  trace: (env_step int64 [cap], eps float32 [cap]) device ring."""
    from melissa_amd import _lib
    eps = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
    step = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    eps_train, eps_final, fraction, epoch, step_per_epoch = sched
    st = _lib.load().mel_exploration_schedule(
        decisions.data_ptr() + 4 * _lib.S_DECISIONS, _lib.ENV_SCALARS, n_envs, scale, eps_train, eps_final, fraction,
        float(epoch * step_per_epoch), rounds.data_ptr() if rounds is not None else None, eps.data_ptr(), step.data_ptr(),
        trace[0].numel() if trace is not None else 0, trace[0].data_ptr() if trace is not None else None,
        trace[1].data_ptr() if trace is not None else None, _lib.current_stream_ptr())
    return st, int(step.item()), np.float32(eps.item())


def scalars_with(decisions):
    """[n, 16] int32 with random junk in every other column."""
    rng = np.random.RandomState(len(decisions))
    sc = rng.randint(-5, 1 << 20, size=(len(decisions), 16)).astype(np.int32)
    sc[:, 8] = decisions
    return torch.from_numpy(sc).cuda()


@pytest.mark.parametrize("n_envs", [1, 3, 64, 65, 1025])
def test_schedule_kernel_matches_the_formula(n_envs):
    from melissa_amd import _lib
    assert _lib.S_DECISIONS == 8 and _lib.ENV_SCALARS == 16
    rng = np.random.RandomState(n_envs)
    horizon = 600000
    # totals spread over the decay and past its end
    for total_target in (0, 1, horizon // 7, horizon // 2, horizon, 3 * horizon):
        dec = rng.multinomial(total_target, np.ones(n_envs) / n_envs).astype(np.int32) if total_target else np.zeros(n_envs, np.int32)
        st, env_step, eps = launch_schedule(scalars_with(dec), n_envs)
        assert st == _lib.OK
        assert env_step == int(dec.astype(np.int64).sum()) == total_target
        want = np.float32(exploration_eps(env_step, *DEFAULTS))
        print(f"n_envs {n_envs} env_step {env_step} eps {eps!r} want {want!r} diff {abs(float(eps) - float(want)):.3e}")
        assert abs(float(eps) - float(want)) <= EPS_TOL
    assert launch_schedule(scalars_with(np.zeros(n_envs, np.int32)), n_envs)[2] == np.float32(1.0)
    # scale: every decision stands for `scale` env steps
    dec = rng.randint(0, 2 * (horizon // 3) // n_envs + 1, size=n_envs).astype(np.int32)
    st, env_step, eps = launch_schedule(scalars_with(dec), n_envs, scale=3)
    assert st == _lib.OK and env_step == 3 * int(dec.astype(np.int64).sum())
    assert abs(float(eps) - float(np.float32(exploration_eps(env_step, *DEFAULTS)))) <= EPS_TOL


@pytest.mark.parametrize("scale", [1, 2])
def test_schedule_kernel_sums_past_32_bits(scale):
    from melissa_amd import _lib
    n_envs, each = 1025, 4194304
    st, env_step, eps = launch_schedule(scalars_with(np.full(n_envs, each, np.int32)), n_envs, scale=scale)
    assert st == _lib.OK
    assert env_step == scale * n_envs * each and env_step > 1 << 32
    assert eps == np.float32(0.05) == np.float32(exploration_eps(env_step, *DEFAULTS))


def test_schedule_trace_ring_wraps():
    from melissa_amd import _lib
    cap, n_envs = 4, 65
    trace = (torch.full((cap,), -1, dtype=torch.int64, device="cuda"), torch.full((cap,), -1.0, dtype=torch.float32, device="cuda"))
    rounds = torch.zeros(1, dtype=torch.int32, device="cuda")
    calls = []
    for r in range(6):
        rounds.fill_(r)
        dec = np.full(n_envs, 1000 * (r + 1), np.int32)
        st, env_step, eps = launch_schedule(scalars_with(dec), n_envs, rounds=rounds, trace=trace)
        assert st == _lib.OK and env_step == 65000 * (r + 1)
        calls.append((env_step, eps))
        if r == 2:                                              # three calls in: slot 3 untouched
            assert trace[0].cpu().tolist() == [65000, 130000, 195000, -1] and float(trace[1][3]) == -1.0
    got_step, got_eps = trace[0].cpu().numpy(), trace[1].cpu().numpy()
    for slot, r in enumerate([4, 5, 2, 3]):                     # rounds 4 and 5 overwrote rounds 0 and 1
        assert got_step[slot] == calls[r][0] and got_eps[slot] == calls[r][1]
    # no round counter: slot 0
    st, env_step, eps = launch_schedule(scalars_with(np.full(n_envs, 7, np.int32)), n_envs, trace=trace)
    assert st == _lib.OK and int(trace[0][0]) == env_step == 455 and trace[0].cpu().tolist()[1:] == [c[0] for c in (calls[5], calls[2], calls[3])]


def test_schedule_rejects_invalid_arguments():
    from melissa_amd import _lib
    sc = scalars_with(np.arange(3, dtype=np.int32))
    for bad in [(1.0, 0.05, 0.0, 10, 100000),                   # horizon <= 0
                (1.0, 0.05, 0.6, 0, 100000),
                (1.0, 0.05, -0.5, 10, 100000),
                (1.0, 0.0, 0.6, 10, 100000),                    # eps_final <= 0
                (1.0, -0.1, 0.6, 10, 100000),
                (0.04, 0.05, 0.6, 10, 100000)]:                 # eps_final > eps_train
        st, env_step, eps = launch_schedule(sc, 3, sched=bad)
        assert st == _lib.ERR_INVALID_ARG, bad
        assert env_step == -1 and eps == np.float32(-1.0)       # nothing was launched
    assert launch_schedule(sc, 3, sched=(0.05, 0.05, 0.6, 10, 100000))[0] == _lib.OK      # a constant schedule is one
    torch.cuda.synchronize()


def random_obs_matrix(rng, bs, n):
    m = np.zeros((bs, n, 8), dtype=np.float32)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, 9, size=(bs, n))
    m[:, :, 3] = rng.randint(0, 4, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.1)
    return m


def random_node_sets(rng, bs, n):
    """Mixed live sets (one env with none) as int64 words [bs] / [bs, 2]."""
    member = rng.randint(0, 2, size=(bs, n)).astype(bool)
    member[1] = False
    words = np.zeros((bs, (n + 63) // 64), dtype=np.uint64)
    for b, a in zip(*np.nonzero(member)):
        words[b, a // 64] |= np.uint64(1) << np.uint64(a % 64)
    words = words[:, 0] if n <= 64 else words
    return torch.from_numpy(words.view(np.int64)).cuda(), member


@pytest.mark.parametrize("model,n,bs", [("l_dgn", 12, 5), ("hl_dgn", 20, 4), ("hl_dgn", 70, 3), ("l_dgn", 70, 3)])
def test_selection_reads_eps_from_the_device(model, n, bs):
    """eps_dev -> x (with a different host eps next to it) selects, bit for bit, what eps = x selects without eps_dev."""
    from melissa_amd import _lib
    from melissa_amd.networks import HLDGNNetwork, LDGNNetwork
    torch.manual_seed(4)
    if model == "l_dgn":
        net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip")
    else:
        net = HLDGNNetwork(5, 128, 2, 4, n, aggregator="max", dueling_param=DUEL(), device="cuda", backend="hip")
    rng = np.random.RandomState(n + bs)
    obs = torch.from_numpy(random_obs_matrix(rng, bs, n).reshape(bs, n * 8)).cuda()
    live, member = random_node_sets(rng, bs, n)
    rounds = torch.tensor([5], dtype=torch.int32, device="cuda")
    eps_dev = torch.zeros(1, dtype=torch.float32, device="cuda")

    def run(host_eps, device_eps):
        act = torch.full((bs * n,), -1, dtype=torch.int32, device="cuda")
        sel = _lib.MelSelect()
        sel.act, sel.eps, sel.seed, sel.step_dev = act.data_ptr(), host_eps, 1234, rounds.data_ptr()
        if device_eps is not None:
            eps_dev.fill_(device_eps)
            sel.eps_dev = eps_dev.data_ptr()
        with torch.no_grad():
            if model == "l_dgn":
                logits, offsets = net.hip_forward_agents(obs, live, bs * n, select=sel)
                logits = logits[:int(offsets[-1])]
            else:
                sel.live, sel.n_nodes = live.data_ptr(), n
                logits = net.hip_forward_envs(obs, select=sel)
        return act.cpu().numpy(), logits.cpu().numpy()

    acts = {}
    for eps in (0.0, 0.3, 1.0):
        act_dev, logits_dev = run(0.9, eps)
        act_host, logits_host = run(eps, None)
        np.testing.assert_array_equal(act_dev, act_host)
        np.testing.assert_array_equal(logits_dev, logits_host)
        chosen = act_host >= 0
        assert chosen.sum() == member.sum()
        if model != "l_dgn":                                    # dense [bs, n] layout: exactly the live agents got an action
            np.testing.assert_array_equal(chosen.reshape(bs, n), member)
        acts[eps] = act_host
    # (the rate matters at all: fully random and greedy selections differ somewhere among these dozens of agents)
    assert (acts[0.0] != acts[1.0]).any()


def run_round_loop(use_graph, schedule, rounds, per_round=None):
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.networks import LDGNNetwork
    from melissa_amd.policy import DQNPolicy
    n, B = 20, 8
    torch.manual_seed(11)
    net = LDGNNetwork(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip")
    venv = HipGraphVectorEnv(B, n, graph_pool=synthetic_graph_pool(n, 4, first_seed=5), dynamic_graph=True, device="cuda",
                             max_moves=48, construct_like_reference=False)
    loop = RoundLoop(venv, DQNPolicy(net), seed=3, eps=0.5, use_graph=use_graph, graph_rounds=4, eps_schedule=schedule)
    if per_round is not None:
        for _ in range(rounds):
            per_round(loop)
            loop.run(1)
    else:
        loop.run(rounds)
    torch.cuda.synchronize()
    state = [venv.scalars().cpu().numpy().copy(), venv.node_sets().cpu().numpy().copy(), venv.positions().cpu().numpy().copy(),
             loop.act.cpu().numpy().copy()]
    return loop, state


def test_graph_replay_follows_the_schedule():
    """26 rounds - one eager, the capture, six replays of the four-round graph, one of the one-round graph - walk the trajectory
    of 26 eager rounds, eps falling from eps_train to the floor on the way with nothing recaptured."""
    rounds = 26
    probe, _ = run_round_loop(False, None, rounds)                 # how many decisions such a run produces (eps = 0.5 throughout)
    produced = probe.counters()["decisions"]
    assert produced > 100
    schedule = EpsSchedule(eps_train=1.0, eps_final=0.05, exploration_fraction=0.5, epoch=1, step_per_epoch=produced, trace=32)
    horizon = 0.5 * produced
    before = []
    eager, eager_state = run_round_loop(False, schedule, rounds, per_round=lambda loop: before.append(loop.counters()["decisions"]))
    graph, graph_state = run_round_loop(True, schedule, rounds)
    assert graph.graph is not None and graph.group_graph is not None and eager.graph is None
    for mine, theirs in zip(eager_state, graph_state):
        np.testing.assert_array_equal(mine, theirs)
    assert eager.counters() == graph.counters() and eager.counters()["errors"] == 0 and eager.counters()["iterations"] == rounds
    (step_e, eps_e), (step_g, eps_g) = eager.eps_trace(), graph.eps_trace()
    np.testing.assert_array_equal(step_e, step_g)
    np.testing.assert_array_equal(eps_e, eps_g)
    assert eager.eps_now() == graph.eps_now() == (int(step_g[rounds - 1]), float(eps_g[rounds - 1]))
    step, eps = step_g[:rounds], eps_g[:rounds]
    assert (step_g[rounds:] == 0).all()                            # 26 rounds wrote 26 slots of the 32
    assert list(step) == before                                    # each round's eps comes from the decisions taken before it
    assert (np.diff(step) >= 0).all() and step[0] == before[0] and step[-1] > horizon
    assert step[-1] < graph.counters()["decisions"] <= step[-1] + 8 * 20       # the last round's own decisions come on top
    for r in range(rounds):
        want = np.float32(exploration_eps(int(step[r]), 1.0, 0.05, 0.5, 1, produced))
        assert abs(float(eps[r]) - float(want)) <= EPS_TOL, r
    assert step[0] == 0 and eps[0] == np.float32(1.0) and eps[-1] == np.float32(0.05)
    assert (np.diff(eps) <= 0).all() and len(set(eps.tolist())) > 5     # it decays round by round in between
    # without a schedule the loop is what it was: the host value, no device eps
    assert probe.eps_schedule is None and probe._select.eps_dev is None and probe._select.eps == 0.5


TRAIN = dict(model="l_dgn", n_nodes=20, envs=8, step_per_epoch=400, test_num=3, model_name="run", log=lambda line: None)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    from melissa_amd.train import train
    logdir = tmp_path_factory.mktemp("log")
    lines = []
    out = train(epoch=2, logdir=str(logdir), **{**TRAIN, "log": lines.append})
    return out, str(logdir), lines


def test_train_in_epochs_evaluates_and_saves(trained):
    import json
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network
    from melissa_amd.watch import watch
    out, logdir, lines = trained
    assert json.loads(lines[-1])["epochs"] == out["epochs"]                    # the result line carries the epochs
    ep = out["epochs"]
    assert [e["epoch"] for e in ep] == [0, 1, 2]                               # before the first epoch and after each
    rews = [e["test_rew"] for e in ep]
    assert out["best_rew"] == max(rews) and out["best_epoch"] == rews.index(max(rews))
    assert [e["best"] for e in ep] == [i == 0 or rews[i] > max(rews[:i]) for i in range(3)]
    assert all(e["test_len"] > 0 and 0.0 < e["coverage"] <= 1.0 and e["episodes"] == 3 for e in ep)
    # epochs: step_per_epoch more env steps each, noticed one update iteration late
    for prev, e in zip(ep, ep[1:]):
        assert e["overshoot"] == e["env_step"] - (prev["env_step"] + 400) and e["overshoot"] >= 0
        assert e["overshoot"] <= 2 * 4 * 8 * 20                                # two iterations of four rounds of <= envs * nodes decisions
        assert e["updates"] >= 2
    assert out["updates"] == ep[1]["updates"] + ep[2]["updates"] and out["decisions"] == ep[2]["env_step"]
    # exploration: the horizon is 0.6 * 2 * 400 = 480 env steps, long past at the end
    assert ep[0]["eps"] > ep[1]["eps"] >= ep[2]["eps"] == float(np.float32(0.05))
    assert ep[0]["eps"] >= float(np.float32(exploration_eps(ep[0]["env_step"], 1.0, 0.05, 0.6, 2, 400))) - EPS_TOL
    assert out["errors"] == 0 and out["replicas_identical"] and np.isfinite(out["loss_last"])
    # checkpoints
    weights = os.path.join(logdir, "l_dgn", "weights")
    assert out["best_path"] == os.path.join(weights, "run_best.pth") and out["last_path"] == os.path.join(weights, "run_last.pth")
    keys = set(DQNPolicy(build_network("l_dgn", 20, "cuda"), target_update_freq=1).state_dict())
    assert all(k.startswith(("model.", "model_old.")) for k in keys) and any(k.startswith("model_old.") for k in keys)
    for path in (out["best_path"], out["last_path"]):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert set(sd) == keys
    last = torch.load(out["last_path"], map_location="cpu", weights_only=True)
    checksum = float(torch.cat([last[k].flatten() for k in last if k.startswith("model.")]).double().sum())
    assert checksum == pytest.approx(out["param_checksum"], rel=1e-12)
    seen = watch(model="l_dgn", n_nodes=20, envs=1, episodes=3, load=out["last_path"])
    assert seen["n/ep"] >= 3 and 0.0 < seen["coverage"] <= 1.0


def test_train_resumes_from_a_checkpoint(trained, tmp_path):
    from melissa_amd.train import train
    first, _, _ = trained
    again = train(epoch=1, resume_path=first["last_path"], logdir=str(tmp_path), capture_updates=False,
                  **{**TRAIN, "step_per_epoch": 100, "test_num": 2})
    assert again["param_checksum_start"] == first["param_checksum"]
    assert again["param_checksum_start"] != first["param_checksum_start"] and again["param_checksum"] != again["param_checksum_start"]
    assert [e["epoch"] for e in again["epochs"]] == [0, 1] and os.path.exists(again["last_path"])


def test_train_without_epochs_is_unchanged():
    from melissa_amd.train import train
    out = train(model="l_dgn", n_nodes=20, envs=8, updates=2, capture_updates=False, log=lambda line: None)
    assert set(out) == {"rank", "world", "model", "updates", "seconds", "loss_first", "loss_last", "decisions", "episodes",
                        "errors", "param_checksum", "updates_from_hip_graphs", "prio_buffer", "warmup_updates", "heuristic",
                        "scripted_agents_ratio", "episode_supply", "replicas_identical"}
    assert out["updates"] == 2 and out["errors"] == 0


def _two_rank_worker(rank, world, port, out_dir):
    import json
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    from melissa_amd.train import train
    out = train(backend="gloo", epoch=2, logdir=os.path.join(out_dir, "log"), **{**TRAIN, "step_per_epoch": 300, "test_num": 1})
    with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
        json.dump(out, f)
    torch.distributed.destroy_process_group()


def test_two_ranks_end_every_epoch_at_the_same_iteration(tmp_path):
    """Two ranks on one GPU (gloo): their envs differ, so do their decision counts - yet both must take the same number of
    updates in every epoch (the gradient all-reduce pairs them), from targets and counts both hold."""
    import json
    import socket
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = [mp.get_context("spawn").Process(target=_two_rank_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(150)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
    assert not hung, "a rank is stuck: the ranks left an epoch at different iterations"
    assert [p.exitcode for p in procs] == [0, 0]
    r0, r1 = (json.load(open(tmp_path / f"rank{r}.json")) for r in range(2))
    assert (r0["world"], r1["world"], r0["rank"], r1["rank"]) == (2, 2, 0, 1)
    assert r0["decisions"] != r1["decisions"]                                   # their own counts differ ...
    for a, b in zip(r0["epochs"], r1["epochs"]):                                # ... what they steer by does not
        assert (a["epoch"], a["env_step"], a["updates"], a["overshoot"]) == (b["epoch"], b["env_step"], b["updates"], b["overshoot"])
    assert [e["epoch"] for e in r0["epochs"]] == [e["epoch"] for e in r1["epochs"]] == [0, 1, 2]
    assert r0["epochs"][2]["env_step"] == 2 * min(r0["decisions"], r1["decisions"])
    assert r0["updates"] == r1["updates"] >= 2 and r0["param_checksum"] == r1["param_checksum"]
    assert r0["replicas_identical"] and r1["replicas_identical"] and r0["errors"] == r1["errors"] == 0
    assert "test_rew" in r0["epochs"][0] and "test_rew" not in r1["epochs"][0]  # rank 0 evaluates (and writes)
    assert os.path.exists(r0["last_path"]) and os.path.exists(r0["best_path"])
    for e in r0["epochs"][1:]:
        assert 0 <= e["overshoot"] <= 2 * 2 * 4 * 8 * 20                        # two iterations' decisions of both ranks
