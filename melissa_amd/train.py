"""Data-parallel DQN training over env shards: the distributed counterpart of ``train_agent``
(l_dgn.py:131-269 / hl_dgn.py / dgn_r.py: collect ``step_per_collect`` transitions, then
``update_per_step`` gradient steps).

One process per GPU (``python -m torch.distributed.run --nproc-per-node N -m melissa_amd.train ...``):
every rank owns ``envs`` independent envs (no data-path collective: rank r steps and evaluates its own
shard with the HIP kernels, device-resident replay), replicas start from rank 0's weights, and the ONE
collective of the path is the flat-gradient all-reduce (RCCL over xGMI) between backward and the Adam step,
so all replicas stay bit-identical.  Target-network sync, eps schedule and counters are replicated locally.
"""
from __future__ import annotations

import argparse
import datetime
import json
import math
import os
import time

# torch and the package's GPU-facing modules are imported inside the functions that need them: ``python -m melissa_amd.train
# --gpus N`` runs this module top to bottom in the LAUNCHER PARENT, which must stay GPU-free (melissa_amd/launch.py) - it
# parses its arguments, starts the ranks and never gets as far as ``train()``.


MODELS = ("l_dgn", "hl_dgn", "dgn_r", "n_dgn_r", "l_n_dgn_r", "hl_n_dgn_r")       # the reference's args.algorithm names
# N-DGN (policies/n_dgn.py): n_dgn_r.py / l_n_dgn_r.py / hl_n_dgn_r.py train DGN-R / L-DGN / HL-DGN networks with it
N_DGN_NETWORK = {"n_dgn_r": "dgn_r", "l_n_dgn_r": "l_dgn", "hl_n_dgn_r": "hl_dgn"}


AGGREGATORS = ("max", "mean", "add")                           # hl_dgn.py:56-60


def check_network_args(name: str, hidden_emb=128, num_heads=4, dueling_q_hidden_sizes=(128, 128),
                       dueling_v_hidden_sizes=(128, 128), aggregator_function="max", feature_dtype=None) -> None:
    """ValueError, with the reason, for a network shape the HIP path does not run (:func:`melissa_amd.shapes.hip_shape_supported`
    and the dueling heads' rule of ``validate()``, csrc/fwd.hip) - before anything is built, not at the first forward.  No torch."""
    from .shapes import MAX_HEAD_LAYERS, require_hip_shape
    require_hip_shape(hidden_emb, num_heads)
    q, v = list(dueling_q_hidden_sizes), list(dueling_v_hidden_sizes)
    for flag, sizes in (("dueling_q_hidden_sizes", q), ("dueling_v_hidden_sizes", v)):
        if any(int(x) < 64 or int(x) % 64 for x in sizes):
            raise ValueError(f"{flag}={sizes}: every hidden layer of a dueling head must be a multiple of 64 wide")
    if len(q) != len(v) or len(q) + 1 > MAX_HEAD_LAYERS:
        raise ValueError(f"dueling_q_hidden_sizes={q} and dueling_v_hidden_sizes={v}: the Q and V heads must have the same depth, "
                         f"at most {MAX_HEAD_LAYERS - 1} hidden layers")
    if feature_dtype == "bf16" and not q:
        # (the bf16 feature path's last head layer reads fp32 rows that only a hidden layer writes)
        raise ValueError("feature dtype bf16 needs at least one hidden layer in the dueling heads: "
                         "dueling_q_hidden_sizes / dueling_v_hidden_sizes are empty")
    if aggregator_function not in AGGREGATORS:
        raise ValueError(f"aggregator_function={aggregator_function!r}: one of {AGGREGATORS}")
    if aggregator_function != "max" and N_DGN_NETWORK.get(name, name) != "hl_dgn":
        raise ValueError(f"aggregator_function={aggregator_function!r} is for the HL-DGN models (hl_dgn, hl_n_dgn_r): "
                         f"{name} has no graph pool")


def build_network(name: str, n_nodes: int, device, hidden=128, heads=4, dueling_q_hidden_sizes=(128, 128),
                  dueling_v_hidden_sizes=(128, 128), aggregator="max"):
    """The reference's network of a model name at its ``--hidden-emb`` / ``--num-heads`` / ``--dueling-*-hidden-sizes`` /
    ``--aggregator-function`` (common.py:29-30,41-43; the defaults are the reference's)."""
    from .networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    duel = ({"hidden_sizes": [int(x) for x in dueling_q_hidden_sizes]},
            {"hidden_sizes": [int(x) for x in dueling_v_hidden_sizes]})          # common.py:41-42
    name = N_DGN_NETWORK.get(name, name)
    if name == "l_dgn":
        return LDGNNetwork(5, hidden, 2, heads, n_nodes, dueling_param=duel, device=device)
    if name == "hl_dgn":
        return HLDGNNetwork(5, hidden, 2, heads, n_nodes, aggregator=aggregator, dueling_param=duel, device=device)
    if name == "dgn_r":
        return DGNRNetwork(5, hidden, 2, heads, n_nodes, dueling_param=duel, device=device)
    raise ValueError(name)


def load_policy_weights(policy, path, device) -> None:
    """``policy.load_state_dict`` of a saved policy (keys ``model.*`` / ``model_old.*``).  A checkpoint trained at another
    ``--hidden-emb`` / ``--num-heads`` / dueling shape fails HERE, naming the first mismatching key and both shapes."""
    import torch
    sd = torch.load(path, map_location=device, weights_only=True)
    own = policy.state_dict()
    for key, value in sd.items():
        if key in own and tuple(own[key].shape) != tuple(value.shape):
            raise ValueError(f"{path} was trained at another network shape: {key} is {tuple(value.shape)} in the checkpoint and "
                             f"{tuple(own[key].shape)} in the network built here (--hidden-emb / --num-heads / "
                             f"--dueling-q-hidden-sizes / --dueling-v-hidden-sizes must be the training run's)")
    policy.load_state_dict(sd)


def policy_and_learner(name: str):
    """(policy class, learner class, replay records neighbours) of a model name: dgn_r.py trains with DGNPolicy (summed sibling
    Q, policies/dgn.py), the three N scripts with N-DGN (policies/n_dgn.py, siblings restricted to the one-hop neighbours),
    l_dgn.py / hl_dgn.py with DQNPolicy."""
    from .policy import DGNPolicy, DQNPolicy, NDGNPolicy
    from .replay import DGNLearner, DQNLearner, NDGNLearner
    if name not in MODELS:
        raise ValueError(name)
    if name in N_DGN_NETWORK:
        return NDGNPolicy, NDGNLearner, True
    if name == "dgn_r":
        return DGNPolicy, DGNLearner, False
    return DQNPolicy, DQNLearner, False


def default_model_name() -> str:
    """common.py:54: the reference names a run after the time it starts."""
    return datetime.datetime.now().strftime("%y%m%d-%H%M%S")


def _param_checksum(net) -> float:
    import torch
    return float(torch.cat([p.detach().flatten() for p in net.parameters()]).double().sum())


def _evaluate(policy, n_nodes, test_num, eps_test, seed, device, heuristic, scripted_agents_ratio) -> dict:
    """``test_num`` episodes of the evaluation schedule at ``eps_test`` with the training policy's network (``test_fn`` +
    ``episode_per_test``, l_dgn.py:240-253), on an env built as :func:`melissa_amd.watch.watch` builds it.  ONE env, like the
    reference's ``test_envs``: every env of a batch walks the same list of test seeds, more envs would repeat episodes.  The
    env is built anew for every evaluation, so each one plays the same ``test_num`` episodes from the top of that list.
    -> rew / len / the ``logger_stats`` means over those episodes."""
    import numpy as np
    from . import _lib
    from .collect import Collector
    from .env import HipGraphVectorEnv, connected_graph_pool
    venv = HipGraphVectorEnv(1, n_nodes, graph_pool=connected_graph_pool(n_nodes, 16, first_seed=0, device=device), dynamic_graph=True,
                             device=device, max_moves=64, seed=seed, construct_like_reference=False, is_testing=True,
                             num_test_episodes=test_num, scripted_agents_ratio=scripted_agents_ratio, heuristic=heuristic)
    col = Collector(policy, venv, episodes_per_env=test_num + 2, seed=seed, eps=eps_test, chunk=4, use_graph=False)
    was_training = policy.model.training
    policy.model.eval()                                        # (as watch() and [3P] test_episode do; back to train mode after)
    try:
        res = col.collect(n_episode=test_num)
    finally:
        policy.model.train(was_training)
    # (the last chunk of rounds may finish an episode more than asked for: the first test_num count)
    out = dict(rew=float(np.mean(res.returns[:test_num])), len=float(np.mean(res.lens[:test_num])), episodes=int(test_num),
               rew_std=float(np.std(res.returns[:test_num])))
    out.update({k: float(np.mean(res.episode_info[k][:test_num])) for k in _lib.LOGGER_KEYS})
    return out


def _evaluate_spread(policy, n_nodes, test_num, test_envs, eps_test, seed, device, heuristic, scripted_agents_ratio) -> dict:
    """The same ``test_num`` episodes as :func:`_evaluate` - same env settings, same list of test seeds, same graph pool - played
    by ``test_envs`` envs at once: env b takes list positions ``b, b + test_envs, ...``, the schedule is drawn on the device and
    the rounds replay from a HIP graph (:func:`melissa_amd.collect.evaluate_spread`).  Means are taken in list-position order.
    With ``eps_test`` 0 the episodes are the ones :func:`_evaluate` plays; with exploration the random draws differ (they are
    indexed by env and round)."""
    import numpy as np
    from . import _lib
    from .collect import evaluate_spread
    from .env import HipGraphVectorEnv, connected_graph_pool
    venv = HipGraphVectorEnv(test_envs, n_nodes, graph_pool=connected_graph_pool(n_nodes, 16, first_seed=0, device=device), dynamic_graph=True,
                             device=device, max_moves=64, seed=seed, construct_like_reference=False, is_testing=True,
                             num_test_episodes=test_num, scripted_agents_ratio=scripted_agents_ratio, heuristic=heuristic,
                             spread_test_episodes=True)
    was_training = policy.model.training
    policy.model.eval()
    try:
        res, _positions = evaluate_spread(policy, venv, test_num, eps=eps_test, seed=seed)
    finally:
        policy.model.train(was_training)
    out = dict(rew=float(np.mean(res.returns)), len=float(np.mean(res.lens)), episodes=int(test_num),
               rew_std=float(np.std(res.returns)))
    out.update({k: float(np.mean(res.episode_info[k])) for k in _lib.LOGGER_KEYS})
    return out


def _agreed_decisions(loop, world, device) -> int:
    """The decision count every rank uses for the run's env steps: the smallest rank's (a host read: synchronises)."""
    from . import parallel
    own = loop.counters()["decisions"]
    return own if world == 1 else -int(parallel.all_reduce_max(-float(own), device))


class _StaleDecisionCount:
    """The agreed decision count as it stood one update iteration ago: ``push`` enqueues a snapshot of the device counters
    (``RoundLoop.snapshot_counters``), their sum and its copy into pinned host memory, and hands back the count of the PREVIOUS
    push, whose copy has long been done - one host read per iteration that waits for nothing still queued, so the launch queue
    never drains.  With several ranks the smallest rank's count is what every rank gets (a device all-reduce in the same queue),
    the same number :func:`_agreed_decisions` gives: compared with a target derived from that number too, every rank ends an
    epoch at the same iteration - it must, because the gradient all-reduce pairs the ranks' updates one to one."""

    def __init__(self, loop, world):
        import torch
        self.loop, self.world = loop, world
        self.host = [torch.zeros(1, dtype=torch.int64).pin_memory() for _ in range(2)]
        self.done = [torch.cuda.Event(), torch.cuda.Event()]
        self.pushed = 0

    def push(self):
        import torch
        import torch.distributed as dist
        from . import _lib
        scalars, _ = self.loop.snapshot_counters()
        count = scalars[:, _lib.S_DECISIONS].sum(dtype=torch.int64).reshape(1)
        if self.world > 1:
            if dist.get_backend() == "gloo":                   # (host tensors: the rehearsal backend synchronises)
                h = count.cpu()
                dist.all_reduce(h, op=dist.ReduceOp.MIN)
                count = h.to(count.device)
            else:
                dist.all_reduce(count, op=dist.ReduceOp.MIN)
        k = self.pushed & 1
        self.pushed += 1
        previous = None
        if self.pushed > 1:
            self.done[k ^ 1].synchronize()
            previous = int(self.host[k ^ 1][0])
        self.host[k].copy_(count, non_blocking=True)
        self.done[k].record()
        return previous


def updates_owed(env_step: int, base: int, done: int, update_per_step: float) -> int:
    """Updates to run now, ``env_step`` env steps into a run that counts from ``base`` and has taken ``done`` updates: what brings
    the total to ``floor(update_per_step * (env_step - base))``, never less than 0 (a count that has not moved past the updates
    already taken owes nothing).

    The reference's trainer ([3P] tianshou ``OffpolicyTrainer.policy_update_fn``) takes ``round(update_per_step * n_collected)``
    updates after every collect, rounding collect by collect.  This rule is the cumulative floor instead: the two agree where
    ``update_per_step * step_per_collect`` is a whole number (the reference's defaults, 0.1 * 10 = one update per collect), and
    for every other value the cumulative form neither drifts away from ``update_per_step`` updates per env step nor depends on how
    the run is cut into collects - summed over any split of a run into iterations it ends at the same total."""
    return max(0, int(math.floor(update_per_step * (env_step - base))) - int(done))


def rounds_per_collect(step_per_collect: int, envs: int, world: int = 1) -> int:
    """``--step-per-collect`` in rounds: a round steps every env of every rank, so ``ceil(S / (envs * world))`` of them, at least
    one, collect ``S`` env steps (a static number: the rounds of an iteration still replay from one HIP graph)."""
    return max(1, -(-int(step_per_collect) // (int(envs) * int(world))))


def replay_rounds_for(buffer_size: int, envs: int, n_nodes: int) -> int:
    """``--buffer-size`` in rounds per env.  The reference splits its buffer into one sub-buffer per (env, agent) of
    ``buffer_size / (envs * n_nodes)`` transitions (125 at its defaults: 100 000 / (40 * 20)); an agent acts at most once per
    round, so a ring of that many rounds holds at least that many of its transitions.  Never below 8 (the pre-fill)."""
    return max(8, -(-int(buffer_size) // (int(envs) * int(n_nodes))))


def _run_epochs(loop, policy, iteration, evaluate, before_first_epoch, epoch, step_per_epoch, rank, world, device, best_path,
                last_path, pace=None, pooled=None, state_io=None, train_log=None, log_file=None):
    """The reference's training structure ([3P] tianshou ``OffpolicyTrainer`` as l_dgn.py:246-261 configures it): evaluate, then
    ``epoch`` times [update iterations until ``step_per_epoch`` more env steps are collected; evaluate; keep the best policy], then
    save the last one.  env steps = decisions x ``world``, the decisions being this rank's - with several ranks the smallest
    rank's, a number all of them hold (:func:`_agreed_decisions`), so that targets and counts, and with them the number of updates
    of every epoch, are the same everywhere.  The end of an epoch is noticed from a count that is one iteration old
    (:class:`_StaleDecisionCount`), so an epoch runs one iteration past its target: ``overshoot`` env steps.
    ``before_first_epoch()`` runs after the first evaluation (the update's capture, whose warm-up updates that evaluation and
    the first ``_best.pth`` must not see).  Rank 0 evaluates and writes; the others wait at the barrier; every rank keeps the
    epochs' counters.  -> (losses [first, last], training seconds, updates, result)

    ``pace`` = (collect, update, update_per_step) switches to updates paced by env steps (``--update-per-step``): an iteration is
    ``collect()`` followed by as many ``update(index)`` as the stale count owes (:func:`updates_owed`, counted from the first
    evaluation's env step; 0 or many), and at the end of an epoch the count read with a synchronise settles the rest before
    the evaluation - ``updates_done == floor(update_per_step * (env_step - base))`` at every epoch boundary.  Every rank
    derives the number from the same agreed count, so all take the same updates.  The target-network sync keeps counting
    updates.  Epoch records then also carry ``update_debt`` (0).
    ``pooled()`` (``--collect-stats steps``): the means of the ``logger_stats`` of every env step this rank's training envs played
    since the last call; every epoch record carries them (``train_info_rows``, ``train_<key>``).
    ``state_io`` = (write, restore, stop_after), each optional (:mod:`melissa_amd.train_state`): ``write(numbers)`` is called with
    this function's own numbers and records after every epoch's evaluation - after ``before_first_epoch()`` for epoch 0, so
    that every state holds a captured update's two warm-up updates; ``restore()`` replaces the first evaluation: the update is
    captured where a fresh run captures it, then ``restore()`` overwrites everything and hands back the numbers a ``write`` was
    given, and the loop goes on with the epoch after ``state_epoch``; ``stop_after``: the last epoch this process runs.
    ``train_log`` (:class:`melissa_amd.train_log.TrainLog`) / ``log_file``: the log is armed with ``base`` after the first
    evaluation and the update's capture (warm-up updates are not logged), drained after every epoch's evaluation and before
    ``write`` - the last epoch of the run with its open interval -, and rank 0 appends the drained rows and one ``test/*`` row
    per epoch to ``log_file``; the result then carries ``log_file`` and ``log_rows``."""
    import torch
    from . import parallel
    from .train_log import append_rows
    log_rows, test_std = 0, [None]

    def log_epoch(index, final=False):
        """Drain (every rank: the ring must not fill) and, on rank 0, append the rows and the epoch's evaluation."""
        nonlocal log_rows
        if train_log is None:
            return
        rows = [dict(r, ranks_pooled=1) for r in train_log.drain(final=final)]
        if rank == 0:
            rec = epochs[-1]
            rows.append({"env_step": rec["env_step"], "epoch": index, "test/reward": rec.get("test_rew"),
                         "test/reward_std": test_std[0], "test/length": rec.get("test_len")})
            log_rows += append_rows(log_file, rows)
    write, restore, stop_after = state_io if state_io is not None else (None, None, None)
    if rank == 0:
        os.makedirs(os.path.dirname(best_path), exist_ok=True)
    epochs, best = [], None

    def numbers(index):
        return dict(state_epoch=index, env_step=env_step, base=base, updates=updates, iterations=iterations, seconds=seconds,
                    epochs=epochs, best_epoch=None if best is None else best[0], best_rew=None if best is None else best[1],
                    loss_first=None if first is None else float(first), loss_last=None if last is None else float(last))

    def test(index, env_step, **more):
        nonlocal best
        rec = dict(epoch=index, env_step=env_step, eps=loop.eps_now()[1], **more)
        if pooled is not None:
            rec.update(pooled())
        stats = evaluate()
        if rank == 0:
            is_best = best is None or stats["rew"] > best[1]   # (the first evaluation sets the best: [3P] BaseTrainer.reset)
            if is_best:
                best = (index, stats["rew"])
                torch.save(policy.state_dict(), best_path)     # save_best_fn, l_dgn.py:215-222
            rec.update(test_rew=stats["rew"], test_len=stats["len"], best=is_best)
            # (rew_std goes to the training log's test row only: the epoch records keep the keys they have always had)
            test_std[0] = stats.get("rew_std")
            rec.update({k: v for k, v in stats.items() if k not in ("rew", "len", "rew_std")})
        epochs.append(rec)
        parallel.barrier()

    first = last = None
    updates, seconds, iterations, start = 0, 0.0, 0, 1
    if restore is None:
        env_step = base = _agreed_decisions(loop, world, device) * world
        test(0, env_step, overshoot=0, updates=0, seconds=0.0, **({} if pace is None else {"update_debt": 0}))
        before_first_epoch()
        if train_log is not None:
            train_log.arm(base)
            log_epoch(0)
        if write is not None:
            write(numbers(0))
    else:
        before_first_epoch()
        run = restore()
        env_step, base, updates, iterations, seconds = (run[k] for k in ("env_step", "base", "updates", "iterations", "seconds"))
        first, last, start = run["loss_first"], run["loss_last"], int(run["state_epoch"]) + 1
        epochs.extend(run["epochs"])
        best = None if run["best_epoch"] is None else (run["best_epoch"], run["best_rew"])
    # (a resumed run's counter starts empty like the fresh run's: its first push hands back nothing, where the straight
    # run's first push of an epoch hands back the count the previous epoch ended on - below the target and already settled)
    stale = _StaleDecisionCount(loop, world)
    for e in range(start, epoch + 1):
        target = env_step + step_per_epoch
        n, t0, more = 0, time.perf_counter(), {}
        if pace is None:
            while True:
                last = iteration(updates + n)
                first = last if first is None else first
                n += 1
                seen = stale.push()
                if seen is not None and seen * world >= target:
                    break
            env_step = _agreed_decisions(loop, world, device) * world     # (synchronises: the epoch is over)
        else:
            collect, update, update_per_step = pace

            def settle(count):
                nonlocal n, first, last
                for _ in range(updates_owed(count, base, updates + n, update_per_step)):
                    last = update(updates + n)
                    first = last if first is None else first
                    n += 1

            while True:
                collect()
                iterations += 1
                seen = stale.push()
                if seen is not None:
                    settle(seen * world)
                    if seen * world >= target:
                        break
            env_step = _agreed_decisions(loop, world, device) * world     # (synchronises: the epoch is over)
            settle(env_step)
            more["update_debt"] = int(math.floor(update_per_step * (env_step - base))) - (updates + n)
        dt = time.perf_counter() - t0
        updates, seconds = updates + n, seconds + dt
        test(e, env_step, overshoot=env_step - target, updates=n, seconds=dt, **more)
        log_epoch(e, final=e == epoch)
        if write is not None:
            write(numbers(e))
        if stop_after is not None and e >= stop_after:
            break
    if rank == 0:
        torch.save(policy.state_dict(), last_path)             # l_dgn.py:263-266
    parallel.barrier()
    best = best if best is not None else (None, None)
    result = dict(epochs=epochs, best_epoch=best[0], best_rew=best[1], best_path=best_path, last_path=last_path)
    if pace is not None:
        result["env_steps_per_iteration"] = (env_step - base) / max(1, iterations)
    if train_log is not None:
        result.update(log_file=log_file, log_rows=log_rows)
    return [first, last], seconds, updates, result


def train(model="hl_dgn", n_nodes=20, envs=256, updates=20, rounds_per_update=4, batch_size=32, n_step=4,
          gamma=0.99, lr=1e-3, target_update_freq=500, eps=0.1, replay_rounds=64, seed=9, backend=None, log=print,
          probe=None, graphs=16, ring=16, capture_updates=None, prio_buffer=False, alpha=0.6, beta=0.4,
          heuristic=None, scripted_agents_ratio=0.0, epoch=None, step_per_epoch=100000, eps_train=1.0, eps_train_final=0.05,
          exploration_fraction=0.6, eps_test=0.001, test_num=100, logdir="log", model_name=None, resume_path=None,
          update_per_step=None, step_per_collect=10, buffer_size=None, test_envs=1, collect_stats="episodes", graph_pool=None,
          hidden_emb=128, num_heads=4, dueling_q_hidden_sizes=(128, 128), dueling_v_hidden_sizes=(128, 128),
          aggregator_function="max", save_state=False, stop_after_epoch=None, resume_state=None, log_interval=None,
          log_file=None):
    """``probe(update_index, net, learner, phase)`` (optional) is called with phase "before" / "after" around every
    update - tests use it to re-derive an update's loss from the sampled batch with the oracle.
    ``graphs``: size of the synthetic training-graph dataset (the reference trains on 50 000 graphs per size, README.md:92-93;
    pools >= 4096 go through the on-disk packed cache, ``melissa_amd.env.cached_graph_pool``); the graphs are drawn by the
    device generator (``melissa_amd.env.device_graph_pool``), the same ones the host loop ``synthetic_graph_pool`` finds.
    ``graph_pool``: a packed ``.npz`` file (``save_graph_pool``, ``python -m melissa_amd.env.episodes``) that is the training
    pool instead; ``graphs`` is then not used.  Episodes come from the
    device episode stream: every reset draws a new (graph, source, interested set, movement seed) like World.reset.
    ``capture_updates``: replay the update from HIP graphs (``DQNLearner.capture``; DGN-R and N-DGN too: their dense sibling forms
    have static shapes, replay.DGNLearner / replay.NDGNLearner).  None = on unless a probe is attached; with several ranks the collective stays
    eager between two graphs.  The capture takes two extra (real, untimed) updates first: ``warmup_updates`` in the result.
    ``prio_buffer`` / ``alpha`` / ``beta``: the reference's ``--prio-buffer --alpha --beta`` (common.py:52,64-65): sample from a
    :class:`melissa_amd.replay.PrioritizedRoundReplay` (each rank owns its buffer; nothing more is exchanged).
    ``heuristic`` / ``scripted_agents_ratio``: the reference's ``--heuristic --scripted-agents-ratio`` (common.py:67,69; every
    training script hands them to its training envs, l_dgn.py:137-146): that fraction of the nodes, drawn anew on every reset
    by the device episode stream (core.py:197-217,395), runs the heuristic instead of the policy and is never recorded.
    ``epoch``: None (the default) runs ``updates`` updates at the constant ``eps`` - the fixed-updates mode.  A number runs the
    reference's training structure instead (``OffpolicyTrainer`` as l_dgn.py:246-261 configures it; see :func:`_run_epochs`):
    ``epoch`` epochs of ``step_per_epoch`` env steps, eps decaying on the device from ``eps_train`` to ``eps_train_final`` over
    ``exploration_fraction`` of the run, ``test_num`` evaluation episodes at ``eps_test`` before the first epoch and after every
    epoch, ``<logdir>/<model>/weights/<model_name>_best.pth`` / ``_last.pth`` checkpoints (``policy.state_dict()``).
    ``resume_path``: start from the weights of such a file (weights only, as the reference's ``--resume-path``).
    ``update_per_step`` (epoch mode only, else ValueError): pace the updates by the env steps collected, the reference's
    ``--update-per-step`` (common.py:35; 0.1 there: one update per 10 env steps) - after every iteration as many updates as
    :func:`updates_owed` says, the rest settled at each epoch's end (:func:`_run_epochs`); the TD target and the TD loss of these
    updates are one HIP launch each (``fused_td``, :mod:`melissa_amd.td`).  An iteration then collects ``step_per_collect`` env
    steps (``--step-per-collect``, common.py:34: :func:`rounds_per_collect` rounds instead of ``rounds_per_update``).
    ``buffer_size``: the reference's ``--buffer-size`` (transitions in all; :func:`replay_rounds_for` rounds per env instead of
    ``replay_rounds``).
    ``test_envs`` (epoch mode): 1 evaluates with one env, a host-drawn episode table and eager rounds; more evaluates with
    ``min(test_envs, test_num)`` envs that share one pass over the list of test seeds, drawn on the device and replayed from a
    HIP graph (:func:`_evaluate_spread`).  The epoch records carry the number used as ``test_envs``.
    ``collect_stats``: "steps" pools the ``logger_stats`` of every env step the training envs play on the device, as the
    reference's training collects do (multi_agent_collector.py:276,316-322; ``HipGraphVectorEnv.enable_step_stats``), and
    reports their means (``train_info_rows``, ``train_<key>``: per epoch record, or over the whole run in the fixed-updates
    mode; each rank pools its own envs, rank 0 reports).  An epoch record is written before that epoch's evaluation and its
    pool is read and emptied there, so it holds the training rounds since the previous record and never an evaluation's (those
    run on envs of their own); the record of epoch 0 holds the pre-fill rounds.  "episodes" (the default) pools nothing.
    ``hidden_emb`` / ``num_heads`` / ``dueling_q_hidden_sizes`` / ``dueling_v_hidden_sizes`` / ``aggregator_function``: the
    reference's network flags (common.py:29-30,41-43) with its defaults; a shape the HIP path does not run is a ValueError with
    the reason before anything is built (:func:`check_network_args`); a run at another shape than the default 128 x 4 records
    ``hidden_emb`` and ``num_heads`` in its result.
    ``save_state`` / ``stop_after_epoch`` / ``resume_state`` (epoch mode; :mod:`melissa_amd.train_state`, NOTES.md "Resuming a
    run"): ``save_state`` writes this rank's FULL training state after every epoch's evaluation to
    ``<logdir>/<model>/weights/<model_name>_state.pth`` (``_state.rank<r>.pth`` with several ranks; the result carries
    ``state_path``); ``stop_after_epoch=K`` ends the process after epoch K of the ``epoch`` the run has in all (``epoch`` stays
    the total: the eps horizon depends on it); ``resume_state=FILE`` continues the run that wrote FILE from the epoch after
    the one it holds, bit for bit what the uninterrupted run computes.  The file's header must be this call's: a ValueError
    names the first argument that differs, before anything is built.
    ``log_interval`` / ``log_file`` (epoch mode, else ValueError; :mod:`melissa_amd.train_log`, NOTES.md "Training curves"): sum
    the training curve on the device per ``log_interval`` env steps (the reference's loggers use 1000) - episodes, returns,
    lengths, eps, loss, TD error, gradient norm - and append it after every epoch, with the epoch's evaluation, to ``log_file``
    (default ``<logdir>/<model>/<model_name>_progress.jsonl``), one JSON object per line; a resumed run appends to the file.  Each
    rank sums its own envs, rank 0 writes its rows (``"ranks_pooled": 1``).  The result gains ``log_file`` and ``log_rows``.
    Without ``log_interval`` no launch is added and no buffer allocated."""
    from . import train_state
    from .train_log import check_log_args
    train_state.check_resume_args(epoch, save_state, stop_after_epoch, resume_state, resume_path)
    check_log_args(epoch, log_interval, log_file)
    check_network_args(model, hidden_emb, num_heads, dueling_q_hidden_sizes, dueling_v_hidden_sizes, aggregator_function)
    if collect_stats not in ("episodes", "steps"):
        raise ValueError(f"collect_stats={collect_stats!r}: 'episodes' or 'steps'")
    if int(test_envs) < 1:
        raise ValueError(f"test_envs={test_envs} must be >= 1")
    if update_per_step is not None:
        if epoch is None:
            raise ValueError("update_per_step paces the updates of the epoch mode: it needs epoch")
        if not (float(update_per_step) > 0 and math.isfinite(float(update_per_step))):
            raise ValueError(f"update_per_step={update_per_step} must be a positive number")
        if int(step_per_collect) < 1:
            raise ValueError(f"step_per_collect={step_per_collect} must be >= 1")
    if buffer_size is not None and int(buffer_size) < 1:
        raise ValueError(f"buffer_size={buffer_size} must be >= 1")
    import torch
    from . import launch, parallel
    from .collect import EpsSchedule, RoundLoop
    from .env import HipGraphVectorEnv, cached_graph_pool, connected_graph_pool, load_graph_pool
    from .replay import PrioritizedRoundReplay, RoundReplay
    if backend != "gloo":
        launch.check_rank_device()                             # exit 2 when LOCAL_RANK names a GPU this rank cannot see
    # a run that is to be continued bit for bit sums its bias gradients in the form a graph replay cannot disturb; every other
    # run keeps the form it has always had, and with it its weights (networks/autograd_ops.py: set_replay_safe_column_sums)
    from .networks.autograd_ops import set_replay_safe_column_sums
    set_replay_safe_column_sums(bool(save_state) or resume_state is not None)
    rank, local_rank, world = parallel.init_distributed(backend)
    device = torch.device("cuda", local_rank if backend != "gloo" else 0)
    torch.cuda.set_device(device)
    paced = update_per_step is not None
    if buffer_size is not None:
        replay_rounds = replay_rounds_for(buffer_size, envs, n_nodes)
    if paced:
        rounds_per_update = rounds_per_collect(step_per_collect, envs, world)
    if capture_updates is None:
        # on by default, with any number of ranks: the collective stays EAGER between two graphs (pack | all-reduce | unpack +
        # step), so RCCL never enters a capture; rehearsed with two ranks on one GPU (tests/test_gpu_round.py)
        capture_updates = probe is None
    captured = bool(capture_updates) and device.type == "cuda"
    header = saved = None
    if save_state or resume_state is not None:
        from . import _lib
        header = train_state.state_header(
            model=model, n_nodes=n_nodes, envs=envs, world=world, rank=rank, hidden_emb=hidden_emb, num_heads=num_heads,
            dueling_q_hidden_sizes=dueling_q_hidden_sizes, dueling_v_hidden_sizes=dueling_v_hidden_sizes,
            aggregator_function=aggregator_function, batch_size=batch_size, n_step=n_step, gamma=gamma, lr=lr,
            target_update_freq=target_update_freq, prio_buffer=bool(prio_buffer), alpha=alpha, beta=beta, heuristic=heuristic,
            scripted_agents_ratio=scripted_agents_ratio, epoch=int(epoch), step_per_epoch=int(step_per_epoch),
            eps_train=eps_train, eps_train_final=eps_train_final, exploration_fraction=exploration_fraction,
            update_per_step=None if update_per_step is None else float(update_per_step), step_per_collect=int(step_per_collect),
            replay_rounds=int(replay_rounds), rounds_per_update=int(rounds_per_update), ring=int(ring), seed=int(seed),
            captured=captured, collect_stats=collect_stats, mel_version=_lib.load().mel_version().decode(),
            **({} if log_interval is None else {"log_interval": int(log_interval)}))
    if resume_state is not None:
        # the header is compared before the network, the envs or a graph exist (the file is memory-mapped: reading the header
        # reads no tensor); the training pool's identity follows as soon as there is a pool
        resume_state = train_state.rank_state_path(resume_state, rank, world)
        saved = train_state.load_state_file(resume_state)
        train_state.check_state_header(saved["config"], header, resume_state)
    torch.manual_seed(seed)                                    # same init everywhere, then broadcast anyway
    net = build_network(model, n_nodes, device, hidden=hidden_emb, heads=num_heads,
                        dueling_q_hidden_sizes=dueling_q_hidden_sizes, dueling_v_hidden_sizes=dueling_v_hidden_sizes,
                        aggregator=aggregator_function)
    parallel.broadcast_parameters(net, src=0)
    policy_cls, learner_cls, neighbours = policy_and_learner(model)
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=lr), discount_factor=gamma,
                        estimation_step=n_step, target_update_freq=target_update_freq)
    if resume_path is not None:
        # --resume-path (l_dgn.py:311 load_policy): the weights of a saved policy, model.* and model_old.*, nothing else
        load_policy_weights(policy, resume_path, device)
        parallel.broadcast_parameters(net, src=0)
    checksum_start = _param_checksum(net) if epoch is not None else None      # (what the first update starts from)
    if graph_pool is not None:
        graph_list = load_graph_pool(graph_pool)
        if len(graph_list) < 1 or graph_list[0].pos.shape[0] != n_nodes:
            raise ValueError(f"graph_pool={graph_pool!r} holds {len(graph_list)} graphs of "
                             f"{graph_list[0].pos.shape[0] if graph_list else 0} nodes, not of {n_nodes}")
    elif graphs >= 4096:
        graph_list = cached_graph_pool(n_nodes, graphs, 0, device=device)
    else:
        graph_list = connected_graph_pool(n_nodes, graphs, first_seed=0, device=device)
    if header is not None:
        header.update(train_state.pool_identity(graph_list))
        if saved is not None:
            train_state.check_state_header(saved["config"], header, resume_state)
    venv = HipGraphVectorEnv(envs, n_nodes, graph_pool=graph_list, dynamic_graph=True, device=device, max_moves=48,
                             seed=1000 + rank * envs, construct_like_reference=False, heuristic=heuristic,
                             scripted_agents_ratio=scripted_agents_ratio)
    pooled = None
    if collect_stats == "steps":
        venv.enable_step_stats()                               # before the loop is built: every captured round pools

        def pooled():
            count, stats = venv.read_step_stats(reset=True)
            return dict(train_info_rows=count, **{f"train_{k}": v.mean for k, v in stats.items()})
    train_log = None
    if log_interval is not None:
        # before the loop is built: every captured round holds the episode log's pointers.  The ring holds an epoch's intervals
        # and what the loop may run past its target (the end of an epoch is noticed an iteration late: two iterations' decisions)
        from .train_log import TrainLog, ring_capacity
        overshoot = 2 * max(1, rounds_per_update) * envs * n_nodes * world
        train_log = TrainLog(venv, int(log_interval), ring_capacity(step_per_epoch, log_interval, overshoot), scale=world,
                             device=device)
    if prio_buffer:
        replay = PrioritizedRoundReplay(envs, n_nodes, replay_rounds, device, neighbours=neighbours, alpha=alpha, beta=beta)
    else:
        replay = RoundReplay(envs, n_nodes, replay_rounds, device, neighbours=neighbours)
    # the rounds between two updates replay from one HIP graph (bit-identical to the eager launches: tests/test_gpu_round.py)
    schedule = None
    if epoch is not None:
        # training rounds take eps from the device schedule; every rank collects as much again, so a decision here is `world`
        # env steps of the run
        schedule = EpsSchedule(eps_train=eps_train, eps_final=eps_train_final, exploration_fraction=exploration_fraction,
                               epoch=int(epoch), step_per_epoch=int(step_per_epoch), scale=world)
    loop = RoundLoop(venv, policy, seed=1000 + rank * envs, eps=eps, replay=replay, ring=ring,
                     use_graph=device.type == "cuda" and probe is None, graph_rounds=max(1, rounds_per_update),
                     eps_schedule=schedule, **({} if train_log is None else {"train_log": train_log}))
    learner = learner_cls(policy, replay, batch_size=batch_size, n_step=n_step, gamma=gamma,
                         grad_hook=parallel.FlatGradAllReducer(net), seed=seed + rank, **({"fused_td": True} if paced else {}),
                         **({} if train_log is None else {"train_log": train_log}))
    with torch.no_grad():
        loop.run(max(n_step + 1, 8))                           # pre-fill (l_dgn.py:201)
    warmup_updates = 2 if captured else 0

    def capture():
        if captured:
            learner.capture()                                  # (two warm-up updates, then the graphs)

    if epoch is None:
        capture()
    def collect():
        with torch.no_grad():
            loop.run(rounds_per_update)

    def update(index):
        """One update; -> its loss (a device tensor when the update is replayed from graphs)"""
        if probe is not None:
            probe(index, net, learner, "before")
        loss = learner.step()["loss"]
        if probe is not None:
            probe(index, net, learner, "after")
        return loss

    def iteration(index):
        """``rounds_per_update`` rounds, then one update; -> its loss"""
        collect()
        return update(index)

    extra = {}
    if epoch is None:
        t0 = time.perf_counter()
        losses = [iteration(i) for i in range(updates)]
        torch.cuda.synchronize(device)
        dt = time.perf_counter() - t0
    else:
        n_test_envs = min(int(test_envs), int(test_num))

        def evaluate():
            if rank != 0:
                return None
            if n_test_envs > 1:
                stats = _evaluate_spread(policy, n_nodes, test_num, n_test_envs, eps_test, seed, device, heuristic,
                                         scripted_agents_ratio)
            else:
                stats = _evaluate(policy, n_nodes, test_num, eps_test, seed, device, heuristic, scripted_agents_ratio)
            stats["test_envs"] = n_test_envs
            return stats
        weights_dir = os.path.join(logdir, model, "weights")
        name = model_name if model_name is not None else default_model_name()
        if train_log is not None and log_file is None:
            from .train_log import default_log_file
            log_file = default_log_file(logdir, model, name)
        # (epoch mode captures the update AFTER the first evaluation: `param_checksum_start`, that evaluation and the first
        # _best.pth are all of the policy no update has touched)
        state_path = train_state.rank_state_path(os.path.join(weights_dir, f"{name}_state.pth"), rank, world)

        def write_state(numbers):
            os.makedirs(weights_dir, exist_ok=True)
            config = dict(header, state_epoch=numbers["state_epoch"])
            numbers = dict(numbers, param_checksum_start=checksum_start)
            train_state.write_state_file(train_state.gather_state(config, numbers, policy, learner, replay, loop, venv, device,
                                                                  train_log=train_log), state_path)

        def restore_state():
            nonlocal checksum_start
            numbers = train_state.restore_state(saved, policy, learner, replay, loop, venv, device, train_log=train_log)
            checksum_start = numbers["param_checksum_start"]
            return numbers

        state_io = (write_state if save_state else None, restore_state if saved is not None else None,
                    None if stop_after_epoch is None else int(stop_after_epoch))
        losses, dt, updates, extra = _run_epochs(loop, policy, iteration, evaluate, capture, int(epoch), int(step_per_epoch), rank,
                                                 world, device, os.path.join(weights_dir, f"{name}_best.pth"),
                                                 os.path.join(weights_dir, f"{name}_last.pth"),
                                                 pace=(collect, update, float(update_per_step)) if paced else None,
                                                 pooled=pooled, state_io=state_io, train_log=train_log, log_file=log_file)
        extra["param_checksum_start"] = checksum_start
        if save_state:
            extra["state_path"] = state_path
        if paced:
            extra.update(update_per_step=float(update_per_step), rounds_per_collect=rounds_per_update,
                         replay_rounds=replay.K, fused_td=learner.fused_td)
    # (device tensors when the update is replayed from graphs; a paced run too short to owe an update has no loss)
    losses = [float(x) if x is not None else float("nan") for x in losses]
    c = loop.counters()
    checksum = _param_checksum(net)
    out = dict(rank=rank, world=world, model=model, updates=updates, seconds=dt, loss_first=losses[0],
               loss_last=losses[-1], decisions=c["decisions"], episodes=c["episodes"], errors=c["errors"],
               param_checksum=checksum, updates_from_hip_graphs=captured, prio_buffer=bool(prio_buffer),
               # the capture's warm-up updates are REAL optimizer steps taken before the timed loop (they advance the policy's
               # iteration counter and the replay sampler's generator): a run with capture on has taken `updates +
               # warmup_updates` steps, `seconds` covers `updates` of them
               warmup_updates=warmup_updates, heuristic=heuristic, scripted_agents_ratio=float(scripted_agents_ratio),
               episode_supply=loop.supply.describe())
    out.update(extra)
    if (int(hidden_emb), int(num_heads)) != (128, 4):
        # a run at another shape than the reference's default records it (the keys of a default run stay what they were)
        out.update(hidden_emb=int(hidden_emb), num_heads=int(num_heads))
    if pooled is not None and epoch is None:
        out.update(pooled())
    # replicas must be identical after averaged-gradient steps
    same = parallel.all_reduce_max(checksum, device) == parallel.all_reduce_max(-checksum, device) * -1
    out["replicas_identical"] = bool(same)
    if rank == 0:
        log(json.dumps(out))
    parallel.barrier()
    set_replay_safe_column_sums(False)
    return out


def arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="hl_dgn", choices=list(MODELS))
    ap.add_argument("--nodes", type=int, default=20)
    ap.add_argument("--envs", "--training-num", dest="envs", type=int, default=256,
                    help="envs per GPU (--training-num: the reference's name, common.py:37)")
    ap.add_argument("--updates", type=int, default=20)
    ap.add_argument("--rounds-per-update", type=int, default=4)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--backend", default=None)
    ap.add_argument("--graphs", type=int, default=16, help="training-graph dataset size (50000 = the reference's)")
    ap.add_argument("--graph-pool", default=None, metavar="FILE",
                    help="packed training-graph dataset (.npz of python -m melissa_amd.env.episodes) used instead of --graphs")
    ap.add_argument("--gpus", type=int, default=1, help="ranks to start (one per GPU) when not under torch.distributed.run")
    ap.add_argument("--capture-updates", choices=["auto", "on", "off"], default="auto",
                    help="replay the DQN update from HIP graphs (auto: on; the capture runs 2 extra untimed warm-up updates first, "
                         "reported as warmup_updates - compare on / off runs at equal total updates)")
    # the reference's names and defaults (common.py:52,64-65)
    ap.add_argument("--prio-buffer", action="store_true", default=False, help="prioritized experience replay")
    ap.add_argument("--alpha", type=float, default=0.6, help="prioritization exponent")
    ap.add_argument("--beta", type=float, default=0.4, help="importance-weight exponent")
    # the reference's names and defaults (common.py:67,69); the probabilistic heuristics are not offered
    ap.add_argument("--heuristic", default=None, choices=["simple_broadcast", "broadcast_if_any_interested", "silent", "mpr"],
                    help="heuristic the scripted agents run")
    ap.add_argument("--scripted-agents-ratio", type=float, default=0.0,
                    help="fraction of the nodes that are scripted agents, drawn anew for every episode")
    # the reference's training structure, names and defaults (common.py:20-39,46,54); --epoch absent: the fixed-updates mode
    ap.add_argument("--epoch", type=int, default=None,
                    help="train in epochs like the reference (whose default is 10): eps decay, evaluation and checkpoints; "
                         "--updates and the constant eps do not apply")
    ap.add_argument("--step-per-epoch", type=int, default=100000)
    # update pacing, the reference's names (common.py:25,34,35); --update-per-step absent: one update per iteration
    ap.add_argument("--update-per-step", type=float, default=None,
                    help="updates per collected env step (the reference: 0.1); needs --epoch; the iterations then collect "
                         "--step-per-collect env steps instead of --rounds-per-update rounds")
    ap.add_argument("--step-per-collect", type=int, default=10, help="env steps per iteration when --update-per-step is given")
    ap.add_argument("--buffer-size", type=int, default=None,
                    help="replay size in transitions (the reference: 100000); absent: 64 rounds per env")
    ap.add_argument("--eps-train", type=float, default=1.0)
    ap.add_argument("--eps-train-final", type=float, default=0.05)
    ap.add_argument("--exploration-fraction", type=float, default=0.6)
    ap.add_argument("--eps-test", type=float, default=0.001)
    ap.add_argument("--test-num", type=int, default=100)
    ap.add_argument("--test-envs", type=int, default=1,
                    help="envs of an evaluation: 1 plays the --test-num episodes one after another; more share them out, draw "
                         "them on the device and replay the rounds from a HIP graph")
    ap.add_argument("--collect-stats", choices=["episodes", "steps"], default="episodes",
                    help="steps: pool the logger_stats of every env step of the training envs on the device (the reference's "
                         "statistic) and report their means")
    ap.add_argument("--logdir", type=str, default="log")
    ap.add_argument("--model-name", type=str, default=default_model_name())
    ap.add_argument("--resume-path", type=str, default=None)
    # a run cut at epoch boundaries (needs --epoch, which stays the run's total)
    ap.add_argument("--save-state", action="store_true", default=False,
                    help="write the full training state after every epoch (<logdir>/<model>/weights/<model-name>_state.pth)")
    ap.add_argument("--stop-after-epoch", type=int, default=None, metavar="K",
                    help="end the process after epoch K of the --epoch the run has in all")
    ap.add_argument("--resume-state", type=str, default=None, metavar="FILE",
                    help="continue the run that wrote FILE (--save-state) from the epoch after the one it holds; every other "
                         "argument must be that run's")
    # the training curve (the reference's loggers write about every 1000 env steps, l_dgn.py:203-213)
    ap.add_argument("--log-interval", type=int, default=None, metavar="N",
                    help="sum the training curve on the device per N env steps (the reference: 1000) and append it, with every "
                         "epoch's evaluation, to --log-file as JSON lines; needs --epoch")
    ap.add_argument("--log-file", type=str, default=None, metavar="FILE",
                    help="default <logdir>/<model>/<model-name>_progress.jsonl; a resumed run appends")
    # the reference's network flags, names and defaults (common.py:29-30,41-43)
    ap.add_argument("--hidden-emb", type=int, default=128, help="encoder width and channels per attention head")
    ap.add_argument("--num-heads", type=int, default=4, help="attention heads (a power of two, or 6)")
    ap.add_argument("--dueling-q-hidden-sizes", type=int, nargs="*", default=[128, 128])
    ap.add_argument("--dueling-v-hidden-sizes", type=int, nargs="*", default=[128, 128])
    ap.add_argument("--aggregator-function", type=str, default="max", choices=list(AGGREGATORS),
                    help="graph pool of the HL-DGN models")
    ap.add_argument("--seed", type=int, default=9)
    ap.add_argument("--lr", type=float, default=0.001)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--n-step", type=int, default=4)
    ap.add_argument("--target-update-freq", type=int, default=500)
    return ap


def train_kwargs(a: argparse.Namespace) -> dict:
    """The keyword arguments of :func:`train` a parsed command line stands for (``epoch`` None = the fixed-updates mode)."""
    return dict(model=a.model, n_nodes=a.nodes, envs=a.envs, updates=a.updates, rounds_per_update=a.rounds_per_update,
                batch_size=a.batch_size, backend=a.backend, graphs=a.graphs,
                capture_updates={"auto": None, "on": True, "off": False}[a.capture_updates],
                prio_buffer=a.prio_buffer, alpha=a.alpha, beta=a.beta, heuristic=a.heuristic,
                scripted_agents_ratio=a.scripted_agents_ratio, epoch=a.epoch, step_per_epoch=a.step_per_epoch,
                eps_train=a.eps_train, eps_train_final=a.eps_train_final, exploration_fraction=a.exploration_fraction,
                eps_test=a.eps_test, test_num=a.test_num, logdir=a.logdir, model_name=a.model_name, resume_path=a.resume_path,
                seed=a.seed, lr=a.lr, gamma=a.gamma, n_step=a.n_step, target_update_freq=a.target_update_freq,
                update_per_step=a.update_per_step, step_per_collect=a.step_per_collect, buffer_size=a.buffer_size,
                test_envs=a.test_envs, collect_stats=a.collect_stats, graph_pool=a.graph_pool,
                hidden_emb=a.hidden_emb, num_heads=a.num_heads, dueling_q_hidden_sizes=list(a.dueling_q_hidden_sizes),
                dueling_v_hidden_sizes=list(a.dueling_v_hidden_sizes), aggregator_function=a.aggregator_function,
                save_state=a.save_state, stop_after_epoch=a.stop_after_epoch, resume_state=a.resume_state,
                log_interval=a.log_interval, log_file=a.log_file)


def parse_args(argv=None) -> argparse.Namespace:
    """The command line, with what argparse alone cannot say: ``--update-per-step`` needs ``--epoch``, and the network flags
    must name a shape the HIP path runs (an error here, with the reason, not at the first forward)."""
    ap = arg_parser()
    a = ap.parse_args(argv)
    try:
        check_network_args(a.model, a.hidden_emb, a.num_heads, a.dueling_q_hidden_sizes, a.dueling_v_hidden_sizes,
                           a.aggregator_function)
    except ValueError as e:
        ap.error(str(e))
    if a.update_per_step is not None and a.epoch is None:
        ap.error("--update-per-step paces the updates of the epoch mode: it needs --epoch")
    from . import train_state
    try:
        train_state.check_resume_args(a.epoch, a.save_state, a.stop_after_epoch, a.resume_state, a.resume_path)
    except ValueError as e:
        ap.error(str(e))
    from .train_log import check_log_args
    try:
        check_log_args(a.epoch, a.log_interval, a.log_file)
    except ValueError as e:
        ap.error(str(e))
    import sys
    given = sys.argv[1:] if argv is None else argv
    if a.graph_pool is not None and any(x == "--graphs" or x.startswith("--graphs=") for x in given):
        print(f"--graph-pool {a.graph_pool} is the training pool: --graphs {a.graphs} is ignored", file=sys.stderr)
    return a


def main(argv=None):
    a = parse_args(argv)
    import sys
    from . import launch
    given = sys.argv[1:] if argv is None else list(argv)
    rc = launch.maybe_spawn("-m", ["melissa_amd.train", *given], a.gpus, check_devices=a.backend != "gloo")
    if rc is not None:
        raise SystemExit(rc)
    from .train_state import StateMismatch
    try:
        train(**train_kwargs(a))
    except StateMismatch as e:                                 # the state file is another run's: an argument error
        arg_parser().error(str(e))


if __name__ == "__main__":
    main()
