"""The collector hot loop, device resident.

Reference: ``MultiAgentCollector.collect``'s ``while True`` loop (multi_agent_collector.py:150-308):
one iteration = policy forward over the ready envs -> eps-greedy -> ``env.step`` -> next obs, with a
host<->device round trip and O(envs) Python bookkeeping per iteration.  ``DecisionLoop`` runs the same
iteration as a fixed sequence of HIP launches on one stream with no host synchronisation:

    obs [B, 8N+1] (HBM) -> mel_{l,hl}dgn_forward -> logits -> mel_select_action -> act
        -> mel_env_step (+ last() + on-device episode reset) -> obs (same buffer)

Finished episodes are re-seeded on the device from a pre-sampled episode pool (the packed replacement
of the reference's per-reset pickle.load + RNG draws).  Replay-buffer routing
(multi_agent_collector.py:229-271) is not part of this loop.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .env.episodes import EpisodeSampler, pack_episodes
from .env.stream import make_supply
from .env.vector_env import HipGraphVectorEnv, ObsBuffers
from .record_common import check_rides


def sample_episode_table(venv: HipGraphVectorEnv, episodes_per_env: int, seed: int = 0):
    """Pre-draw ``episodes_per_env`` episodes for every env with the reference's RNG protocol (env k's
    generator seeded ``seed + k``) -> (packed pool dict, episode_table int32 [B, K])."""
    episodes, table = [], np.zeros((venv.env_num, episodes_per_env), dtype=np.int32)
    for b in range(venv.env_num):
        sampler = venv.make_sampler(seed + b, env=b)   # same evaluation schedule / scripted ratio / density as the env
        for k in range(episodes_per_env):
            table[b, k] = len(episodes)
            episodes.append(sampler.sample())
    packed = pack_episodes(episodes, venv.graphs, venv.n, venv.max_moves, venv.dynamic_graph)
    return packed, table


@dataclasses.dataclass
class EpsSchedule:
    """The exploration schedule of the reference's trainers (``train_fn``, l_dgn.py:225-234): eps decays from ``eps_train`` to
    ``eps_final`` over ``exploration_fraction`` of the ``epoch * step_per_epoch`` env steps of a run, as a function of the env
    steps collected so far.  Given to :class:`RoundLoop`, the device evaluates it before every round from the envs' own
    decision counters (``mel_exploration_schedule``); ``scale``: env steps per decision of THIS loop (the world size when every
    rank collects as much again), ``trace``: keep the (env_step, eps) of the last ``trace`` rounds in a device ring."""
    eps_train: float = 1.0
    eps_final: float = 0.05
    exploration_fraction: float = 0.6
    epoch: int = 10
    step_per_epoch: int = 100000
    scale: int = 1
    trace: int = 0

    @property
    def total_steps(self) -> int:
        return self.epoch * self.step_per_epoch

    def eps(self, env_step: int) -> float:
        return exploration_eps(env_step, self.eps_train, self.eps_final, self.exploration_fraction, self.epoch,
                               self.step_per_epoch)


def exploration_eps(env_step: int, eps_train: float = 1.0, eps_final: float = 0.05, exploration_fraction: float = 0.6,
                    epoch: int = 10, step_per_epoch: int = 100000) -> float:
    """eps after ``env_step`` collected env steps, in the reference's own arithmetic (l_dgn.py:229-233) - the host-side
    statement of what ``mel_exploration_schedule`` computes as ``eps_train * exp(env_step * ln(eps_final) / horizon)``."""
    decay_factor = 1.0 - math.pow(math.e, math.log(eps_final) / (exploration_fraction * epoch * step_per_epoch))
    return max(eps_train * (1.0 - decay_factor) ** env_step, eps_final)


def _counters_of(scalars: torch.Tensor, iterations: int) -> dict:
    sc = scalars.cpu().numpy()
    return dict(decisions=int(sc[:, _lib.S_DECISIONS].sum()), episodes=int(sc[:, _lib.S_EPISODES_DONE].sum()),
                errors=int(np.bitwise_or.reduce(sc[:, _lib.S_ERROR])), iterations=iterations)


class DecisionLoop:
    """AEC-order loop: one agent decision per env per iteration (the reference collector's granularity)."""

    def __init__(self, venv: HipGraphVectorEnv, policy, episodes_per_env: int = 8, seed: int = 0,
                 eps: float = 0.0, episodes=None, stream: bool | None = None, ring: int = 64, discard: int = 0):
        """Episodes: a device stream (fresh episodes for ever, ``melissa_amd.env.stream``) unless ``episodes`` =
        (packed, table) is given or ``stream`` is False (a host-drawn table of ``episodes_per_env`` per env)."""
        self.venv, self.policy, self.eps = venv, policy, eps
        dev = venv.device
        self.supply = make_supply(venv, seed, episodes, episodes_per_env, stream, ring, discard, reset_snapshots=False)
        self.pool, self.table = self.supply.pool, self.supply.table
        self.n_actions = policy.model.output_dim
        self.obs = torch.empty(venv.env_num, 8 * venv.n + 1, dtype=torch.float32, device=dev)
        self.out = ObsBuffers(venv.env_num, venv.n, dev, obs=self.obs)
        self.logits = torch.empty(venv.env_num, self.n_actions, dtype=torch.float32, device=dev)
        self.act = torch.empty(venv.env_num, dtype=torch.int32, device=dev)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.iterations = 0
        venv.reset_device(self.pool, self.supply.first_episode_ids(), self.out)

    def step(self):
        """One collector iteration for every env (one agent decision per env)."""
        self.supply.before_step(self.iterations)
        net = self.policy.model
        # observations written by the env kernels: integer node features (unless scripted agents relay beyond four times)
        net.hip_forward(self.obs, out=self.logits,
                        integer_features=self.venv._sampler_kw["scripted_agents_ratio"] == 0.0)
        if self.eps > 0.0:
            rand_u = torch.rand(self.venv.env_num, device=self.obs.device, generator=self.gen)
            rand_q = torch.rand(self.venv.env_num, self.n_actions, device=self.obs.device, generator=self.gen)
            self.policy.select_action(self.logits, self.out.action_mask, self.eps, rand_u, rand_q, out=self.act)
        else:
            self.policy.select_action(self.logits, self.out.action_mask, out=self.act)
        self.venv.step_device(self.pool, self.act, self.out, self.table)
        self.iterations += 1

    def run(self, iterations: int):
        for _ in range(iterations):
            self.step()

    def snapshot_counters(self):
        """Device-side copy of the per-env counters as they stand when the launches enqueued so far have run (no host
        synchronisation: the copy is one more launch in the queue); ``counters(snapshot)`` reads it later."""
        return (self.venv.scalars().clone(), self.iterations)

    def counters(self, snapshot=None) -> dict:
        """Host read of the per-env counters (synchronises)."""
        if snapshot is not None:
            return _counters_of(*snapshot)
        return _counters_of(self.venv.scalars(), self.iterations)


class RoundLoop:
    """Round-batched loop: one iteration = one whole env ROUND for every env.

    Within a round every active agent observes the same ``obs_matrix`` (graph.py:186-188: the rows differ
    only in the controlling-agent column) and no agent's action is visible to another before the world
    step (graph.py:324-347), so all of a round's decisions are taken by ONE forward
    (``mel_ldgn_forward_agents``: shared encoder / conv1 over the union of the receptive fields) and applied
    by ONE env launch (``mel_env_round``) that replays the reference's AEC order - pending dead agents first,
    then each active agent with its own action, then the world step.  Per-env trajectories are identical to
    the AEC-order loop under the same actions; an iteration yields ~N/6 decisions per env instead of one.
    """

    def __init__(self, venv: HipGraphVectorEnv, policy, episodes_per_env: int = 8, seed: int = 0,
                 eps: float = 0.0, episodes=None, rows_cap: int | None = None, use_graph: bool = False,
                 stream: "torch.cuda.Stream | None" = None, replay=None, episode_stream: "bool | str | None" = None,
                 ring: int = 16, discard: int = 0, graph_rounds: int = 4, eps_schedule: "EpsSchedule | None" = None,
                 train_log=None, recorder=None, decisions=None, attention=None):
        """Episodes: by default a device STREAM (``melissa_amd.env.stream.EpisodeStream``: every reset draws a new episode
        like World.reset does, core.py:372-394; ``ring`` slots per env, ``discard`` construction-time samplings dropped);
        ``episodes`` = (packed, table) or ``episode_stream=False`` give a fixed table of ``episodes_per_env`` episodes;
        ``episode_stream="test"`` streams the evaluation schedule of an env in testing mode from the device
        (``melissa_amd.env.stream.TestEpisodeStream``; such an env gets a host-drawn table otherwise).
        ``eps_schedule`` (:class:`EpsSchedule`): every round starts with one small launch that computes eps from the envs'
        decision counters and the selection reads that device value instead of ``eps`` - eager rounds and replayed graphs
        alike, nothing is recaptured when eps changes.
        ``train_log`` (:class:`melissa_amd.train_log.TrainLog`, built on ``venv`` BEFORE this loop): every round, eager or
        captured, and every round of a group graph is followed by ``mel_train_log_round``, which folds the episodes the round
        ended into the log's open record.  None (the default): no such launch.
        ``recorder`` (:class:`melissa_amd.round_record.RoundRecorder` on ``venv``): every round, eager or captured, is followed
        by ``mel_round_record_round``, which samples the state the round left into the recorder's per-round curves and traces;
        one more launch behind the constructor's ``first`` launch records the first episodes' round 0.  None (the default): no
        such launch, the sequence is the one without the recorder.
        ``decisions`` (:class:`melissa_amd.decision_record.DecisionRecorder` on ``venv``): every round, eager or captured, issues
        ``mel_decision_record_round`` BETWEEN the forward and ``mel_env_round`` - the only place where the round's logits, actions
        and ``live`` sets exist together - which books the policy's decisions by round index and by node degree.  It does not
        touch the episode log: with or without ``recorder`` / ``train_log``.  None (the default): no such launch.
        ``attention`` (:class:`melissa_amd.attention_record.AttentionRecorder` on ``venv`` and the policy's network, L-DGN or
        DGN-R): every round, eager or captured, issues ``mel_forward_attention`` and ``mel_attention_record_round`` right behind
        the decision recorder's place - conv2's coefficients of the round's agent rows, read back from the forward's workspace,
        booked by round index, node degree and head.  It writes nothing the loop reads.  None (the default): no such launch."""
        self.venv, self.policy, self.eps, self.seed = venv, policy, eps, seed
        check_rides("RoundLoop", "attention", attention, venv)
        self.attention = attention
        check_rides("RoundLoop", "decisions", decisions, venv)
        self.decisions = decisions
        check_rides("RoundLoop", "recorder", recorder, venv)
        if recorder is not None and train_log is not None:
            raise ValueError("RoundLoop: train_log empties the episode log every round, the recorder looks ended episodes up in "
                             "it: not both on one loop")
        self.recorder = recorder
        if train_log is not None and train_log.venv is not venv:
            raise ValueError("RoundLoop: train_log was built on another env batch")
        self.train_log = train_log
        self.use_graph, self.graph = use_graph, None
        # run(): whole groups of `graph_rounds` rounds are replayed from ONE HIP graph - a graph launch costs the device ~8 us
        # of idle time between the last kernel of one replay and the first of the next (rocprofv3 kernel trace of the
        # one-round graph: tools/gap_trace.py), a quarter of that per round with four rounds per graph
        self.graph_rounds, self.group_graph = max(1, int(graph_rounds)), None
        # the observations are the env kernels' own, so their node features are integers in known ranges and the forward may
        # evaluate encoder / conv1 projections once per feature TUPLE (MEL_FWD_INTEGER_FEATURES); False forces row lists
        # (scripted agents relay without a step budget, so their message counts leave the table's range: row lists then)
        self.integer_features = venv._sampler_kw["scripted_agents_ratio"] == 0.0
        self.stream = stream                       # None: torch's current stream
        self.replay = replay                       # optional melissa_amd.replay.RoundReplay
        dev = venv.device
        # episode ends load their next state from reset snapshots (static tables: precomputed here; streams: by the refill)
        if stream is not None:
            with torch.cuda.stream(stream):
                self.supply = make_supply(venv, seed, episodes, episodes_per_env, episode_stream, ring, discard)
        else:
            self.supply = make_supply(venv, seed, episodes, episodes_per_env, episode_stream, ring, discard)
        self.pool, self.table = self.supply.pool, self.supply.table
        self.n_actions = policy.model.output_dim
        # HL-DGN's logits do not depend on the agent (hl_dgn.py:108): one row per env, dense action layout
        self.per_env_logits = policy.model._MODEL == _lib.MODEL_HLDGN
        self.rows_cap = venv.env_num if self.per_env_logits else int(rows_cap or venv.env_num * venv.n)
        self.live = torch.zeros(venv.env_num, *(() if venv.n <= 64 else (_lib.set_words(venv.n),)), dtype=torch.int64,
                                device=dev)         # the round's active sets (node sets: [B], or [B, W] beyond 64 nodes)
        self.offsets = torch.zeros(venv.env_num + 1, dtype=torch.int32, device=dev)
        self.logits = torch.zeros(self.rows_cap, self.n_actions, dtype=torch.float32, device=dev)
        self.act = torch.zeros(venv.env_num * venv.n if self.per_env_logits else self.rows_cap, dtype=torch.int32,
                               device=dev)
        if attention is not None:
            if self.per_env_logits:
                raise ValueError("RoundLoop: attention records conv2's coefficients per agent row; an HL-DGN policy has no second "
                                 "convolution and one logits row per env")
            if attention.net is not policy.model:
                raise ValueError("RoundLoop: attention was built for another network than the policy's")
            if attention.rows_cap != self.rows_cap:
                raise ValueError(f"RoundLoop: attention was built for another rows_cap ({attention.rows_cap}), the loop's forward "
                                 f"runs with {self.rows_cap}")
        self.iterations = 0
        self._rounds_base = 0
        self.rounds = torch.zeros(1, dtype=torch.int32, device=dev)     # device-side round counter (RNG step, refill pacing)
        self._select = _lib.MelSelect()
        self._select.act, self._select.eps = self.act.data_ptr(), float(eps)
        self._select.seed, self._select.step_dev = seed & 0xFFFFFFFF, self.rounds.data_ptr()
        if self.per_env_logits:                    # every agent of live[b] draws from env b's logits row
            self._select.live, self._select.n_nodes = self.live.data_ptr(), venv.n
        self.eps_schedule = eps_schedule
        if eps_schedule is not None:
            cap = max(0, int(eps_schedule.trace))
            self._eps_dev = torch.full((1,), float(eps_schedule.eps_train), dtype=torch.float32, device=dev)
            self._env_step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
            self._trace_env_step = torch.zeros(cap, dtype=torch.int64, device=dev)
            self._trace_eps = torch.zeros(cap, dtype=torch.float32, device=dev)
            self._select.eps_dev = self._eps_dev.data_ptr()
        self._obs_matrix = venv.obs_matrix()
        # own forward scratch: several loops may share one network on different streams
        self.workspace = torch.empty(policy.model.agents_workspace_bytes(venv.env_num, self.rows_cap),
                                     dtype=torch.uint8, device=dev)
        # the env round also writes the plan masks of the next forward into this workspace (mel_env_batch.plan_*): one
        # launch less per round
        self._plan = policy.model.plan_pointers(venv.env_num, 0 if self.per_env_logits else self.rows_cap, self.workspace)
        torch.cuda.synchronize(dev)
        venv.reset_device(self.pool, self.supply.first_episode_ids(), None)
        self._bind_plan()
        venv.round_device(self.pool, None, None, self.live, None, first=True)
        self._launch_recorder()                    # round 0 of every env's first episode
        torch.cuda.synchronize(dev)

    def _bind_plan(self):
        """Point the venv's plan sink at THIS loop's workspace (cheap; done before every launch because the struct belongs to
        the venv and another loop may have used it in between)."""
        e = self.venv.env
        e.plan_adj, e.plan_live, e.plan_u1, e.plan_u2, e.plan_cnt = self._plan

    def _launch(self):
        """The fixed launch sequence of one round (no host reads, no allocation: capturable)."""
        net = self.policy.model
        if self.eps_schedule is not None:
            self._launch_schedule()
        if self.per_env_logits:
            # forward + per-(env, agent) argmax / eps-greedy in the launch that writes the logits (same stream of draws as
            # mel_select_action_envs)
            net.hip_forward_envs(self._obs_matrix, out=self.logits, workspace=self.workspace, select=self._select,
                                 plan_ready=True, integer_features=self.integer_features)
            self._launch_decisions(None)
            self._bind_plan()
            self.venv.round_device(self.pool, self.act, None, self.live, self.table, round_counter=self.rounds,
                                   replay=self.replay)
            self._launch_train_log()
            self._launch_recorder()
            return
        # forward + fused argmax / eps-greedy (the dueling tail writes the action next to the logits)
        # (integer_features: the obs rows are the env kernel's own -> encoder / conv1 projections per feature tuple)
        net.hip_forward_agents(self._obs_matrix, self.live, self.rows_cap, out=self.logits, row_offsets=self.offsets,
                               select=self._select, workspace=self.workspace, plan_ready=True,
                               integer_features=self.integer_features)
        self._launch_decisions(self.offsets)
        self._launch_attention()
        self._bind_plan()
        self.venv.round_device(self.pool, self.act, self.offsets, self.live, self.table, round_counter=self.rounds,
                               replay=self.replay)
        self._launch_train_log()
        self._launch_recorder()

    def _launch_decisions(self, offsets):
        """What the forward just decided, with the state it decided in, into the decision tables and traces."""
        if self.decisions is not None:
            self.decisions.launch(self.logits, self.act, offsets, self.live)

    def _launch_attention(self):
        """Whom the forward's deciding agents attended to, with the state they decided in, into the attention tables."""
        if self.attention is not None:
            self.attention.launch(self.policy.model, self.workspace, self.rows_cap, self.offsets, self.live)

    def _launch_recorder(self):
        """The state the round just left, into the per-round curves and traces."""
        if self.recorder is not None:
            self.recorder.launch()

    def _launch_train_log(self):
        """The episodes the round just ended, into the training log (with the eps the round was played at)."""
        if self.train_log is not None:
            self.train_log.launch_round(self._eps_dev if self.eps_schedule is not None else None)

    def _launch_schedule(self):
        """eps of the round about to be played, from the decisions collected before it (read by the selection through
        ``mel_select.eps_dev``)."""
        sch, cap = self.eps_schedule, self._trace_eps.numel()
        _lib.check(_lib.load().mel_exploration_schedule(
            self.venv.scalars().data_ptr() + 4 * _lib.S_DECISIONS, _lib.ENV_SCALARS, self.venv.env_num, int(sch.scale),
            float(sch.eps_train), float(sch.eps_final), float(sch.exploration_fraction), float(sch.total_steps),
            self.rounds.data_ptr(), self._eps_dev.data_ptr(), self._env_step_dev.data_ptr(), cap,
            self._trace_env_step.data_ptr() if cap else None, self._trace_eps.data_ptr() if cap else None,
            _lib.current_stream_ptr(self.venv.device)), "mel_exploration_schedule")

    def eps_now(self):
        """(env_step, eps) of the last scheduled round, read from the device (synchronises); without a schedule
        (None, the host eps)."""
        if self.eps_schedule is None:
            return None, float(self.eps)
        return int(self._env_step_dev.item()), float(self._eps_dev.item())

    def eps_trace(self):
        """The schedule's trace ring as (env_step int64 [trace], eps float32 [trace]): slot ``r % trace`` holds round r's
        values (synchronises).  Needs a schedule."""
        if self.eps_schedule is None:
            raise RuntimeError("eps_trace(): this RoundLoop was built without eps_schedule")
        return self._trace_env_step.cpu().numpy(), self._trace_eps.cpu().numpy()

    def step(self):
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                self._step()
        else:
            self._step()

    def _step(self):
        # episode stream: refill on a side stream every few rounds, paced by the device-side round counter; the pacing gate
        # goes into its queue AFTER the launches it waits for (EpisodeStream.after_step)
        it = self.iterations - self._rounds_base
        self.supply.before_step(it, self.rounds)
        if self.use_graph:
            if self.graph is None:
                self._launch()                        # warm-up outside capture (lazy init)
                self.iterations += 1
                self.supply.after_step(it, self.rounds)
                torch.cuda.synchronize(self.venv.device)
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):    # launches land on the capture stream (torch's current one)
                    self._launch()
                return                                # capture does not execute: the next call replays
            # a replay runs no Python: whatever changed the weights since the last step (an optimizer step, a checkpoint load)
            # is picked up here - the converted projection weights the captured launches read are brought up to date first
            self.policy.model.ensure_prepared(self.venv.device)
            self.graph.replay()
        else:
            self._launch()
        self.iterations += 1
        self.supply.after_step(it, self.rounds)

    def _run_groups(self, groups: int):
        """``groups`` replays of the graph that holds ``graph_rounds`` rounds back to back (same launches, same buffers, same
        device-side round counter as the one-round graph: bit-identical trajectories)."""
        G, dev = self.graph_rounds, self.venv.device
        if self.group_graph is None:
            torch.cuda.synchronize(dev)
            self.group_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.group_graph):
                for _ in range(G):
                    self._launch()
        for _ in range(groups):
            it = self.iterations - self._rounds_base
            for k in range(G):
                self.supply.before_step(it + k, self.rounds)
            self.policy.model.ensure_prepared(dev)
            self.group_graph.replay()
            self.iterations += G
            for k in range(G):                    # the refill gates go into the side stream's queue behind the rounds they wait for
                self.supply.after_step(it + k, self.rounds)

    def run(self, iterations: int):
        paced = getattr(self.supply, "_paced", None)            # (event-ordered refills touch the main stream between rounds)
        while self.use_graph and self.graph is None and iterations > 0:      # eager warm-up round, then the capture
            self.step()
            iterations -= 1
        if (self.use_graph and self.graph is not None and self.graph_rounds > 1 and iterations >= self.graph_rounds
                and (paced is None or paced(self.rounds))):
            groups = iterations // self.graph_rounds
            if self.stream is not None:
                with torch.cuda.stream(self.stream):
                    self._run_groups(groups)
            else:
                self._run_groups(groups)
            iterations -= groups * self.graph_rounds
        for _ in range(iterations):
            self.step()

    def snapshot_counters(self):
        """Device-side copy of the per-env counters as they stand when the launches enqueued so far have run (no host
        synchronisation: the copy is one more launch on the loop's stream); ``counters(snapshot)`` reads it later."""
        if self.stream is not None:
            with torch.cuda.stream(self.stream):
                return (self.venv.scalars().clone(), self.iterations)
        return (self.venv.scalars().clone(), self.iterations)

    def counters(self, snapshot=None) -> dict:
        if snapshot is not None:
            return _counters_of(*snapshot)
        return _counters_of(self.venv.scalars(), self.iterations)

    def feature_table(self) -> dict:
        """What the last forward did with the node-feature table: rows used (0 = row-list path) and how many envs had a
        node feature outside the integer ranges the table assumes (must be 0 for env-produced observations)."""
        t = self.policy.model.hip_tap(3, self.venv.env_num, 0 if self.per_env_logits else self.rows_cap,
                                      workspace=self.workspace).cpu().numpy()
        return dict(table_rows=int(t[0]), bad_envs=int(t[1:].sum()))


class MultiStreamRoundLoop:
    """The GPU's envs split into independent sub-batches, each a :class:`RoundLoop` on its own HIP stream.
    One serial launch chain leaves the chip under-filled (latency-bound plan / env / attention launches, GEMM
    tails); sub-batches on separate streams fill those gaps with each other's work.  Envs are independent, so
    this changes nothing about any env's trajectory."""

    def __init__(self, make_venv, policy, n_envs: int, streams: int = 2, episodes_per_env: int = 8, seed: int = 0,
                 eps: float = 0.0, use_graph: bool = True, ring: int = 16):
        per = (n_envs + streams - 1) // streams
        self.loops = []
        for k in range(streams):
            lo, hi = k * per, min((k + 1) * per, n_envs)
            if hi <= lo:
                break
            venv = make_venv(hi - lo, seed + lo)
            self.loops.append(RoundLoop(venv, policy, episodes_per_env=episodes_per_env, seed=seed + lo, eps=eps,
                                        use_graph=use_graph, stream=torch.cuda.Stream(device=venv.device), ring=ring))
        self.iterations = 0

    @property
    def use_graph(self):
        return self.loops[0].use_graph

    @use_graph.setter
    def use_graph(self, v):
        for l in self.loops:
            l.use_graph = v

    def step(self):
        for l in self.loops:
            l.step()
        self.iterations += 1

    def run(self, iterations: int):
        for _ in range(iterations):
            self.step()

    def snapshot_counters(self):
        return [l.snapshot_counters() for l in self.loops]

    def counters(self, snapshot=None) -> dict:
        out = dict(decisions=0, episodes=0, errors=0, iterations=self.iterations)
        for k, l in enumerate(self.loops):
            c = l.counters(snapshot[k] if snapshot is not None else None)
            out["decisions"] += c["decisions"]
            out["episodes"] += c["episodes"]
            out["errors"] |= c["errors"]
        return out


@dataclasses.dataclass
class SequenceSummaryStats:
    """[3P] tianshou 1.0.0 ``SequenceSummaryStats``: mean / std / max / min of a sequence (what ``returns_stat`` / ``lens_stat`` /
    ``info.stats[key]`` of the reference's collect result hold, collector.py:14-36)."""
    mean: float
    std: float
    max: float
    min: float

    @classmethod
    def from_sequence(cls, sequence) -> "SequenceSummaryStats":
        a = np.asarray(sequence, dtype=np.float64)
        return cls(mean=float(a.mean()), std=float(a.std()), max=float(a.max()), min=float(a.min()))


@dataclasses.dataclass
class DictOfSequenceSummaryStats:
    """collector.py:14-30: ``stats[key]`` summarises the values of ``logger_stats[key]`` (graph.py:166-178)."""
    stats: dict

    @classmethod
    def from_dict(cls, stats: dict) -> "DictOfSequenceSummaryStats":
        return cls(stats={k: SequenceSummaryStats.from_sequence(v) for k, v in stats.items() if len(v)})


class StepStatsPool:
    """Host model of the device's per-step ``logger_stats`` accumulator (``mel_env_batch.step_stats``, env.hip ``StepPool``):
    per key the sample count, running mean, M2 (sum of squared deviations from the mean), min and max, merged by the Chan /
    Welford rule in the kernels' own operation order -

        n = na + nb;  d = mb - ma;  mean = ma + d * nb / n;  M2 = M2a + M2b + d * d * na * nb / n

    - never sum and sum of squares (the std of ``total_messages_transmitted``-sized values over 1e5 rows must not cancel).
    Count-gated: an empty side of a merge leaves the other untouched, the first sample sets mean = min = max = value and
    M2 = 0, so a constant sequence has std == 0 exactly."""

    def __init__(self, keys: int = _lib.ENV_LOGGER_STATS):
        self.count = 0
        self.mean, self.m2 = np.zeros(keys), np.zeros(keys)
        self.min, self.max = np.zeros(keys), np.zeros(keys)

    @classmethod
    def from_row(cls, row) -> "StepStatsPool":
        """One env's accumulator as the device stores it: ``[1 + 4 * keys]`` = count, then per key mean, M2, min, max."""
        row = np.asarray(row, dtype=np.float64)
        self = cls((len(row) - 1) // 4)
        body = row[1:].reshape(-1, 4)
        self.count = int(row[0])
        self.mean, self.m2, self.min, self.max = (body[:, j].copy() for j in range(4))
        return self

    def to_row(self) -> np.ndarray:
        return np.concatenate([[float(self.count)], np.stack([self.mean, self.m2, self.min, self.max], axis=1).reshape(-1)])

    def add(self, values, count: int = 1) -> "StepStatsPool":
        """``count`` identical samples (one value per key) in ONE merge: a block with n = count, mean = values, M2 = 0."""
        block = StepStatsPool(len(self.mean))
        v = np.asarray(values, dtype=np.float64)
        block.count, block.mean, block.min, block.max = int(count), v.copy(), v.copy(), v.copy()
        return self.merge(block)

    def merge(self, other: "StepStatsPool") -> "StepStatsPool":
        if other.count == 0:
            return self
        if self.count == 0:
            self.count = other.count
            self.mean, self.m2, self.min, self.max = other.mean.copy(), other.m2.copy(), other.min.copy(), other.max.copy()
            return self
        na, nb = float(self.count), float(other.count)
        n = na + nb
        d = other.mean - self.mean
        self.mean = self.mean + d * nb / n
        self.m2 = self.m2 + other.m2 + d * d * na * nb / n
        self.min, self.max = np.minimum(self.min, other.min), np.maximum(self.max, other.max)
        self.count += other.count
        return self

    def summary(self, keys=_lib.LOGGER_KEYS) -> dict:
        """{key: SequenceSummaryStats} with the population std sqrt(M2 / n) of ``SequenceSummaryStats.from_sequence``; empty
        without a sample."""
        if self.count == 0:
            return {}
        std = np.sqrt(self.m2 / float(self.count))
        return {key: SequenceSummaryStats(mean=float(self.mean[k]), std=float(std[k]), max=float(self.max[k]),
                                          min=float(self.min[k])) for k, key in enumerate(keys)}


@dataclasses.dataclass
class CollectStatsWithInfo:
    """The reference collectors' return value (collector.py:33-36 on top of [3P] tianshou ``CollectStats``; built at
    multi_agent_collector.py:341-353) with the reference's field names.  ``returns[i]`` is episode i's reward sum as the env
    reports it at the episode's last step (``logger_stats['episode_rewards_sum']``, graph.py:166-178), ``lens[i]`` its number
    of rounds - not the reference's ``ep_rew`` / ``ep_len`` of the last saved sub-buffer.  ``info.stats[key]``: with a
    collector built with ``stats="episodes"`` (the default) it summarises the episodes' FINAL ``logger_stats``; with
    ``stats="steps"`` it is what the reference computes, the mean / std / max / min of ``logger_stats[key]`` over EVERY
    collected env step (multi_agent_collector.py:276,316-322), pooled on the device, and ``n_info_rows`` is the number of
    pooled steps.  ``episode_info``: the per-episode values (the rows behind ``info`` in "episodes" mode).  The mapping
    protocol (``result["n/ep"]`` ...) is the Tianshou-0.x spelling of the same numbers, kept for callers written against it."""
    n_collected_episodes: int = 0
    n_collected_steps: int = 0
    collect_time: float = 0.0
    collect_speed: float = 0.0
    returns: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0))
    returns_stat: "SequenceSummaryStats | None" = None
    lens: np.ndarray = dataclasses.field(default_factory=lambda: np.zeros(0, int))
    lens_stat: "SequenceSummaryStats | None" = None
    info: "DictOfSequenceSummaryStats | None" = None
    episode_info: dict = dataclasses.field(default_factory=dict)
    n_info_rows: int = 0

    _ALIASES = {"n/ep": "n_collected_episodes", "n/st": "n_collected_steps"}

    def __getitem__(self, key):
        if key in self._ALIASES:
            return getattr(self, self._ALIASES[key])
        if key in ("rew", "len"):
            stat = self.returns_stat if key == "rew" else self.lens_stat
            if stat is None:
                raise KeyError(key)
            return stat.mean
        if key != "info" and self.info is not None and key in self.info.stats:
            return self.info.stats[key].mean
        if key.startswith("_") or not hasattr(self, key):
            raise KeyError(key)
        return getattr(self, key)

    def __contains__(self, key):
        try:
            self[key]
            return True
        except KeyError:
            return False

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        names = [f.name for f in dataclasses.fields(self)] + ["n/ep", "n/st"]
        if self.returns_stat is not None:
            names += ["rew", "len"]
        return names + (list(self.info.stats) if self.info is not None else [])

    def __iter__(self):
        return iter(self.keys())

    def items(self):
        return [(k, self[k]) for k in self.keys()]


def result_from_episode_log(stats: np.ndarray, meta: np.ndarray, total: int, steps: int, dt: float) -> CollectStatsWithInfo:
    """The collect result from the device's episode log (``HipGraphVectorEnv.read_episode_log``: one row per finished episode
    = the ``logger_stats`` of its last step and (env, pool episode, num_moves)), ``steps`` collected decisions, ``dt`` seconds."""
    episode_info = {k: stats[:, i].copy() for i, k in enumerate(_lib.LOGGER_KEYS)}
    returns = episode_info["episode_rewards_sum"].copy()
    lens = meta[:, 2].astype(int)
    return CollectStatsWithInfo(
        n_collected_episodes=total, n_collected_steps=steps, collect_time=dt, collect_speed=steps / dt,
        returns=returns, returns_stat=SequenceSummaryStats.from_sequence(returns) if len(returns) else None,
        lens=lens, lens_stat=SequenceSummaryStats.from_sequence(lens) if len(lens) else None,
        info=DictOfSequenceSummaryStats.from_dict(episode_info), episode_info=episode_info)


class Collector:
    """The collect() surface of the reference's collectors (multi_agent_collector.py:89-353: ``collect(n_step=...)`` /
    ``collect(n_episode=...)`` returning counts, speed and the episodes' ``logger_stats``) on top of the device-resident
    :class:`RoundLoop`: rounds are issued in chunks without host reads, the device counters and the on-device episode
    log (``mel_env_batch.log_*``) are read between chunks.  ``n_step`` counts live agent decisions (what the reference
    counts as collected transitions), ``n_episode`` finished episodes.  Evaluation as in l_dgn.py:92-129: build the
    vector env with ``is_testing=True`` and call ``collect(n_episode=...)``."""

    def __init__(self, policy, venv: HipGraphVectorEnv, episodes_per_env: int = 16, seed: int = 0, eps: float = 0.0,
                 replay=None, log_capacity: int = 65536, chunk: int = 8, use_graph: bool = True,
                 episode_stream: "bool | str | None" = None, ring: int = 16, stats: str = "episodes", recorder=None,
                 decisions=None, attention=None):
        """``episode_stream`` / ``ring`` / ``recorder`` / ``decisions`` / ``attention``: the episode supply, the per-round recorder, the decision recorder and the attention recorder, as :class:`RoundLoop` takes them.  ``stats``: what ``info`` of a
        collect result summarises - ``"episodes"``: the final ``logger_stats`` row of each finished episode; ``"steps"``: the
        ``logger_stats`` of every env step played during the call, as the reference pools them
        (multi_agent_collector.py:276,316-322), accumulated by the env kernels (``HipGraphVectorEnv.enable_step_stats``)."""
        if stats not in ("episodes", "steps"):
            raise ValueError(f"stats={stats!r}: 'episodes' or 'steps'")
        self.venv, self.policy, self.chunk, self.stats = venv, policy, int(chunk), stats
        venv.enable_episode_log(log_capacity)
        if stats == "steps":
            venv.enable_step_stats()            # before the loop: its `first` launch and every capture see the pool
        self.loop = RoundLoop(venv, policy, episodes_per_env=episodes_per_env, seed=seed, eps=eps, replay=replay,
                              use_graph=use_graph, episode_stream=episode_stream, ring=ring, recorder=recorder,
                              decisions=decisions, attention=attention)
        self._decisions = self.loop.counters()["decisions"]
        self.collect_step, self.collect_episode, self.collect_time = 0, 0, 0.0

    def collect(self, n_step: int | None = None, n_episode: int | None = None) -> CollectStatsWithInfo:
        import time
        if (n_step is None) == (n_episode is None):
            raise ValueError("give exactly one of n_step / n_episode")        # the reference asserts the same
        self.venv.log_cursor.zero_()
        if self.stats == "steps":
            self.venv.step_stats.zero_()        # a device buffer: the captured round graphs keep replaying
        t0 = time.perf_counter()
        steps = episodes = 0
        with torch.no_grad():
            while (n_step is not None and steps < n_step) or (n_episode is not None and episodes < n_episode):
                self.loop.run(self.chunk)
                c = self.loop.counters()                                      # synchronises
                steps = c["decisions"] - self._decisions
                episodes = int(self.venv.log_cursor.item())
                if c["errors"]:
                    raise RuntimeError(f"env error flags {c['errors']:#x} (episode pool exhausted or desynchronised actions)")
        dt = max(time.perf_counter() - t0, 1e-9)
        stats, meta, total = self.venv.read_episode_log()
        self._decisions += steps
        self.collect_step += steps
        self.collect_episode += total
        self.collect_time += dt
        result = result_from_episode_log(stats, meta, total, steps, dt)
        if self.stats == "steps":
            result.n_info_rows, pooled = self.venv.read_step_stats()
            result.info = DictOfSequenceSummaryStats(stats=pooled)
        else:
            result.n_info_rows = len(stats)
        return result

    def set_eps(self, eps: float) -> None:
        """Exploration rate of the following collects.  The rate is an argument of the selection fused into the forward's last
        launch: in HIP-graph mode a new value means a new capture (taken by the next round)."""
        eps = float(eps)
        if eps != self.loop.eps:
            self.loop.eps = eps
            self.loop._select.eps = eps
            self.loop.graph = None


def test_shares(n_episode: int, n_envs: int) -> list:
    """How many of the ``n_episode`` list positions env b of ``n_envs`` owns when the evaluation schedule is spread
    (positions ``b, b + n_envs, ...`` below ``n_episode``): ``ceil((n_episode - b) / n_envs)``, 0 for envs beyond the list."""
    return [max(0, -(-(int(n_episode) - b) // int(n_envs))) for b in range(int(n_envs))]


test_shares.__test__ = False           # (a helper, whatever the name says to pytest)


def evaluate_spread(policy, venv: HipGraphVectorEnv, n_episode: int, eps: float = 0.0, seed: int = 0, use_graph: bool = True,
                    chunk: int = 8, ring: int = 16, log_capacity: int | None = None, recorder=None, decisions=None,
                    attention=None):
    """One pass over the evaluation schedule with all envs of ``venv`` at once: ``venv`` is built with ``is_testing=True,
    num_test_episodes=n_episode, spread_test_episodes=True``, so env b owns the list positions ``b, b + B, ...``
    (:func:`test_shares`; envs beyond the list own none).  The episodes come from the device sampler
    (:class:`melissa_amd.env.stream.TestEpisodeStream`), the rounds replay from the HIP graph in chunks of ``chunk`` until
    every env has finished its share.  An env that is done keeps playing while the others finish (it walks on through the
    list): those surplus episodes are dropped - of env b's rows in the episode log (they appear in play order) the first
    share-many count, and the e-th of them is list position ``b + e * B``.

    -> (:class:`CollectStatsWithInfo` with ``returns`` / ``lens`` / ``episode_info`` in list-position order, positions).
    ``n_collected_steps`` counts every decision taken, the surplus episodes' included.  The loop is built with ``eps`` and
    used once; calling again on the same ``venv`` starts again from the top of the list.

    ``recorder`` (:class:`melissa_amd.round_record.RoundRecorder` on ``venv``): reset here, given the shares as its quota - so
    the surplus episodes stay out of its curves and traces too - and launched behind every round; its traces are drained after
    every chunk, where this loop synchronises anyway (read the result with ``recorder.curves()`` / ``recorder.drain_traces()``).
    A ring of fewer than ``2 * chunk`` trace records could be overrun between two drains: ValueError.
    ``decisions`` (:class:`melissa_amd.decision_record.DecisionRecorder` on ``venv``): the same - reset, the shares as its quota,
    launched between every round's forward and env launch, drained after every chunk (``decisions.tables()`` /
    ``decisions.drain_traces()``).
    ``attention`` (:class:`melissa_amd.attention_record.AttentionRecorder` on ``venv`` and the policy's network): the same once
    more (``attention.tables()`` / ``attention.drain_traces()``)."""
    import time
    kw, B, T = venv._sampler_kw, venv.env_num, int(n_episode)
    if not kw["is_testing"] or int(kw["num_test_episodes"]) != T:
        raise ValueError(f"evaluate_spread plays the whole list once: the env needs is_testing and num_test_episodes={T}")
    if (kw.get("test_env_step", 0), kw.get("test_episode_step", 1)) != (1, B):
        raise ValueError("evaluate_spread needs an env built with spread_test_episodes=True")
    shares = np.asarray(test_shares(T, B))
    capacity = int(log_capacity) if log_capacity is not None else max(1024, 16 * (T + B))
    t0 = time.perf_counter()
    for name, rec in (("recorder", recorder), ("decisions", decisions), ("attention", attention)):
        check_rides("evaluate_spread", name, rec, venv, chunk=chunk)
    venv.scalars().zero_()                     # the episode cursors count from 0 again: this pass starts at the top
    for rec in (recorder, decisions, attention):
        if rec is not None:
            rec.reset()
            rec.set_quota(shares)
    col = Collector(policy, venv, seed=seed, eps=eps, chunk=chunk, use_graph=use_graph, log_capacity=capacity,
                    episode_stream="test", ring=ring, recorder=recorder, decisions=decisions,
                    attention=attention)
    with torch.no_grad():
        while True:
            col.loop.run(col.chunk)
            sc = venv.scalars().cpu().numpy()                                     # synchronises
            for rec in (recorder, decisions, attention):
                if rec is not None:
                    rec.drain_traces()
            errors = int(np.bitwise_or.reduce(sc[:, _lib.S_ERROR]))
            if errors:
                raise RuntimeError(f"env error flags {errors:#x} (episode pool exhausted or desynchronised actions)")
            if (sc[:, _lib.S_EPISODES_DONE] >= shares).all():
                break
            if int(venv.log_cursor.item()) >= capacity:
                raise RuntimeError(f"the episode log ({capacity} rows) filled before every env finished its share of the "
                                   f"evaluation: raise log_capacity")
    col.loop.supply.side.synchronize()         # (the last refill may still be writing the ring this call is about to drop)
    steps = int(sc[:, _lib.S_DECISIONS].sum()) - col._decisions
    stats, meta, _total = venv.read_episode_log()
    rows, positions = [], []
    for b in range(B):
        mine = np.flatnonzero(meta[:, 0] == b)[:shares[b]]
        if len(mine) < shares[b]:
            raise RuntimeError(f"the episode log ({capacity} rows) dropped rows of env {b}'s share: raise log_capacity")
        rows.extend(mine.tolist())
        positions.extend(b + e * B for e in range(shares[b]))
    order = np.argsort(np.asarray(positions, dtype=np.int64), kind="stable")
    rows, positions = np.asarray(rows, dtype=np.int64)[order], np.asarray(positions, dtype=np.int64)[order]
    dt = max(time.perf_counter() - t0, 1e-9)
    return result_from_episode_log(stats[rows], meta[rows], T, steps, dt), positions


class MultiAgentCollector(Collector):
    """``MultiAgentCollector(agents_num, policy=..., env=..., buffer=None, exploration_noise=False)`` with
    ``collect(n_step | n_episode, random, render, no_grad)`` -> :class:`CollectStatsWithInfo` - the reference's constructor and
    call (multi_agent_collector.py:31-42, 89-118; call sites l_dgn.py:119-127, 185-201) in front of the device-resident
    :class:`RoundLoop`.  One line changes in the reference's scripts: the import.

    * ``env``: a :class:`melissa_amd.env.HipGraphVectorEnv` (the vector env of the scripts' ``DummyVectorEnv([...])``);
      ``agents_num`` must be its node count.
    * ``buffer``: a :class:`melissa_amd.replay.RoundReplay`, a :class:`melissa_amd.replay.PrioritizedRoundReplay` (the scripts'
      ``--prio-buffer``: ``PrioritizedVectorReplayBuffer``, multi_agent_collector.py:60-65) or None.  The reference routes every agent's transition into one of
      ``env_num * agents_num`` sub-buffers and holds it back until the agent's next observation arrives
      (multi_agent_collector.py:229-271); here a whole env round is one record and ``RoundReplay.export_transitions()``
      yields the same transitions with the reference's ``buffer_id = env * agents_num + agent``.
    * ``exploration_noise``: eps-greedy with ``policy.eps`` (set by ``policy.set_eps`` in the scripts' ``train_fn``) when True,
      greedy when False - [3P] ``DQNPolicy.exploration_noise`` through shared_policy.py:81-91, drawn on the device.
    * ``random=True``: uniformly random actions (eps = 1), as ``self._action_space[i].sample()`` does.
    * ``render``: not offered (the reference's matplotlib view, graph.py:466-484, is out of scope): a truthy value raises.
    * ``no_grad``: accepted and ignored - the collect path never builds an autograd graph (the HIP forward has none).
    * ``stats="steps"``: ``info`` pools the ``logger_stats`` of every collected env step like the reference's (see
      :class:`Collector`); the default ``"episodes"`` summarises the finished episodes' final rows."""

    def __init__(self, agents_num, policy=None, env=None, buffer=None, exploration_noise: bool = False, preprocess_fn=None,
                 seed: int = 0, episodes_per_env: int = 16, chunk: int = 8, use_graph: bool = True, log_capacity: int = 65536,
                 stats: str = "episodes"):
        if policy is None or env is None:
            raise TypeError("MultiAgentCollector needs policy= and env=")
        if preprocess_fn is not None:
            raise NotImplementedError("preprocess_fn: the rounds never leave the device; nothing to hook per step")
        if int(agents_num) != env.n:
            raise ValueError(f"agents_num={agents_num} but the env has {env.n} agents")
        self.agents_num = int(agents_num)
        self.exploration_noise = bool(exploration_noise)
        self.env, self.buffer = env, buffer
        policy = getattr(policy, "policy", policy)          # a MultiAgentSharedPolicy manager wraps the one shared policy
        eps = float(getattr(policy, "eps", 0.0)) if exploration_noise else 0.0
        super().__init__(policy, env, episodes_per_env=episodes_per_env, seed=seed, eps=eps, replay=buffer,
                         log_capacity=log_capacity, chunk=chunk, use_graph=use_graph, stats=stats)

    @property
    def env_num(self) -> int:
        return self.venv.env_num

    def reset(self, reset_buffer: bool = True, gym_reset_kwargs=None) -> None:
        """[3P] ``Collector.reset``: statistics (and the buffer's write cursors) back to zero; the envs keep running - every
        episode end already draws a fresh episode on the device."""
        self.reset_stat()
        if reset_buffer:
            self.reset_buffer()

    def reset_stat(self) -> None:
        self.collect_step, self.collect_episode, self.collect_time = 0, 0, 0.0

    def reset_buffer(self, keep_statistics: bool = False) -> None:
        if self.buffer is not None:
            self.buffer.cursor.zero_()
            self.buffer.episode.fill_(-1)
            if hasattr(self.buffer, "reset_priorities"):    # PrioritizedRoundReplay: priorities, seen, max_prio / min_prio too
                self.buffer.reset_priorities()

    def reset_env(self, gym_reset_kwargs=None) -> None:
        """(the reference resets all envs after an n_episode collect; the device envs reset themselves at every episode end)"""

    def collect(self, n_step: int | None = None, n_episode: int | None = None, random: bool = False, render=False,
                no_grad: bool = False, gym_render_kwargs=None) -> CollectStatsWithInfo:
        if render:
            raise NotImplementedError("render: the reference's matplotlib view (graph.py:466-484) is out of scope")
        if n_step is not None and n_episode is not None:
            raise AssertionError(f"Only one of n_step or n_episode is allowed in Collector.collect, got n_step={n_step}, "
                                 f"n_episode={n_episode}.")
        if n_step is None and n_episode is None:
            raise TypeError("Please specify at least one (either n_step or n_episode) in AsyncCollector.collect().")
        if (n_step is not None and n_step <= 0) or (n_episode is not None and n_episode <= 0):
            raise AssertionError("n_step / n_episode must be positive")
        eps = 1.0 if random else (float(getattr(self.policy, "eps", 0.0)) if self.exploration_noise else 0.0)
        self.set_eps(eps)
        return super().collect(n_step=n_step, n_episode=n_episode)


class CollectiveExperienceCollector(MultiAgentCollector):
    """``CollectiveExperienceCollector(agents_num, policy=..., env=..., buffer=None, exploration_noise=False)`` - the collector of
    the collective scripts (collective_experience_collector.py:20; dgn_r.py, n_dgn_r.py, l_n_dgn_r.py, hl_n_dgn_r.py).  Besides each
    transition it keeps what the collective losses read: the siblings (``info.indices``, :70-80 - in a round record they are the
    ``acted`` set) and the ``info`` of the agent's next observation (:270-290), of which N-DGN reads
    ``active_one_hop_neighbors``.  So the buffer must record neighbours: ``buffer=None`` creates a
    ``RoundReplay(neighbours=True)`` of ``buffer_rounds`` records per env (1: the reference's default
    ``VectorReplayBuffer(env_num * agents_num, env_num * agents_num)`` holds one transition per sub-buffer); a given
    :class:`melissa_amd.replay.RoundReplay` without neighbours raises; a ``PrioritizedRoundReplay(neighbours=True)`` is accepted
    like the reference's prioritized buffer (:60-62).  Everything else is :class:`MultiAgentCollector`."""

    def __init__(self, agents_num, buffer=None, buffer_rounds: int = 1, **kwargs):
        from .replay import RoundReplay
        env = kwargs.get("env")
        if buffer is None and env is not None:
            buffer = RoundReplay(env.env_num, int(agents_num), int(buffer_rounds), env.device, neighbours=True)
        elif buffer is not None and getattr(buffer, "active_nb", None) is None:
            raise ValueError("CollectiveExperienceCollector needs a buffer that records neighbours: RoundReplay(..., neighbours=True)")
        super().__init__(agents_num, buffer=buffer, **kwargs)
