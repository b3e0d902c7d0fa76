"""Device-resident replay for the round-batched loop + n-step return sampling.

Reference: the collectors route each agent's transition into one of ``num_envs x num_agents`` Tianshou
sub-buffers, waiting for the agent's next observation before the record is complete
(multi_agent_collector.py:229-271); ``DQNPolicy.process_fn`` then builds n-step returns
(``estimation_step`` = 4, common.py:28).  In the round-batched loop a whole env round is ONE record
(``mel_round_replay`` in include/melissa_hip.h) written by ``mel_env_round``: all of the round's agents share
``obs`` / ``obs_next`` (they observe the same obs_matrix, graph.py:186-188), so a transition is
``(record, agent)`` and an agent's trajectory is the run of consecutive records of its env in which it acts.
:class:`PrioritizedRoundReplay` samples those transitions by priority (the scripts' ``--prio-buffer``: [3P]
``PrioritizedVectorReplayBuffer``, l_dgn.py:169-176).
"""
from __future__ import annotations

import torch

from . import _lib
from .optim import adam_step
from .td import td_target


class RoundReplay:
    """``neighbours=True`` also records, for each acting agent, ``info['active_one_hop_neighbors']`` at its next observation
    (``active_nb`` [B, K, N(, W)], N * W * 8 bytes per record): what the collective collector stores with every transition and
    N-DGN restricts the sibling sum to (policies/n_dgn.py:36-47, :class:`NDGNLearner`)."""

    def __init__(self, n_envs: int, n_nodes: int, capacity: int, device, neighbours: bool = False):
        self.B, self.n, self.K = n_envs, n_nodes, capacity
        dev = torch.device(device)
        self.obs = torch.zeros(n_envs, capacity, 8 * n_nodes, dtype=torch.float32, device=dev)
        self.obs_next = torch.zeros_like(self.obs)
        # node sets (who acted / who was terminated by the round): one int64 word up to 64 nodes, [W] words beyond
        self.W = _lib.set_words(n_nodes)
        ws = () if self.W == 1 else (self.W,)
        self.acted = torch.zeros(n_envs, capacity, *ws, dtype=torch.int64, device=dev)
        self.done = torch.zeros(n_envs, capacity, *ws, dtype=torch.int64, device=dev)
        self.act = torch.zeros(n_envs, capacity, n_nodes, dtype=torch.int8, device=dev)
        self.rew = torch.zeros(n_envs, capacity, n_nodes, dtype=torch.float32, device=dev)
        self.episode = torch.full((n_envs, capacity), -1, dtype=torch.int32, device=dev)
        self.cursor = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        s = _lib.MelRoundReplay()
        s.capacity = capacity
        s.obs, s.obs_next = self.obs.data_ptr(), self.obs_next.data_ptr()
        s.acted, s.done, s.act = self.acted.data_ptr(), self.done.data_ptr(), self.act.data_ptr()
        s.rew, s.episode, s.cursor = self.rew.data_ptr(), self.episode.data_ptr(), self.cursor.data_ptr()
        self.active_nb = None
        if neighbours:
            self.active_nb = torch.zeros(n_envs, capacity, n_nodes, *ws, dtype=torch.int64, device=dev)
            s.active_nb = self.active_nb.data_ptr()
        self.struct = s
        node = torch.arange(n_nodes, device=dev)
        self._word, self._shift = node // 64, node % 64

    def __len__(self) -> int:
        """Transitions currently held (synchronises)."""
        valid = self._valid_slots()
        return int(self._popcount(self.acted[valid]).sum())

    def _members(self, m: torch.Tensor) -> torch.Tensor:
        """node sets int64 [..., (W)] -> bool [..., N]."""
        if self.W == 1:
            m = m[..., None]
        return ((m[..., self._word] >> self._shift) & 1) != 0

    def _has(self, m: torch.Tensor, agent: torch.Tensor) -> torch.Tensor:
        """node sets int64 [bs, (W)], agent [bs] -> bool [bs]: is agent[i] a member of m[i]?"""
        if self.W == 1:
            m = m[..., None]
        return ((m.gather(-1, (agent // 64)[:, None]).squeeze(-1) >> (agent % 64)) & 1) != 0

    def _bit(self, agent: torch.Tensor) -> torch.Tensor:
        """agent [bs] -> node sets int64 [bs, (W)] holding just that agent."""
        one = torch.ones_like(agent)
        if self.W == 1:
            return one << agent
        return torch.where(agent[:, None] // 64 == torch.arange(self.W, device=agent.device)[None, :],
                           one[:, None] << (agent % 64)[:, None], torch.zeros_like(agent)[:, None])

    def _popcount(self, m: torch.Tensor) -> torch.Tensor:
        return self._members(m).sum(-1)

    def _valid_slots(self) -> torch.Tensor:
        filled = torch.clamp(self.cursor.long(), max=self.K)                       # [B]
        return torch.arange(self.K, device=self.cursor.device)[None, :] < filled[:, None]

    def sample(self, batch_size: int, n_step: int, gamma: float, generator: torch.Generator | None = None):
        """Uniform over (record, acting agent) pairs.  Returns dict of device tensors:
        obs [bs, 8N+1], act [bs], ret [bs] (discounted n-step reward sum), boot_obs [bs, 8N+1] (observation to
        bootstrap from), boot_w [bs] (gamma^steps, 0 when the agent terminated inside the window), env / slot / agent [bs];
        with ``neighbours`` also nb_sibling [bs, (W)]: ``acted & (active_nb[agent] | agent)``, the siblings N-DGN sums over.

        On the GPU this is ONE launch (``mel_replay_sample``; the index arithmetic below is ~150 small launches, 0.6 ms of a
        1.7 ms update replayed from HIP graphs): draws are a counter-based function of the generator's seed and a device-side
        counter that every call advances, so a captured call keeps drawing new batches when replayed.  Host tensors (CPU tests
        of the host logic) take the torch formulation below - same distribution, torch's own random stream."""
        dev = self.obs.device
        if dev.type == "cuda":
            return self._sample_device(batch_size, n_step, gamma, generator)
        valid = self._valid_slots()
        # never start a chain in the slot about to be overwritten next
        cnt = self._popcount(self.acted) * valid
        flat = cnt.flatten().float()
        idx = torch.multinomial(flat, batch_size, replacement=True, generator=generator)
        e, k = idx // self.K, idx % self.K
        mask = self.acted[e, k]
        # pick the j-th acting agent uniformly
        bits = self._members(mask)                                                 # [bs, N]
        u = torch.rand(batch_size, device=dev, generator=generator)
        target = (u * bits.sum(1)).floor().long().clamp(max=self.n - 1)
        order = torch.cumsum(bits.long(), dim=1) - 1
        agent = ((order == target[:, None]) & bits).float().argmax(dim=1)
        return self._walk_host(e, k, agent, n_step, gamma)

    def _walk_host(self, e: torch.Tensor, k: torch.Tensor, agent: torch.Tensor, n_step: int, gamma: float) -> dict:
        """The n-step walk and the batch of the picked transitions (env e, slot k, agent): what follows the pick in ``sample``."""
        dev, batch_size, valid = self.obs.device, e.numel(), self._valid_slots()
        ret = torch.zeros(batch_size, device=dev)
        boot_w = torch.ones(batch_size, device=dev)
        alive = torch.ones(batch_size, dtype=torch.bool, device=dev)
        boot_slot = k.clone()
        ep0 = self.episode[e, k]
        newest = (self.cursor[e].long() - 1) % self.K
        kk = k.clone()
        for j in range(n_step):
            ok = alive & (self.episode[e, kk] == ep0) & self._has(self.acted[e, kk], agent) & valid[e, kk]
            ret = ret + torch.where(ok, (gamma ** j) * self.rew[e, kk, agent], torch.zeros((), device=dev))
            boot_slot = torch.where(ok, kk, boot_slot)
            boot_w = torch.where(ok, torch.full((), gamma ** (j + 1), device=dev), boot_w)
            finished = ok & self._has(self.done[e, kk], agent)
            boot_w = torch.where(finished, torch.zeros((), device=dev), boot_w)
            alive = ok & ~finished & (kk != newest)          # cannot walk past the newest record
            kk = (kk + 1) % self.K
        idx_col = agent.float()[:, None]
        obs = torch.cat([self.obs[e, k], idx_col], dim=1)
        boot_obs = torch.cat([self.obs_next[e, boot_slot], idx_col], dim=1)
        out = dict(obs=obs, act=self.act[e, k, agent].long(), ret=ret, boot_obs=boot_obs, boot_w=boot_w,
                   env=e, slot=k, agent=agent)
        if self.active_nb is not None:
            out["nb_sibling"] = self.acted[e, k] & (self.active_nb[e, k, agent] | self._bit(agent))
        return out


    def sampler_scratch(self) -> None:
        """The device sampler's draw counter (state: every sample advances it) and prefix scratch, created by the first sample -
        or by whoever restores a saved counter before one (:mod:`melissa_amd.train_state`)."""
        if not hasattr(self, "_draws"):
            dev = self.obs.device
            self._draws = torch.zeros(1, dtype=torch.int64, device=dev)            # device-side draw counter
            self._prefix = torch.empty(self.B * self.K + 1, dtype=torch.int32, device=dev)

    def _device_batch(self, batch_size: int, n_step: int, gamma: float, generator):
        """Output tensors of a one-launch sample + what both samplers pass to the library: (out, MelReplayBatch, discount, seed)."""
        import ctypes as C
        dev = self.obs.device
        if not getattr(self, "_nonempty", False):               # (one host read, until the first record is seen)
            if int(self.cursor.max()) < 1:
                raise ValueError("cannot sample from an empty replay: run the collect loop first")
            self._nonempty = True
        self.sampler_scratch()
        width = 8 * self.n + 1
        out = dict(obs=torch.empty(batch_size, width, device=dev), boot_obs=torch.empty(batch_size, width, device=dev),
                   act=torch.empty(batch_size, dtype=torch.int64, device=dev), ret=torch.empty(batch_size, device=dev),
                   boot_w=torch.empty(batch_size, device=dev), env=torch.empty(batch_size, dtype=torch.int64, device=dev),
                   slot=torch.empty(batch_size, dtype=torch.int64, device=dev),
                   agent=torch.empty(batch_size, dtype=torch.int64, device=dev))
        if self.active_nb is not None:
            out["nb_sibling"] = torch.empty(batch_size, *self.acted.shape[2:], dtype=torch.int64, device=dev)
        b = _lib.MelReplayBatch()
        for name, t in out.items():
            setattr(b, name, t.data_ptr())
        disc = (C.c_float * (n_step + 1))(*[gamma ** j for j in range(n_step + 1)])
        seed = (generator.initial_seed() if generator is not None else torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF
        return out, b, disc, seed

    def _sample_device(self, batch_size: int, n_step: int, gamma: float, generator):
        import ctypes as C
        dev, lib = self.obs.device, _lib.load()
        out, b, disc, seed = self._device_batch(batch_size, n_step, gamma, generator)
        _lib.check(lib.mel_replay_sample(C.byref(self.struct), self.B, self.n, batch_size, n_step, disc, seed,
                                         self._draws.data_ptr(), self._prefix.data_ptr(), C.byref(b),
                                         _lib.current_stream_ptr(dev)), "mel_replay_sample")
        return out

    def sample_collective(self, batch_size: int, n_step: int, gamma: float, generator: torch.Generator | None = None):
        """``sample`` plus every sampled transition's SIBLINGS - the agents that acted in the same env round
        (what collective_experience_collector.py:70-80 records as ``info.indices``): here they are simply the
        ``acted`` set of the same record.  Adds ``active_obs`` [M, 8N+1], ``active_act`` [M], ``segment`` [M]
        (rows ordered by experience, then agent id) for :class:`melissa_amd.policy.DGNPolicy`."""
        b = self.sample(batch_size, n_step, gamma, generator)
        e, k = b["env"], b["slot"]
        bits = self._members(self.acted[e, k])                                     # [bs, N]
        seg, agent = torch.nonzero(bits, as_tuple=True)                            # row-major: by experience, then id
        obs = torch.cat([self.obs[e[seg], k[seg]], agent.float()[:, None]], dim=1)
        b.update(active_obs=obs, active_act=self.act[e[seg], k[seg], agent].long(), segment=seg, sibling_mask=self.acted[e, k])
        return b

    def export_transitions(self):
        """The buffer in the reference collectors' layout (multi_agent_collector.py:229-271,
        collective_experience_collector.py:70-80,251-309): one row per (record, acting agent) transition with
        ``buffer_id = env * N + agent`` (the Tianshou VectorReplayBuffer sub-buffer it is routed to) and
        ``indices`` [T, N]: row of each SIBLING transition (agent j acted in the same env round) or -1.
        Rows are ordered by env, record age (oldest first), agent id.  With ``neighbours``, ``active_one_hop_neighbors`` [T, N]
        bool: the info of the agent's next observation, as the collective collector stores it (:270-290).  Host NumPy;
        synchronises."""
        import numpy as np
        valid = self._valid_slots()
        B, K, n = self.B, self.K, self.n
        # oldest-first slot order per env: the ring's next write position is cursor % K
        start = torch.where(self.cursor.long() > K, self.cursor.long() % K, torch.zeros_like(self.cursor.long()))
        order = (start[:, None] + torch.arange(K, device=start.device)[None, :]) % K          # [B, K]
        env = torch.arange(B, device=start.device)[:, None].expand(B, K)
        ok = valid.gather(1, order)
        e, k = env[ok], order[ok]
        bits = self._members(self.acted[e, k])
        rec, agent = torch.nonzero(bits, as_tuple=True)
        T = rec.numel()
        row_of = torch.full((e.numel(), n), -1, dtype=torch.int64, device=start.device)
        row_of[rec, agent] = torch.arange(T, device=start.device)
        ee, kk = e[rec], k[rec]
        idx_col = agent.float()[:, None]
        out = dict(obs=torch.cat([self.obs[ee, kk], idx_col], 1), obs_next_matrix=self.obs_next[ee, kk],
                   act=self.act[ee, kk, agent].long(), rew=self.rew[ee, kk], rew_agent=self.rew[ee, kk, agent],
                   done=self._has(self.done[ee, kk], agent), env_id=ee, agent_id=agent,
                   buffer_id=ee * n + agent, record_slot=kk, episode=self.episode[ee, kk].long(), indices=row_of[rec])
        if self.active_nb is not None:
            out["active_one_hop_neighbors"] = self._members(self.active_nb[ee, kk, agent])
        return {name: t.cpu().numpy() for name, t in out.items()}


class PrioritizedRoundReplay(RoundReplay):
    """:class:`RoundReplay` sampled by priority: the counterpart of [3P] tianshou 1.0.0 ``PrioritizedVectorReplayBuffer(total_size,
    buffer_num, alpha=, beta=)``, which the reference's six scripts switch to with ``--prio-buffer --alpha 0.6 --beta 0.4``
    (common.py:52,64-65, l_dgn.py:169-176).  Parity unpinned: tianshou is restated from its published behaviour.

    One priority per transition (env, slot, acting agent), one sum over the whole buffer: ``prio`` [B, K, N] holds ``p ** alpha``
    (0 for agents that did not act and for slots not yet filled), ``max_prio = min_prio = 1``.

    * a new transition gets ``max_prio ** alpha`` - lazily, by the first ``sample`` that sees its record (``seen`` [B] remembers
      ``cursor`` at the last sample; ``max_prio`` only changes in ``update_weight``, which always follows a ``sample``, so the value
      is the one upstream's ``add`` would have written, and the collect loop's launch stays as it is);
    * ``sample``: ``scalar = u * prio.sum()``, the first transition in buffer order whose inclusive float64 prefix sum exceeds
      it, with replacement; ``weight = (prio[index] / min_prio) ** -beta`` (upstream's simplified form: the numerator is already
      ``p ** alpha``, the denominator the raw ``min_prio``), divided by its maximum over the batch when ``weight_norm``;
    * ``update_weight(batch, td)`` ([3P] ``BasePolicy.post_process_fn`` -> ``update_weight(indices, batch.weight)``): ``p = |td| +
      eps`` in float32, ``prio = p ** alpha``, ``max_prio`` / ``min_prio`` follow ``p``; an index sampled twice keeps the LAST.

    On the GPU these are three launches with no host value in the loop (``mel_replay_sample_prio``: refresh + sample;
    ``mel_replay_update_priority``), so a captured update contains them.  Host tensors take the torch formulation of the same rules
    (float64 cumsum + searchsorted, torch's own random stream)."""

    def __init__(self, n_envs: int, n_nodes: int, capacity: int, device, neighbours: bool = False, alpha: float = 0.6,
                 beta: float = 0.4, weight_norm: bool = True):
        if alpha < 0 or beta < 0:
            raise ValueError(f"alpha={alpha} and beta={beta} must be >= 0")
        super().__init__(n_envs, n_nodes, capacity, device, neighbours=neighbours)
        self.alpha, self.beta, self.weight_norm = float(alpha), float(beta), bool(weight_norm)
        dev = self.obs.device
        self.prio = torch.zeros(n_envs, capacity, n_nodes, dtype=torch.float32, device=dev)
        self.seen = torch.zeros(n_envs, dtype=torch.int32, device=dev)
        self.max_prio = torch.ones(1, dtype=torch.float32, device=dev)
        self.min_prio = torch.ones(1, dtype=torch.float32, device=dev)
        self._rec_sum = torch.zeros(n_envs * capacity, dtype=torch.float64, device=dev)
        self._prio_prefix = torch.zeros(n_envs * capacity + 1, dtype=torch.float64, device=dev)
        p = _lib.MelReplayPriority()
        p.prio, p.rec_sum, p.prefix, p.seen = self.prio.data_ptr(), self._rec_sum.data_ptr(), self._prio_prefix.data_ptr(), self.seen.data_ptr()
        p.max_prio, p.min_prio = self.max_prio.data_ptr(), self.min_prio.data_ptr()
        p.alpha, p.beta, p.weight_norm = self.alpha, self.beta, int(self.weight_norm)
        self.prio_struct = p

    def reset_priorities(self) -> None:
        """Back to the state of construction (the collectors' ``reset_buffer`` calls this with the write cursors)."""
        self.prio.zero_()
        self.seen.zero_()
        self.max_prio.fill_(1.0)
        self.min_prio.fill_(1.0)

    def refresh(self) -> None:
        """Host form of the lazy initialisation (the device does it inside ``sample``): records written since the last sample get
        ``max_prio ** alpha`` for their acting agents, 0 elsewhere.  A slot at or beyond ``min(cursor, K)`` holds no record: it is
        never fresh, whatever ``seen`` says (a cursor that went back marks the whole env written), and its priorities are 0."""
        cur, seen = self.cursor.long(), self.seen.long()
        written = cur - seen
        d = (torch.arange(self.K, device=cur.device)[None, :] - (seen % self.K)[:, None]) % self.K           # [B, K]
        fresh = (written[:, None] >= self.K) | (written[:, None] < 0) | (d < written[:, None])
        init = torch.pow(self.max_prio, self.alpha)                                                        # float32, like powf
        zero = torch.zeros((), device=cur.device)
        new = torch.where(self._members(self.acted), init, zero)
        self.prio.copy_(torch.where(self._valid_slots()[:, :, None], torch.where(fresh[:, :, None], new, self.prio), zero))
        self.seen.copy_(self.cursor)

    def sample(self, batch_size: int, n_step: int, gamma: float, generator: torch.Generator | None = None):
        """:meth:`RoundReplay.sample` by priority; adds ``weight`` [bs] float32."""
        dev = self.obs.device
        if dev.type == "cuda":
            import ctypes as C
            out, b, disc, seed = self._device_batch(batch_size, n_step, gamma, generator)
            out["weight"] = torch.empty(batch_size, device=dev)
            _lib.check(_lib.load().mel_replay_sample_prio(
                C.byref(self.struct), C.byref(self.prio_struct), self.B, self.n, batch_size, n_step, disc, seed,
                self._draws.data_ptr(), C.byref(b), out["weight"].data_ptr(), _lib.current_stream_ptr(dev)), "mel_replay_sample_prio")
            return out
        self.refresh()
        incl = torch.cumsum(self.prio.double().flatten(), 0)
        total = incl[-1]
        if float(total) <= 0:
            raise ValueError("cannot sample from an empty replay: run the collect loop first")
        scalar = torch.rand(batch_size, dtype=torch.float64, device=dev, generator=generator) * total
        idx = torch.searchsorted(incl, scalar, right=True).clamp(max=incl.numel() - 1)
        e, k, agent = idx // (self.K * self.n), (idx // self.n) % self.K, idx % self.n
        out = self._walk_host(e, k, agent, n_step, gamma)
        w = (self.prio[e, k, agent].double() / self.min_prio.double()) ** (-self.beta)
        out["weight"] = (w / w.max() if self.weight_norm else w).float()
        return out

    def update_weight(self, batch: dict, td: torch.Tensor) -> None:
        """``batch``: the ``env`` / ``slot`` / ``agent`` of a sampled batch; ``td``: its TD error [bs] (any sign; a device tensor on the
        GPU: no host synchronisation)."""
        e, k, a = batch["env"], batch["slot"], batch["agent"]
        dev = self.obs.device
        td = td.detach().to(torch.float32).flatten()
        if td.numel() != e.numel():
            raise ValueError(f"update_weight: {td.numel()} TD errors for {e.numel()} samples")
        if dev.type == "cuda":
            import ctypes as C
            td = td.contiguous()
            _lib.check(_lib.load().mel_replay_update_priority(
                C.byref(self.prio_struct), self.B, self.K, self.n, td.numel(), e.data_ptr(), k.data_ptr(), a.data_ptr(),
                td.data_ptr(), _lib.current_stream_ptr(dev)), "mel_replay_update_priority")
            return
        p = td.abs() + torch.finfo(torch.float32).eps
        key = (e * self.K + k) * self.n + a
        uniq, inv = torch.unique(key, return_inverse=True)
        last = torch.zeros_like(uniq).scatter_reduce(0, inv, torch.arange(key.numel()), "amax", include_self=False)
        self.prio.view(-1)[uniq] = torch.pow(p[last], self.alpha)
        self.max_prio.copy_(torch.maximum(self.max_prio, p.max()))
        self.min_prio.copy_(torch.minimum(self.min_prio, p.min()))


class DQNLearner:
    """n-step DQN update over a :class:`RoundReplay` (the learn half of the reference's training loop,
    l_dgn.py:246-261 -> [3P] DQNPolicy.process_fn / learn): target = ret + boot_w * max_a Q_target(boot_obs)
    with the target network evaluated by the HIP forward, then one autograd step (``grad_hook`` = the flat
    RCCL gradient all-reduce of melissa_amd.parallel).  ``fused_td``: the target's argmax / gather / mul / add and the loss with its
    seed gradient are one HIP launch each (``mel_td_target`` / ``mel_td_loss``, :mod:`melissa_amd.td`) instead of torch expressions -
    on device tensors, eagerly and inside a captured update; off by default, so every existing caller keeps its launches."""

    def __init__(self, policy, replay: RoundReplay, batch_size: int = 32, n_step: int = 4, gamma: float = 0.99,
                 grad_hook=None, seed: int = 0, fused_td: bool = False, train_log=None):
        self.policy, self.replay, self.fused_td = policy, replay, bool(fused_td)
        # optional melissa_amd.train_log.TrainLog: every update, eager or captured, launches mel_train_log_update directly in
        # front of the Adam step (behind the gradient hook: it sees the gradient Adam applies)
        self.train_log = train_log
        self.batch_size, self.n_step, self.gamma, self.grad_hook = batch_size, n_step, gamma, grad_hook
        self.gen = torch.Generator(device=replay.obs.device)
        self.gen.manual_seed(seed)
        self.captured = None

    def _returns(self, b: dict) -> torch.Tensor:
        """n-step targets of a sampled batch: ``ret + boot_w * Q_target(boot_obs)[best action]`` [bs]."""
        with torch.no_grad():
            target_net = self.policy.model_old if getattr(self.policy, "_target", False) else self.policy.model
            fwd = (lambda net, o: net.hip_forward(o)) if b["boot_obs"].is_cuda else (lambda net, o: net.torch_forward(o))
            q_next = fwd(target_net, b["boot_obs"])
            online = fwd(self.policy.model, b["boot_obs"]) if self.policy._is_double else None     # double DQN: the online net's argmax
            if self.fused_td and q_next.is_cuda:
                return td_target(q_next, online, b["ret"], b["boot_w"])
            if online is not None:
                best = q_next.gather(1, online.argmax(dim=1, keepdim=True)).squeeze(1)
            else:
                best = q_next.max(dim=1).values
            return b["ret"] + b["boot_w"] * best

    def _policy_kwargs(self) -> dict:
        """What ``policy.learn`` / ``policy.loss_backward`` get on top of the batch (nothing unless ``fused_td``: policies behind
        this learner need not know the switch)."""
        return {"fused_td": True} if self.fused_td else {}

    def sample_batch(self) -> dict:
        """Sample + n-step targets: dict(obs, act, returns) of device tensors, no host synchronisation."""
        b = self.replay.sample(self.batch_size, self.n_step, self.gamma, self.gen)
        returns = self._returns(b)
        # (boot_obs / ret / boot_w: what `returns` was built from - tests recompute it through the target network)
        out = dict(obs=b["obs"], act=b["act"], returns=returns, boot_obs=b["boot_obs"], ret=b["ret"], boot_w=b["boot_w"])
        return self._with_priority_keys(out, b)

    @staticmethod
    def _with_priority_keys(out: dict, b: dict) -> dict:
        """A batch sampled from a :class:`PrioritizedRoundReplay` also carries its importance ``weight`` (the loss uses it) and the
        ``env`` / ``slot`` / ``agent`` its priorities are written back to."""
        if "weight" in b:
            out.update(weight=b["weight"], env=b["env"], slot=b["slot"], agent=b["agent"])
        return out

    def write_back(self, batch: dict) -> None:
        """Prioritized replay only: the TD error ``loss_backward`` left in ``batch`` becomes the sampled transitions' priorities
        ([3P] ``post_process_fn``) - between backward and the optimizer step, eagerly and inside a captured update's graph."""
        if "weight" in batch and hasattr(self.replay, "update_weight"):
            self.replay.update_weight(batch, batch["td_error"])

    def _learn(self, batch: dict) -> dict:
        """``policy.learn`` on a copy of ``batch`` with the priority write-back ahead of the gradient hook; the TD error ends up in
        ``last_batch["td_error"]``."""
        work = dict(batch)
        if self.train_log is not None:
            out = self._learn_logged(work)
            self.last_batch["td_error"] = work["td_error"]
            return out

        def hook(model):
            self.write_back(work)
            if self.grad_hook is not None:
                self.grad_hook(model)

        out = self.policy.learn(work, grad_hook=hook if "weight" in work else self.grad_hook, **self._policy_kwargs())
        if "td_error" in work:
            self.last_batch["td_error"] = work["td_error"]
        return out

    def _learn_logged(self, work: dict) -> dict:
        """``policy.learn`` spelled out, with the training log's launch between the gradient hook and the optimizer step."""
        policy = self.policy
        if policy._target and policy._iter % policy._freq == 0:
            policy.sync_weight()
        loss = policy.loss_backward(work, **self._policy_kwargs())
        self.write_back(work)
        if self.grad_hook is not None:
            self.grad_hook(policy.model)
        self.train_log.launch_update(loss, work["td_error"], policy.optim)
        adam_step(policy.optim)
        policy._iter += 1
        return {"loss": float(loss)}

    def step(self) -> dict:
        if self.captured is not None:
            return self.captured.step()
        self.last_batch = self.sample_batch()                                      # what the update regressed on (tests)
        return self._learn(self.last_batch)

    def capture(self) -> "CapturedUpdate":
        """From now on ``step`` replays the update from HIP graphs (see :class:`CapturedUpdate`)."""
        self.captured = CapturedUpdate(self)
        return self.captured


class CapturedUpdate:
    """One DQN update replayed from HIP graphs instead of issued launch by launch from Python.

    An update is a few hundred small launches (replay sampling, the target forward, forward + backward, Adam) behind
    ~3 ms of Python; the device needs a third of that.  All shapes of a DQN update are static (batch x (8 N + 1)
    observations), so after two eager warm-up updates the whole chain is captured once:

        graph A   sample -> n-step targets (target network, HIP forward) -> zero_grad -> forward -> loss -> backward
                  [-> priority write-back (PrioritizedRoundReplay)] [-> gradients packed into the reducer's flat buffer]
        eager     [one all-reduce of the flat buffer + division: RCCL stays outside the capture]
        graph B   [flat buffer unpacked into the gradients ->] optimizer step

    (one graph when there is no collective).  What stays in Python per update: the target network's periodic weight sync
    and invalidating the networks' per-weight-version caches (prepared bf16 planes / feature tables are keyed on torch's
    parameter version counters, which a replay does not bump).  The optimizer must be a torch optimizer with a
    ``capturable`` flag (Adam / AdamW / ...): it is switched on here and the step counters moved to the device.
    ``step`` returns the loss as a device tensor (``float()`` it to synchronise); ``last_batch`` aliases the graph's static
    tensors (valid until the next replay)."""

    def __init__(self, learner: "DQNLearner", warmup: int = 2):
        self.learner = L = learner
        policy = L.policy
        dev = L.replay.obs.device
        if dev.type != "cuda":
            raise ValueError("CapturedUpdate needs a ROCm / CUDA device")
        opt = policy.optim
        for group in opt.param_groups:
            if "capturable" not in group:
                raise ValueError(f"{type(opt).__name__} has no capturable mode; cannot capture its step")
            group["capturable"] = True
        for st in opt.state.values():
            if "step" in st and torch.is_tensor(st["step"]) and not st["step"].is_cuda:
                st["step"] = st["step"].to(dev)
        hook = L.grad_hook
        self.collective = hook is not None and getattr(hook, "active", lambda: True)()
        if self.collective and not all(hasattr(hook, m) for m in ("pack", "reduce", "unpack")):
            raise ValueError("a captured update needs a grad_hook with pack / reduce / unpack phases (FlatGradAllReducer)")
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):                       # warm-up off the capture stream (lazy inits, optimizer state)
            for _ in range(warmup):
                self._sync_target()
                batch = L.sample_batch()
                warm_loss = policy.loss_backward(batch, **L._policy_kwargs())
                L.write_back(batch)
                if self.collective:
                    hook.pack(), hook.reduce(), hook.unpack()
                self._log_update(warm_loss, batch)
                adam_step(opt)
                policy._iter += 1
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph_a = torch.cuda.CUDAGraph()
        self.graph_a.register_generator_state(L.gen)
        with torch.cuda.graph(self.graph_a):
            self.batch = L.sample_batch()
            self.loss = policy.loss_backward(self.batch, **L._policy_kwargs())
            L.write_back(self.batch)                        # (prioritized replay: the next replay samples by what this one wrote)
            if self.collective:
                hook.pack()
            else:
                self._log_update(self.loss, self.batch)
                adam_step(opt)
        self.graph_b = None
        if self.collective:
            self.graph_b = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool()):
                hook.unpack()
                self._log_update(self.loss, self.batch)     # (behind unpack: the averaged gradient Adam applies)
                adam_step(opt)
        L.last_batch = self.batch

    def _log_update(self, loss, batch):
        if self.learner.train_log is not None:
            self.learner.train_log.launch_update(loss, batch["td_error"], self.learner.policy.optim)

    def _sync_target(self):
        policy = self.learner.policy
        if policy._target and policy._iter % policy._freq == 0:
            policy.sync_weight()
            # the target network only ever runs INSIDE graph A, whose launches read its converted projection weights from the
            # buffer captured with them: reconvert the new weights into that buffer now (no Python runs during a replay)
            policy.model_old.ensure_prepared(self.learner.replay.obs.device)

    def step(self) -> dict:
        policy = self.learner.policy
        self._sync_target()
        if policy._is_double:                  # graph A also evaluates the ONLINE network through the HIP forward
            policy.model.ensure_prepared(self.learner.replay.obs.device)
        self.graph_a.replay()
        if self.collective:
            self.learner.grad_hook.reduce()
            self.graph_b.replay()
        policy._iter += 1
        # the replay changed the parameters behind torch's version counters: mark the per-weight-version caches stale (the
        # prepared planes keep their buffer - launches captured elsewhere hold its address - and are converted again by the
        # next forward)
        policy.model.mark_weights_changed()
        return {"loss": self.loss.clone()}                     # (self.loss is the graph's static tensor: the next replay overwrites it)


class DGNLearner(DQNLearner):
    """DGN-R update (policies/dgn.py): the sampled experiences' n-step returns regress on the summed Q of their
    siblings (policy = :class:`melissa_amd.policy.DGNPolicy`).  All siblings of an experience acted in the same env round and
    so share its observation matrix: the network body runs once per sampled experience and its head once per (experience,
    node) - ``GraphQNetwork.torch_forward_all_agents`` - instead of one whole forward per sibling row (the reference's loop,
    dgn.py:31-55: ~21 siblings per experience at N = 50).  Every tensor of the update then has a static shape, so it replays
    from HIP graphs like the DQN update (``capture()``)."""

    def sample_batch(self) -> dict:
        """Sample + n-step targets in the DENSE form (static shapes, no host synchronisation): obs_matrix [B, 8N], act_all
        [B, N], sibling [B, N] (the agents that acted in the sampled round), returns [B]."""
        return self._dense_batch(self.replay.sample(self.batch_size, self.n_step, self.gamma, self.gen))

    def _dense_batch(self, b: dict) -> dict:
        e, k = b["env"], b["slot"]
        returns = self._returns(b)
        out = dict(obs_matrix=self.replay.obs[e, k], act_all=self.replay.act[e, k].long(),
                   sibling=self.replay._members(self.replay.acted[e, k]), returns=returns, boot_obs=b["boot_obs"], ret=b["ret"],
                   boot_w=b["boot_w"], env=e, slot=k)
        return self._with_priority_keys(out, b)

    def row_form(self, batch: dict) -> dict:
        """The same batch in the reference's row form (what collective_experience_collector.py:70-80 records as ``info.indices``:
        one row per sibling, ordered by experience then agent id): active_obs [M, 8N+1], active_act [M], segment [M].  M depends
        on the data (host synchronisation): for tests and for callers that keep the reference's loss loop."""
        seg, agent = torch.nonzero(batch["sibling"], as_tuple=True)
        obs = torch.cat([batch["obs_matrix"][seg], agent.float()[:, None]], dim=1)
        return dict(active_obs=obs, active_act=batch["act_all"][seg, agent], segment=seg, returns=batch["returns"])

    def step(self) -> dict:
        if self.captured is not None:
            return self.captured.step()
        batch = self.sample_batch()
        self.last_batch = dict(batch, **self.row_form(batch))
        return self._learn(batch)


class NDGNLearner(DGNLearner):
    """N-DGN update (policies/n_dgn.py:22-75, policy = :class:`melissa_amd.policy.NDGNPolicy`): the DGN-R loss with each sampled
    experience's siblings restricted to the agent itself and the one-hop neighbours its next observation reported active
    (``info['active_one_hop_neighbors']``).  Needs a ``RoundReplay(neighbours=True)``; the sampler returns the restricted set
    (``nb_sibling``), so the dense form keeps static shapes and ``capture()`` replays it from HIP graphs.  Targets are DGN-R's:
    ``ret + boot_w * best``.  ``row_form`` (inherited) only when a caller asks for it."""

    def __init__(self, policy, replay: RoundReplay, *args, **kwargs):
        if replay.active_nb is None:
            raise ValueError("NDGNLearner needs a RoundReplay(neighbours=True): N-DGN restricts the siblings to active_nb")
        super().__init__(policy, replay, *args, **kwargs)

    def sample_batch(self) -> dict:
        """Like :meth:`DGNLearner.sample_batch`, with ``sibling`` [B, N] = the restricted set ``nb_sibling``."""
        b = self.replay.sample(self.batch_size, self.n_step, self.gamma, self.gen)
        out = self._dense_batch(b)
        out["sibling"] = self.replay._members(b["nb_sibling"])
        out["agent"] = b["agent"]
        return out

    def step(self) -> dict:
        if self.captured is not None:
            return self.captured.step()
        self.last_batch = self.sample_batch()
        return self._learn(self.last_batch)
