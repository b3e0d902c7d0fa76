"""Full training state of an epoch-mode run (``train(save_state=True)`` / ``train(resume_state=FILE)``, :mod:`melissa_amd.train`):
what a second process needs to continue a run as if it had never stopped - bit for bit, since training is deterministic from
run to run.  NOTES.md "Resuming a run" holds the inventory and the reasons; in short:

* the file is ONE ``torch.save`` of nested dicts of tensors, numbers, strings and lists (``torch.load(..., weights_only=True)``
  reads it), written under a temporary name and moved into place (:func:`write_state_file`);
* ``config`` is a header of everything the state's meaning depends on (:func:`state_header`); :func:`check_state_header`
  compares it with the resuming call's - pure Python, before anything is built;
* every tensor is restored IN PLACE (``copy_`` into the tensor the run already holds): the captured round graph and the
  captured update hold the addresses;
* three things are brought to a canonical form before the copy, because they depend on WHEN the side stream's refill ran and
  not on what the run computed (:func:`gather_state`): the episode stream is topped up, its scratch is left out, and the plan
  masks in the loop's forward workspace are re-derived from the env state after a restore instead of being stored.
"""
from __future__ import annotations

import os
import re
import zlib

FORMAT = 1

# header keys a resuming call must repeat exactly, in the order they are compared (``state_epoch`` and ``format`` are the file's own)
HEADER_KEYS = ("model", "n_nodes", "envs", "world", "rank", "hidden_emb", "num_heads", "dueling_q_hidden_sizes",
               "dueling_v_hidden_sizes", "aggregator_function", "batch_size", "n_step", "gamma", "lr", "target_update_freq",
               "prio_buffer", "alpha", "beta", "heuristic", "scripted_agents_ratio", "epoch", "step_per_epoch", "eps_train",
               "eps_train_final", "exploration_fraction", "update_per_step", "step_per_collect", "replay_rounds",
               "rounds_per_update", "ring", "seed", "captured", "collect_stats", "pool_graphs", "pool_checksum", "mel_version")
# header keys only a run with the feature on carries (a file without the feature has exactly HEADER_KEYS): compared both ways
OPTIONAL_HEADER_KEYS = ("log_interval",)


class StateMismatch(ValueError):
    """The state file belongs to another run than the one the resuming call describes."""


def check_resume_args(epoch=None, save_state=False, stop_after_epoch=None, resume_state=None, resume_path=None) -> None:
    """ValueError for a combination of the three state arguments that means nothing (no torch, nothing built)."""
    if resume_state is not None and epoch is None:
        raise ValueError("resume_state continues an epoch-mode run: it needs epoch (the run's total)")
    if resume_state is not None and resume_path is not None:
        raise ValueError("resume_state and resume_path are mutually exclusive: the state file holds the weights")
    if save_state and epoch is None:
        raise ValueError("save_state writes the state after every epoch: it needs epoch")
    if stop_after_epoch is not None:
        if epoch is None:
            raise ValueError("stop_after_epoch ends an epoch-mode run early: it needs epoch (the run's total)")
        if not 1 <= int(stop_after_epoch) <= int(epoch):
            raise ValueError(f"stop_after_epoch={stop_after_epoch} must be between 1 and epoch={epoch}")


def state_header(**values) -> dict:
    """The header of a run: exactly :data:`HEADER_KEYS`, as plain numbers / strings / lists (``pool_graphs`` and
    ``pool_checksum`` may be left out until the training pool exists: :func:`pool_identity`)."""
    unknown = set(values) - set(HEADER_KEYS) - set(OPTIONAL_HEADER_KEYS)
    if unknown:
        raise KeyError(f"not header keys: {sorted(unknown)}")
    out = {}
    for key in HEADER_KEYS + OPTIONAL_HEADER_KEYS:
        if key not in values:
            continue
        v = values[key]
        if isinstance(v, (list, tuple)):
            v = [int(x) for x in v]
        elif isinstance(v, bool) or v is None or isinstance(v, str):
            pass
        elif isinstance(v, int):
            v = int(v)
        else:
            v = float(v)
        out[key] = v
    return out


def pool_identity(graph_list) -> dict:
    """What identifies a training-graph pool: its graph count and the CRC-32 of the float64 node positions, in pool order (the
    bytes of the episode stream's ``graph_pos``)."""
    import numpy as np
    pos = np.ascontiguousarray(np.stack([g.pos for g in graph_list]).astype(np.float64))
    return dict(pool_graphs=len(graph_list), pool_checksum=int(zlib.crc32(pos.tobytes())))


def check_state_header(saved: dict, wanted: dict, path: str = "the state file") -> None:
    """:class:`StateMismatch` naming the first key of ``wanted`` (the resuming call's :func:`state_header`, whole or in part)
    that ``saved`` (a file's ``config``) holds another value for, with both values; then the epochs: a state taken after epoch
    ``state_epoch`` continues a run of MORE epochs than that.  No device, no torch."""
    for key in HEADER_KEYS:
        if key not in wanted:
            continue
        if key not in saved:
            raise StateMismatch(f"{path} has no {key} in its header (this call: {key}={wanted[key]!r})")
        if saved[key] != wanted[key]:
            raise StateMismatch(f"{path} was written by a run with {key}={saved[key]!r}; this call has {key}={wanted[key]!r}")
    for key in OPTIONAL_HEADER_KEYS:
        if "epoch" in wanted and saved.get(key) != wanted.get(key):
            raise StateMismatch(f"{path} was written by a run with {key}={saved.get(key)!r}; this call has {key}={wanted.get(key)!r}")
    if "epoch" in wanted and int(saved.get("state_epoch", -1)) >= int(wanted["epoch"]):
        raise StateMismatch(f"{path} holds the state after epoch {saved.get('state_epoch')}: nothing is left of a run of "
                            f"epoch={wanted['epoch']}")


def rank_state_path(path: str, rank: int, world: int) -> str:
    """``X_state.pth`` for a single process, ``X_state.rank<r>.pth`` for rank r of several; a name that already carries a
    ``.rank<k>`` (another rank's file, given to ``--resume-state``) is taken for its run's."""
    root, ext = os.path.splitext(path)
    root = re.sub(r"\.rank\d+$", "", root)
    return f"{root}.rank{int(rank)}{ext}" if int(world) > 1 else f"{root}{ext}"


def write_state_file(state: dict, path: str) -> None:
    """``torch.save`` under a temporary name in the same directory, then ``os.replace``: a process killed (or a write that
    fails) on the way leaves the previous file as it was, and no temporary file behind when the failure is an exception."""
    import torch
    tmp = f"{path}.tmp{os.getpid()}"
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def load_state_file(path: str) -> dict:
    """The file as host tensors, memory-mapped: the header is there at once, a tensor is read when it is copied."""
    import torch
    return torch.load(path, map_location="cpu", weights_only=True, mmap=True)


# ---------------------------------------------------------------------------------------------------------------- the inventory
# name -> attribute, per object; an attribute that is None or absent (a feature that is off) is left out of the file
_REPLAY = ("obs", "obs_next", "acted", "done", "act", "rew", "episode", "cursor", "active_nb", "_draws",
           "prio", "seen", "max_prio", "min_prio")
_LOOP = ("rounds", "_eps_dev", "_env_step_dev", "_trace_env_step", "_trace_eps", "live", "offsets")
_VENV = ("state", "log_cursor", "log_stats", "log_meta", "step_stats")
# (``work`` and ``new_count`` are the refill's scratch: written by its first launch and read by its later ones, stream ordered)
_STREAM = ("pcg", "pcg_half", "produced", "draw_seed", "draw_graph", "draw_scripted")


def _tensors(obj, names) -> dict:
    import torch
    return {n: getattr(obj, n).detach().cpu() for n in names if torch.is_tensor(getattr(obj, n, None))}


def _plain(v):
    """Python numbers for NumPy's (``weights_only`` loads no NumPy scalar)."""
    import numpy as np
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


def _optim_to_host(sd: dict) -> dict:
    import torch
    state = {i: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in sd["state"].items()}
    return dict(state=state, param_groups=_plain(sd["param_groups"]))


def quiesce(loop, device) -> None:
    """Nothing in flight, and the episode stream in the one state that does not depend on when its refills ran: the side
    stream drained, then every env's ring topped up from its cursor (``produced = cursor + ring - 1`` whatever it was).  A
    paced refill reads the cursors when its gate opens - a round or two later in one process than in another - so without
    this ``produced``, the generators and the ring's newest slots differ between two runs of the same trajectory."""
    import torch
    torch.cuda.synchronize(device)
    supply = loop.supply
    side = getattr(supply, "side", None)
    if side is not None:
        side.synchronize()
    if hasattr(supply, "refill"):
        supply.refill()
    torch.cuda.synchronize(device)


def gather_state(config: dict, run: dict, policy, learner, replay, loop, venv, device, train_log=None) -> dict:
    """Host copy of the whole training state (see the module docstring); ``config``: the header with ``state_epoch``,
    ``run``: the epoch loop's own numbers and records; ``train_log``: the run's training log, whose ring and drain position
    the state then holds (key ``train_log``; absent without one)."""
    import torch
    quiesce(loop, device)
    replay.sampler_scratch()                                 # (an eager run that has not sampled yet: the draw counter, at 0)
    supply = loop.supply
    stream = _tensors(supply, _STREAM)
    stream["refills"] = int(getattr(supply, "refills", 0))
    pool = getattr(supply, "pool", None)
    if pool is not None and hasattr(supply, "refill"):       # the ring and its reset snapshots (a static table never changes)
        stream["pool"] = {k: v.detach().cpu() for k, v in pool.tensors.items()}
        if pool.snapshot_state is not None:
            stream["snapshot_state"] = pool.snapshot_state.cpu()
    more = {} if train_log is None else {"train_log": train_log.state()}
    return dict(
        **more, format=FORMAT, config=_plain(dict(config)), run=_plain(dict(run)),
        policy=dict(state_dict={k: v.detach().cpu() for k, v in policy.state_dict().items()}, iter=int(policy._iter),
                    optim=_optim_to_host(policy.optim.state_dict())),
        learner=dict(gen=learner.gen.get_state().cpu()),
        rng=dict(cpu=torch.get_rng_state(), cuda=torch.cuda.get_rng_state(device).cpu()),
        replay=_tensors(replay, _REPLAY),
        loop=dict(_tensors(loop, _LOOP), iterations=int(loop.iterations), rounds_base=int(loop._rounds_base)),
        venv=_tensors(venv, _VENV), stream=stream)


def _put(dst, src, what: str) -> None:
    if tuple(dst.shape) != tuple(src.shape) or dst.dtype != src.dtype:
        raise ValueError(f"state file: {what} is {tuple(src.shape)} {src.dtype}, the run built here holds "
                         f"{tuple(dst.shape)} {dst.dtype}")
    dst.copy_(src)


def _put_all(obj, names, saved: dict, what: str) -> None:
    import torch
    have = [n for n in names if torch.is_tensor(getattr(obj, n, None))]
    if set(have) != set(saved) - {"refills", "pool", "snapshot_state", "iterations", "rounds_base"}:
        raise ValueError(f"state file: {what} holds {sorted(saved)}, the run built here {sorted(have)}")
    for n in have:
        _put(getattr(obj, n), saved[n], f"{what}.{n}")


def _restore_optim(opt, saved: dict) -> None:
    """Adam's moments and step counters into the tensors the optimizer holds (a captured step has their addresses); an
    optimizer that has not stepped yet (the eager path takes no warm-up update) gets them from ``load_state_dict``."""
    import torch
    params = [p for group in opt.param_groups for p in group["params"]]
    if not opt.state:
        if saved["state"]:
            opt.load_state_dict(saved)
        return
    if set(saved["state"]) != {i for i, p in enumerate(params) if p in opt.state}:
        raise ValueError("state file: the optimizer state covers other parameters than the optimizer built here")
    for i, st in saved["state"].items():
        own = opt.state[params[i]]
        for k, v in st.items():
            if torch.is_tensor(v) and torch.is_tensor(own.get(k)):
                if tuple(own[k].shape) != tuple(v.shape):
                    raise ValueError(f"state file: optimizer state {k} of parameter {i} is {tuple(v.shape)}, here {tuple(own[k].shape)}")
                own[k].copy_(v)
            else:
                own[k] = v


def restore_state(state: dict, policy, learner, replay, loop, venv, device, train_log=None) -> dict:
    """Overwrite the run built here with ``state`` (a loaded file), in place; -> its ``run`` part.  The caller has built the run
    as a fresh one would be, played the pre-fill rounds and captured the update, so every lazily created tensor and graph
    exists; what those steps did is overwritten."""
    import torch
    if int(state.get("format", -1)) != FORMAT:
        raise ValueError(f"state file format {state.get('format')!r}: this version reads format {FORMAT}")
    quiesce(loop, device)
    with torch.no_grad():
        own = policy.state_dict()
        if set(own) != set(state["policy"]["state_dict"]):
            raise ValueError("state file: the policy's state_dict has other keys than the policy built here")
        for k, v in state["policy"]["state_dict"].items():
            _put(own[k], v, f"policy.{k}")
        policy._iter = int(state["policy"]["iter"])
        _restore_optim(policy.optim, state["policy"]["optim"])
        learner.gen.set_state(state["learner"]["gen"].clone())
        torch.set_rng_state(state["rng"]["cpu"].clone())
        torch.cuda.set_rng_state(state["rng"]["cuda"].clone(), device)
        replay.sampler_scratch()                             # (the eager path has not sampled yet: the draw counter exists now)
        _put_all(replay, _REPLAY, state["replay"], "replay")
        _put_all(loop, _LOOP, state["loop"], "loop")
        loop.iterations, loop._rounds_base = int(state["loop"]["iterations"]), int(state["loop"]["rounds_base"])
        _put_all(venv, _VENV, state["venv"], "venv")
        if (train_log is None) != ("train_log" not in state):
            raise ValueError("state file: it " + ("holds" if "train_log" in state else "has no") + " training log, the run built "
                             "here " + ("has none" if train_log is None else "has one"))
        if train_log is not None:
            train_log.load_state(state["train_log"])
        supply, saved = loop.supply, state["stream"]
        _put_all(supply, _STREAM, saved, "stream")
        if hasattr(supply, "refills"):
            supply.refills = int(saved["refills"])
        if "pool" in saved:
            if set(saved["pool"]) != set(supply.pool.tensors):
                raise ValueError("state file: the episode ring holds other arrays than the ring built here")
            for k, v in saved["pool"].items():
                _put(supply.pool.tensors[k], v, f"stream.pool.{k}")
            if "snapshot_state" in saved:
                _put(supply.pool.snapshot_state, saved["snapshot_state"], "stream.snapshot_state")
        # the next forward reads its plan masks from the loop's workspace, where the LAST round's env launch left them: they
        # are a function of the env state just restored, and the launch that publishes the first round's active sets writes
        # them again (it plays nothing and counts nothing)
        loop._bind_plan()
        venv.round_device(loop.pool, None, None, loop.live, None, first=True)
    # prepared planes and feature tables are keyed on torch's version counters: stale now, whatever the counters say; the
    # target network's are only ever refreshed at a sync, so bring them up to date here
    policy.model.mark_weights_changed()
    policy.model.ensure_prepared(device)
    if getattr(policy, "_target", False):
        policy.model_old.mark_weights_changed()
        policy.model_old.ensure_prepared(device)
    torch.cuda.synchronize(device)
    return state["run"]
