"""The TD target and the TD loss of one update as one HIP launch each (``mel_td_target`` / ``mel_td_loss``, csrc/td.hpp): what the
policies' ``fused_td`` switch runs instead of the torch formulation's ~20 one-line launches.  Device tensors only - there is no
host form: without the switch the policies keep their torch expressions."""
from __future__ import annotations

import torch

from . import _lib


def _f32(t, device=None) -> torch.Tensor:
    """fp32, contiguous, detached, on ``device`` - from whatever ``torch.as_tensor`` takes (numpy arrays and lists too, as the
    torch formulation accepts them for ``returns`` and ``weight``)."""
    return torch.as_tensor(t, device=device).detach().to(torch.float32).contiguous()


def td_target(q_target: torch.Tensor, q_online: torch.Tensor | None, ret: torch.Tensor, boot_w: torch.Tensor) -> torch.Tensor:
    """``ret + boot_w * q_target[i, argmax q_online[i]]`` (double DQN) or ``ret + boot_w * max_a q_target[i, a]`` (``q_online``
    None): the bits of the torch expression in ``DQNLearner.sample_batch``.  [B, A], [B, A] | None, [B], [B] -> [B]."""
    if not q_target.is_cuda:
        raise ValueError("td_target runs on the device (mel_td_target); host tensors take the torch expression")
    q_target = _f32(q_target)
    ret, boot_w = _f32(ret, q_target.device).flatten(), _f32(boot_w, q_target.device).flatten()
    bs, na = q_target.shape
    if q_online is not None:
        q_online = _f32(q_online, q_target.device)
        if q_online.shape != q_target.shape:
            raise ValueError(f"td_target: q_online {tuple(q_online.shape)} != q_target {tuple(q_target.shape)}")
    if ret.numel() != bs or boot_w.numel() != bs:
        raise ValueError(f"td_target: {ret.numel()} returns / {boot_w.numel()} weights for {bs} samples")
    out = torch.empty(bs, dtype=torch.float32, device=q_target.device)
    _lib.check(_lib.load().mel_td_target(q_target.data_ptr(), q_online.data_ptr() if q_online is not None else None,
                                         ret.data_ptr(), boot_w.data_ptr(), bs, na, out.data_ptr(),
                                         _lib.current_stream_ptr(q_target.device)), "mel_td_target")
    return out


def td_loss(q: torch.Tensor, act: torch.Tensor, member: torch.Tensor | None, returns: torch.Tensor,
            weight: torch.Tensor | None = None, huber: bool = False):
    """``q`` [B, A] (DQN: ``member`` None) or [B, N, A] with ``act`` [B, N] int64 and ``member`` [B, N] (the siblings summed over)
    -> (loss [] , td [B], dq like ``q``): ``td = returns - sum_j member_j q[j, act_j]``, ``loss = mean(weight td^2)`` or the Huber
    form (delta 1, weight unused), ``dq = d loss / d q`` with every element written.  Nothing here is recorded by autograd."""
    if not q.is_cuda:
        raise ValueError("td_loss runs on the device (mel_td_loss); host tensors take the torch formulation")
    qf = _f32(q)
    bs, nn, na = (qf.shape[0], 1, qf.shape[1]) if qf.dim() == 2 else tuple(qf.shape)
    dev = qf.device
    act = torch.as_tensor(act, device=dev).detach().to(torch.int64).contiguous()
    returns = _f32(returns, dev).flatten()
    if act.numel() != bs * nn or returns.numel() != bs:
        raise ValueError(f"td_loss: {act.numel()} actions / {returns.numel()} returns for q {tuple(qf.shape)}")
    if member is not None:
        member = _f32(member, dev)
        if member.numel() != bs * nn:
            raise ValueError(f"td_loss: {member.numel()} members for q {tuple(qf.shape)}")
    if weight is not None:
        weight = _f32(weight, dev).flatten()
        if weight.numel() != bs:
            raise ValueError(f"td_loss: {weight.numel()} weights for {bs} samples")
    loss = torch.empty((), dtype=torch.float32, device=dev)
    td = torch.empty(bs, dtype=torch.float32, device=dev)
    dq = torch.empty_like(qf)
    groups = (bs + _lib.TD_GROUP_ROWS - 1) // _lib.TD_GROUP_ROWS
    scratch = torch.empty(groups, dtype=torch.float32, device=dev) if groups > 1 else None
    _lib.check(_lib.load().mel_td_loss(
        qf.data_ptr(), act.data_ptr(), member.data_ptr() if member is not None else None, returns.data_ptr(),
        weight.data_ptr() if weight is not None else None, bs, nn, na, int(bool(huber)), loss.data_ptr(), td.data_ptr(),
        dq.data_ptr(), scratch.data_ptr() if scratch is not None else None, 4 * groups if scratch is not None else 0,
        _lib.current_stream_ptr(dev)), "mel_td_loss")
    return loss, td, dq
