"""mel_td_target / mel_td_loss (csrc/td.hpp) against a float64 numpy evaluation of their formulas on the same fp32 inputs, and the
policies' ``fused_td`` switch against their torch formulation on one sampled batch."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                                                   # unit roundoff of fp32


def reference(q, act, member, returns, weight, huber):
    """float64: (loss, td [B], dq [B, N, A], sum_j |member q_sel| [B]) of q [B, N, A], act [B, N], member [B, N] | None."""
    B, N, A = q.shape
    q_sel = np.take_along_axis(q.astype(np.float64), act[..., None], 2)[..., 0]
    m = np.ones((B, N)) if member is None else member.astype(np.float64)
    batch_q = (m * q_sel).sum(1)
    td = returns.astype(np.float64) - batch_q
    w = np.ones(B) if weight is None else weight.astype(np.float64)
    if huber:
        z = np.abs(td)
        terms, g = np.where(z < 1.0, 0.5 * td * td, z - 0.5), np.where(z < 1.0, -td, -np.sign(td))
    else:
        terms, g = w * td * td, -2.0 * w * td
    dq = np.zeros((B, N, A))
    np.put_along_axis(dq, act[..., None], (m * (g / B)[:, None])[..., None], 2)
    dq[m == 0] = 0.0
    return terms.mean(), td, dq, np.abs(m * q_sel).sum(1)


def launch(q, act, member, returns, weight, huber, scratch_floats=None):
    """numpy in, one mel_td_loss call, numpy out: status, loss (0-d float32), td, dq."""
    from melissa_amd import _lib
    B, N, A = q.shape
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tq, ta, tm, tr, tw = dev(q), dev(act), dev(member), dev(returns), dev(weight)
    loss = torch.full((1,), np.nan, dtype=torch.float32, device="cuda")
    td = torch.full((B,), np.nan, dtype=torch.float32, device="cuda")
    dq = torch.full((B, N, A), np.nan, dtype=torch.float32, device="cuda")          # (every element must be written)
    groups = (B + _lib.TD_GROUP_ROWS - 1) // _lib.TD_GROUP_ROWS
    n_scratch = groups if scratch_floats is None else scratch_floats
    scratch = torch.zeros(max(1, n_scratch), dtype=torch.float32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    st = _lib.load().mel_td_loss(ptr(tq), ptr(ta), ptr(tm), ptr(tr), ptr(tw), B, N, A, int(huber), ptr(loss), ptr(td), ptr(dq),
                                 scratch.data_ptr(), 4 * n_scratch, _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return st, loss.cpu().numpy()[0], td.cpu().numpy(), dq.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def as_f32_exactly(x64):
    x32 = np.asarray(x64, dtype=np.float32)
    assert np.array_equal(x32.astype(np.float64), np.asarray(x64)), "the reference itself is not an fp32 value"
    return x32


@pytest.mark.parametrize("huber", [False, True], ids=["mse", "huber"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("N", [1, 12, 70, 128])
def test_exact_inputs_give_the_float64_result_bit_for_bit(N, weighted, huber):
    """q multiples of 1/8 in [-2, 2], at most 16 members per row, returns multiples of 1/8 in [-8, 8], weights in {1/4 .. 1}: every
    intermediate is an fp32 value whatever the order of the sums, so loss, td and dq ARE the float64 reference."""
    from melissa_amd import _lib
    B, A = 32, 2
    rng = np.random.RandomState(1000 * N + 10 * weighted + huber)
    q = (rng.randint(-16, 17, size=(B, N, A)) / 8.0).astype(np.float32)
    act = rng.randint(0, A, size=(B, N)).astype(np.int64)
    member = np.zeros((B, N), dtype=np.float32)
    for i in range(B):
        member[i, rng.choice(N, size=rng.randint(0, min(N, 16) + 1), replace=False)] = 1.0
    if N == 1:
        member = None                                            # the DQN form
    returns = (rng.randint(-64, 65, size=B) / 8.0).astype(np.float32)
    weight = rng.choice([0.25, 0.5, 0.75, 1.0], size=B).astype(np.float32) if weighted else None
    st, loss, td, dq = launch(q, act, member, returns, weight, huber)
    assert st == _lib.OK
    want_loss, want_td, want_dq, _ = reference(q, act, member, returns, weight, huber)
    assert np.array_equal(bits(td), bits(as_f32_exactly(want_td)))
    assert np.array_equal(bits(dq), bits(as_f32_exactly(want_dq)))
    assert bits(loss) == bits(as_f32_exactly(want_loss)), (loss, want_loss)
    assert np.count_nonzero(dq) > 0 and np.abs(want_td).max() > 1.0               # (both Huber branches, real gradients)


def normal_case(B, N, A, seed, weighted, empty_row=False):
    rng = np.random.RandomState(seed)
    q = rng.standard_normal((B, N, A)).astype(np.float32)
    act = rng.randint(0, A, size=(B, N)).astype(np.int64)
    member = None if N == 1 else (rng.uniform(size=(B, N)) < 0.5).astype(np.float32)
    if empty_row:
        member[B // 2] = 0.0
    returns = (3.0 * rng.standard_normal(B)).astype(np.float32)
    weight = rng.uniform(0.2, 1.0, size=B).astype(np.float32) if weighted else None
    return q, act, member, returns, weight


GENERAL = [(1, 1, 2), (33, 1, 2), (4096, 1, 2), (33, 20, 2), (1024, 70, 2), (130, 20, 5)]


@pytest.mark.parametrize("mode", ["mse", "weighted", "huber"])
@pytest.mark.parametrize("B,N,A", GENERAL)
def test_normal_inputs_stay_within_the_rounding_bounds(B, N, A, mode):
    """Bounds (u = 2^-24), reference = float64 numpy on the same fp32 inputs:
      td     |td - ref| <= (N + 2) u (|returns_i| + sum_j |q_sel|)
      loss   relative (B + 2 N + 8) u: a sum of B non-negative terms of at most three roundings each, plus the sibling sums
      dq     non-zero entries within a relative 4 u of the formula -2 weight_i td_i / B (its Huber form) evaluated in float64 on
             the td the launch returned - td_i is an output with its own bound above, and a TD error that nearly cancels has no
             relative accuracy to hand on - and, where td is a single subtraction (N = 1), of the pure float64 reference too
      the zeros of dq are exact, and they are where the reference has them."""
    from melissa_amd import _lib
    huber, weighted = mode == "huber", mode == "weighted"
    q, act, member, returns, weight = normal_case(B, N, A, seed=B + 7 * N + A, weighted=weighted)
    st, loss, td, dq = launch(q, act, member, returns, weight, huber)
    assert st == _lib.OK
    want_loss, want_td, want_dq, mass = reference(q, act, member, returns, weight, huber)
    td_err, td_bound = np.abs(td - want_td), (N + 2) * U * (np.abs(returns.astype(np.float64)) + mass)
    loss_err = abs(float(loss) - want_loss) / want_loss
    print(f"B {B} N {N} A {A} {mode}: td err / bound max {np.max(td_err / np.maximum(td_bound, 1e-300)):.3f}  "
          f"loss rel err {loss_err:.3e} bound {(B + 2 * N + 8) * U:.3e}")
    assert (td_err <= td_bound).all()
    assert loss_err <= (B + 2 * N + 8) * U
    # dq: the formula on the returned td
    w = np.ones(B) if weight is None else weight.astype(np.float64)
    t = td.astype(np.float64)
    g = np.where(np.abs(t) < 1.0, -t, -np.sign(t)) if huber else -2.0 * w * t
    m = np.ones((B, N)) if member is None else member.astype(np.float64)
    from_td = np.zeros((B, N, A))
    np.put_along_axis(from_td, act[..., None], (m * (g / B)[:, None])[..., None], 2)
    nz = from_td != 0
    assert np.array_equal(nz, want_dq != 0) and np.array_equal(dq != 0, nz)
    assert np.array_equal(bits(dq[~nz]), np.zeros(int((~nz).sum()), np.uint32))   # exact zeros (+0), all of them written
    rel = np.abs(dq[nz] - from_td[nz]) / np.abs(from_td[nz])
    print(f"    dq rel err max {rel.max():.3e} (of the formula on the returned td), bound {4 * U:.3e}")
    assert rel.max() <= 4 * U
    if N == 1:
        rel = np.abs(dq[nz] - want_dq[nz]) / np.abs(want_dq[nz])
        print(f"    dq rel err max {rel.max():.3e} (of the float64 reference)")
        assert rel.max() <= 4 * U


@pytest.mark.parametrize("B,N,A", [(4096, 1, 2), (1024, 70, 2)])
def test_two_calls_give_identical_bits(B, N, A):
    case = normal_case(B, N, A, seed=5, weighted=True)
    first, second = launch(*case, False), launch(*case, False)
    for x, y in zip(first[1:], second[1:]):
        assert np.array_equal(bits(x), bits(y))


def test_a_row_without_members_has_zero_q_and_gradient():
    B, N, A = 33, 20, 2
    q, act, member, returns, weight = normal_case(B, N, A, seed=3, weighted=False, empty_row=True)
    st, loss, td, dq = launch(q, act, member, returns, weight, False)
    assert st == 0 and not member[B // 2].any()
    assert bits(td[B // 2]) == bits(returns[B // 2])             # batch_q = 0: td is the return itself
    assert np.array_equal(bits(dq[B // 2]), np.zeros((N, A), np.uint32))
    assert np.count_nonzero(dq) == int(member.sum())


def launch_target(q_target, q_online, ret, boot_w):
    from melissa_amd import _lib
    B, A = q_target.shape
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    tt, to, tr, tb = dev(q_target), dev(q_online), dev(ret), dev(boot_w)
    out = torch.full((B,), np.nan, dtype=torch.float32, device="cuda")
    st = _lib.load().mel_td_target(tt.data_ptr(), None if to is None else to.data_ptr(), tr.data_ptr(), tb.data_ptr(), B, A,
                                   out.data_ptr(), _lib.current_stream_ptr())
    torch.cuda.synchronize()
    return st, out.cpu().numpy()


@pytest.mark.parametrize("double", [True, False], ids=["double", "plain"])
@pytest.mark.parametrize("A", [2, 5])
@pytest.mark.parametrize("B", [1, 33, 4096])
def test_td_target_is_numpy_bit_for_bit(B, A, double):
    rng = np.random.RandomState(B + A)
    q_target = rng.standard_normal((B, A)).astype(np.float32)
    # the online values come from a few levels only: many rows have tied maxima, which np.argmax resolves to the first
    q_online = rng.randint(0, 3, size=(B, A)).astype(np.float32) if double else None
    ret = rng.standard_normal(B).astype(np.float32)
    boot_w = np.where(rng.uniform(size=B) < 0.3, 0.0, 0.99 ** rng.randint(1, 5, size=B)).astype(np.float32)
    boot_w[0] = 0.0 if B > 1 else boot_w[0]
    st, got = launch_target(q_target, q_online, ret, boot_w)
    assert st == 0
    best = q_target[np.arange(B), np.argmax(q_online, axis=1)] if double else q_target.max(axis=1)
    want = ret + boot_w * best                                   # float32 numpy: the product, then the sum, each rounded
    assert want.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    if double and B > 1:
        top = q_online.max(axis=1, keepdims=True)
        assert ((q_online == top).sum(axis=1) > 1).any()         # ties did occur
        assert (boot_w == 0).any() and np.array_equal(got[boot_w == 0], ret[boot_w == 0])


def test_td_target_propagates_nan_like_numpy():
    """A NaN among the target values is the plain-DQN maximum (np.max, torch.max), a NaN among the online values is the double-DQN
    argmax - the first one (np.argmax, torch.argmax): a diverged network is not masked."""
    nan = np.float32(np.nan)
    q_target = np.array([[1, nan, 3], [nan, 2, 1], [1, 2, nan], [3, 1, 2]], np.float32)
    ret, boot_w = np.zeros(4, np.float32), np.ones(4, np.float32)
    st, got = launch_target(q_target, None, ret, boot_w)
    assert st == 0 and np.array_equal(np.isnan(got), [True, True, True, False]) and got[3] == 3
    q_online = np.array([[5, nan, 9], [nan, nan, 1], [1, 9, nan], [1, 7, 7]], np.float32)
    values = np.array([[10, 20, 30]] * 4, np.float32)
    st, got = launch_target(values, q_online, ret, boot_w)
    assert st == 0 and np.array_equal(got, values[np.arange(4), np.argmax(q_online, axis=1)])
    assert np.array_equal(got, [20, 10, 30, 20])


def test_td_loss_takes_what_as_tensor_takes():
    """``returns`` and ``weight`` as numpy arrays, as the torch formulation accepts them: same bits as with device tensors."""
    from melissa_amd.td import td_loss
    q, act, member, returns, weight = normal_case(33, 1, 2, seed=11, weighted=True)
    qd, ad = torch.from_numpy(q[:, 0]).cuda(), torch.from_numpy(act[:, 0]).cuda()
    first = td_loss(qd, ad, None, torch.from_numpy(returns).cuda(), torch.from_numpy(weight).cuda())
    second = td_loss(qd, ad, None, returns, weight)
    for x, y in zip(first, second):
        assert np.array_equal(bits(x.cpu().numpy()), bits(y.cpu().numpy()))


def test_argument_errors():
    from melissa_amd import _lib
    case = lambda B, N, A: (np.zeros((B, N, A), np.float32), np.zeros((B, N), np.int64), None, np.zeros(B, np.float32), None)
    assert launch(*case(4, 1, 9), False)[0] == _lib.ERR_INVALID_ARG and b"n_actions" in _lib.load().mel_last_error()
    assert launch(*case(4, 129, 2), False)[0] == _lib.ERR_INVALID_ARG
    assert launch(*case(65, 1, 2), False, scratch_floats=1)[0] == _lib.ERR_WORKSPACE     # two workgroups, room for one sum
    assert launch(*case(65, 1, 2), False, scratch_floats=2)[0] == _lib.OK
    assert launch(*case(64, 1, 2), False, scratch_floats=0)[0] == _lib.OK                # one workgroup needs none
    assert launch_target(np.zeros((4, 9), np.float32), None, np.zeros(4, np.float32), np.zeros(4, np.float32))[0] == _lib.ERR_INVALID_ARG
    from melissa_amd.td import td_loss
    with pytest.raises(ValueError, match="device"):
        td_loss(torch.zeros(4, 2), torch.zeros(4, dtype=torch.int64), None, torch.zeros(4))


# ---- through the policies -------------------------------------------------------------------------------------------------------

def _filled(model, n, envs=16, rounds=12):
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.replay import RoundReplay
    from melissa_amd.train import build_network, policy_and_learner
    torch.manual_seed(3)
    net = build_network(model, n, "cuda")
    policy_cls, learner_cls, neighbours = policy_and_learner(model)
    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 8, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=5, construct_like_reference=False)
    replay = RoundReplay(envs, n, 16, "cuda", neighbours=neighbours)
    policy = policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=3)
    loop = RoundLoop(venv, policy, seed=5, eps=0.2, replay=replay)
    with torch.no_grad():
        loop.run(rounds)
    torch.cuda.synchronize()
    assert loop.counters()["errors"] == 0
    return net, policy, learner_cls, replay


@pytest.mark.parametrize("model,n,weighted", [("l_dgn", 12, False), ("dgn_r", 20, False), ("n_dgn_r", 20, False),
                                              ("l_dgn", 12, True), ("dgn_r", 20, True)])
def test_fused_td_through_the_policies(model, n, weighted):
    """One sampled batch, ``loss_backward`` with and without ``fused_td``: same target bits, same TD error (bit-equal for DQN, whose
    td is one subtraction either way), every parameter gradient within 2e-4 max|g| + 1e-7 (the project's HIP-vs-oracle gradient
    bound, tests/test_gpu_grad.py)."""
    net, policy, learner_cls, replay = _filled(model, n)
    plain = learner_cls(policy, replay, batch_size=16, n_step=4, gamma=0.99, seed=2)
    fused = learner_cls(policy, replay, batch_size=16, n_step=4, gamma=0.99, seed=2, fused_td=True)
    assert plain.fused_td is False and fused.fused_td is True
    sampled = replay.sample(16, 4, 0.99, plain.gen)
    assert np.array_equal(bits(plain._returns(sampled).cpu().numpy()), bits(fused._returns(sampled).cpu().numpy()))
    batch = plain.sample_batch()
    if weighted:
        batch["weight"] = torch.from_numpy(np.random.RandomState(1).uniform(0.2, 1.0, size=16).astype(np.float32)).cuda()
    results = {}
    for switch in (False, True):
        work = dict(batch)
        loss = policy.loss_backward(work, fused_td=switch)
        torch.cuda.synchronize()
        results[switch] = (float(loss), work["td_error"].cpu().numpy(),
                           {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters() if p.grad is not None})
    (loss_t, td_t, grad_t), (loss_f, td_f, grad_f) = results[False], results[True]
    assert td_t.shape == td_f.shape == (16,) and np.abs(td_t).max() > 0
    # both formulations against float64 on the q values of this batch (the learn path's own forward), within the kernel's bounds
    with torch.enable_grad():
        if model == "l_dgn":
            q = policy.model(batch["obs"])[0].detach().cpu().numpy()[:, None, :]
            act, member, nn = batch["act"].cpu().numpy()[:, None], None, 1
        else:
            q = policy.model.torch_forward_all_agents(batch["obs_matrix"]).detach().cpu().numpy()
            act, member, nn = batch["act_all"].cpu().numpy(), batch["sibling"].float().cpu().numpy(), n
    weight = batch["weight"].cpu().numpy() if weighted else None
    returns = batch["returns"].cpu().numpy()
    want_loss, want_td, _, mass = reference(q, act, member, returns, weight, False)
    td_bound = (nn + 2) * U * (np.abs(returns.astype(np.float64)) + mass)
    for td, loss in ((td_t, loss_t), (td_f, loss_f)):
        assert (np.abs(td - want_td) <= td_bound).all()
        assert abs(loss - want_loss) <= (16 + 2 * nn + 8) * U * want_loss
    if model == "l_dgn":
        assert np.array_equal(bits(td_t), bits(td_f))
    assert set(grad_t) == set(grad_f) and len(grad_t) > 10
    worst = worst_rel = 0.0
    for k, g in grad_t.items():
        err, scale = float((grad_f[k] - g).abs().max()), float(g.abs().max())
        worst, worst_rel = max(worst, err / (2e-4 * scale + 1e-7)), max(worst_rel, err / max(scale, 1e-30))
        assert err <= 2e-4 * scale + 1e-7, (k, err, scale)
    print(f"{model} N {n} weighted {weighted}: loss {loss_t!r} / {loss_f!r}, largest gradient difference {worst:.3e} of its bound "
          f"({worst_rel:.3e} of the tensor's largest entry)")
