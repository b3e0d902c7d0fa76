"""GPU tests of head counts that do not fill a wavefront (6 heads: 8 lanes per head, 48 live lanes of 64, 16 idle) and of the
--hidden-emb / --num-heads shapes of train / watch.

hidden / heads (64, 6) and (128, 6): 8 and 16 channels per lane.  Nodes 20 (one set word), 70 (two words: the 16-wave pool
launch), 7 (fewer nodes than a step's sources fill); batches of 3 rows (fewer than a workgroup's four waves), 2048 envs once
for the 4-wave pool launch.  Bars: 1e-4 absolute on logits against oracle.net_oracle; gradients
2e-4 x max|grad| + 1e-7 per tensor (tests/test_gpu_grad.py); bf16 rows: tests/test_gpu_bf16.py's 2e-2."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PARENT_GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "head_shapes_parent.npz")
PARENT_CASES = [("l_dgn", "max"), ("dgn_r", "max"), ("hl_dgn", "max"), ("hl_dgn", "mean"), ("hl_dgn", "add")]
MODELS = PARENT_CASES
SHAPES = [(64, 6), (128, 6)]
SIZES = [(20, 3), (70, 3), (7, 3)]
TOL = 1e-4
# (hidden, heads) -> does the HIP path run it (tests/test_head_shapes.py holds the Python rule to the same table)
SHAPE_TABLE = {(64, 2): True, (64, 4): True, (128, 2): True, (128, 4): True, (256, 2): True, (256, 4): True, (512, 2): True,
               (64, 6): True, (128, 6): True,
               (64, 8): True, (64, 16): True, (128, 1): True, (128, 8): True, (256, 1): True, (512, 1): True,
               (16, 2): False, (16, 4): False, (16, 6): False, (32, 2): False, (32, 4): False, (32, 6): False,
               (512, 4): False, (256, 6): False}


def duel():
    return ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


def random_obs(n, bs, seed):
    """As tests/test_gpu_grad.py::random_obs."""
    rng = np.random.RandomState(seed)
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, 9, size=(bs, n))
    m[:, :, 3] = rng.randint(0, 4, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.2)
    obs[:, -1] = rng.randint(0, n, size=bs)
    return obs


def parent_case_logits(model, agg):
    """(128 hidden, 4 heads), n = 20, bs = 3: the logits tests/golden/head_shapes_parent.npz holds from the parent commit."""
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    n = 20
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    net = cls(5, 128, 2, 4, n, dueling_param=duel(), device="cuda", backend="hip", **kw)
    net.load_state_dict(no.init_weights(model, seed=17, random_conv_bias=True))
    with torch.no_grad():
        return net(random_obs(n, 3, 41))[0].cpu().numpy()


def make_net(model, n, hidden, heads, agg="max", backend="hip"):
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    sd = no.init_weights(model, hidden=hidden, heads=heads, seed=17, random_conv_bias=True)
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    net = cls(5, hidden, 2, heads, n, dueling_param=duel(), device="cuda", backend=backend, **kw)
    net.load_state_dict(sd)
    return net, sd


def oracle_logits(model, sd, obs, n, heads, agg="max"):
    from oracle import net_oracle as no
    torch.set_num_threads(8)
    with torch.no_grad():
        if model == "hl_dgn":
            return no.hldgn_forward(sd, obs, n, heads=heads, aggregator=agg).numpy()
        return (no.ldgn_forward if model == "l_dgn" else no.dgnr_forward)(sd, obs, n, heads=heads).numpy()


def agent_sets(n, bs, seed):
    """Several controlling agents per env: masks (int64 [bs], [bs, 2] beyond 64 nodes) and the (env, agent) rows they stand for,
    by env and then by agent id - the order of hip_forward_agents' logits rows."""
    rng = np.random.RandomState(seed)
    words = (n + 63) // 64
    masks = np.zeros((bs, words), dtype=np.uint64)
    rows = []
    for b in range(bs):
        k = rng.randint(2, min(n, 6) + 1)
        agents = sorted(int(a) for a in rng.choice(n, size=k, replace=False))
        if n > 64 and b == 0:
            agents = sorted(set(agents) | {n - 1})               # an agent in the second word
        for a in agents:
            masks[b, a // 64] |= np.uint64(1) << np.uint64(a % 64)
            rows.append((b, a))
    am = masks.view(np.int64)
    return (am[:, 0].copy() if words == 1 else am), rows


def check_entry_points(net, sd, model, agg, obs, n, heads, integer, tol=TOL, expect_table=None):
    """Every forward entry point of the model on these observations against the oracle -> the logits of the envs / agents call."""
    from melissa_amd import _lib
    bs = obs.shape[0]
    t = torch.from_numpy(obs).cuda()
    mat = t[:, :-1].contiguous()
    want = oracle_logits(model, sd, obs, n, heads, agg)
    with torch.no_grad():
        got = net.hip_forward(t, integer_features=integer).cpu().numpy()
        np.testing.assert_allclose(got, want, atol=tol, rtol=0, err_msg="hip_forward")
        if model == "hl_dgn":
            envs = net.hip_forward_envs(mat, integer_features=integer)
            if expect_table is not None:
                assert (int(net.hip_tap(3, bs)[0]) > 0) == expect_table
            np.testing.assert_allclose(envs.cpu().numpy(), want, atol=tol, rtol=0, err_msg="hip_forward_envs")
            masks, _rows = agent_sets(n, bs, 5)
            live = torch.from_numpy(masks).cuda()
            act = torch.full((bs * n,), -1, dtype=torch.int32, device="cuda")
            rounds = torch.tensor([3], dtype=torch.int32, device="cuda")
            sel = _lib.MelSelect()
            sel.act, sel.eps, sel.seed, sel.step_dev = act.data_ptr(), 0.0, 77, rounds.data_ptr()
            sel.live, sel.n_nodes = live.data_ptr(), n
            chosen = net.hip_forward_envs(mat, select=sel, integer_features=integer)
            assert torch.equal(chosen, envs)
            acted = act.view(bs, n).cpu().numpy()
            for b, a in _rows:                                    # eps 0: the greedy action of the env's logits
                assert acted[b, a] == int(np.argmax(envs[b].cpu().numpy()))
            assert (acted >= 0).sum() == len(_rows)
            return envs
        else:
            masks, rows = agent_sets(n, bs, 5)
            cap = bs * n
            logits, off = net.hip_forward_agents(mat, torch.from_numpy(masks).cuda(), cap, integer_features=integer)
            if expect_table is not None:
                assert (int(net.hip_tap(3, bs, cap)[0]) > 0) == expect_table
            assert int(off[-1]) == len(rows)
            obs_rows = np.concatenate([obs[[b for b, _ in rows], :-1], np.array([[a] for _, a in rows], dtype=np.float32)], axis=1)
            want_rows = oracle_logits(model, sd, obs_rows, n, heads)
            np.testing.assert_allclose(logits[:len(rows)].cpu().numpy(), want_rows, atol=tol, rtol=0, err_msg="hip_forward_agents")
            return logits[:len(rows)].clone()


# ---- 1. forward parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f32a"])
@pytest.mark.parametrize("n,bs", SIZES)
@pytest.mark.parametrize("hidden,heads", SHAPES)
@pytest.mark.parametrize("model,agg", MODELS)
def test_six_head_forward_matches_oracle(model, agg, hidden, heads, n, bs, dtype):
    obs = random_obs(n, bs, 300 + n)
    net, sd = make_net(model, n, hidden, heads, agg)
    net.set_feature_dtype(dtype)
    for integer in (False, True):              # (batches this small never take the node-feature table: the flag alone)
        check_entry_points(net, sd, model, agg, obs, n, heads, integer)


TABLE_CASES = [(m, agg, n, bs, h, k, d) for m, agg, n, bs in [("l_dgn", "max", 20, 128), ("dgn_r", "max", 20, 128),
                                                               ("hl_dgn", "max", 20, 96), ("hl_dgn", "mean", 70, 88)]
               for h, k in SHAPES for d in ("f32", "f32a")] + [("l_dgn", "max", 70, 168, 64, 6, "f32a")]


@pytest.mark.parametrize("model,agg,n,bs,hidden,heads,dtype", TABLE_CASES)
def test_six_head_forward_through_the_node_feature_table(model, agg, n, bs, hidden, heads, dtype):
    """Batches from which the envs / agents forward takes the node-feature table (checked through the tap): the table source form
    of the walk, one and two set words; (128, 6) L-DGN is also the shape whose table comes from the plan launch (table_fuses).
    Per row the table is the row lists' arithmetic in the same order (tests/test_gpu_feature_table.py): the same bits."""
    obs = random_obs(n, bs, 500 + n)
    net, sd = make_net(model, n, hidden, heads, agg)
    net.set_feature_dtype(dtype)
    table = check_entry_points(net, sd, model, agg, obs, n, heads, True, expect_table=True)
    mat = torch.from_numpy(obs[:, :-1].copy()).cuda()
    with torch.no_grad():
        if model == "hl_dgn":
            rows = net.hip_forward_envs(mat)
            assert int(net.hip_tap(3, bs)[0]) == 0
        else:
            masks, pairs = agent_sets(n, bs, 5)
            rows = net.hip_forward_agents(mat, torch.from_numpy(masks).cuda(), bs * n)[0][:len(pairs)]
            assert int(net.hip_tap(3, bs, bs * n)[0]) == 0
    assert torch.equal(rows, table)


@pytest.mark.parametrize("integer", [False, True])
def test_six_head_pool_launch_of_2048_envs(integer):
    """bs >= 2048: four waves per env instead of eight."""
    n, bs = 20, 2048
    obs = random_obs(n, bs, 9)
    net, sd = make_net("hl_dgn", n, 64, 6, "max")
    want = oracle_logits("hl_dgn", sd, obs, n, 6, "max")
    with torch.no_grad():
        got = net.hip_forward_envs(torch.from_numpy(obs[:, :-1].copy()).cuda(), integer_features=integer)
        assert (int(net.hip_tap(3, bs)[0]) > 0) == integer
    np.testing.assert_allclose(got.cpu().numpy(), want, atol=TOL, rtol=0)


@pytest.mark.parametrize("n,bs", [(20, 64), (70, 3)])
@pytest.mark.parametrize("hidden,heads", SHAPES)
@pytest.mark.parametrize("model,agg", [("l_dgn", "max"), ("dgn_r", "max"), ("hl_dgn", "max")])
def test_six_head_forward_at_the_other_precisions(model, agg, hidden, heads, n, bs):
    """f32s: every projection is planned onto a kernel that fits (K = 64 stays on the exact-fp32 kernels), the fp32 bar.
    bf16: the bf16 feature path runs these shapes, tests/test_gpu_bf16.py's bar (2e-2 absolute, the greedy action wherever the
    fp32 action gap exceeds twice the error)."""
    obs = random_obs(n, bs, 700 + n)
    net, sd = make_net(model, n, hidden, heads, agg)
    want = oracle_logits(model, sd, obs, n, heads, agg)
    t = torch.from_numpy(obs).cuda()
    with torch.no_grad():
        net.set_feature_dtype("f32s")
        got = net.hip_forward(t).cpu().numpy()
        print(f"f32s max abs error {np.abs(got - want).max():.2e}")
        np.testing.assert_allclose(got, want, atol=TOL, rtol=0)
        net.set_feature_dtype("bf16")
        got = net.hip_forward(t).cpu().numpy()
    err = np.abs(got - want).max()
    same = got.argmax(1) == want.argmax(1)
    decided = np.abs(want[:, 0] - want[:, 1]) > 2 * max(err, 1e-6)
    print(f"bf16 max abs error {err:.2e}, argmax agreement {same.mean() * 100:.1f} %")
    assert err <= 2e-2 and same[decided].all()
    if bs >= 64:
        assert same.mean() >= 0.99


# ---- hidden 512 with 2 heads: the encoder's first layer as a launch of its own (wider than the GEMMs' fused producer) ----------
@pytest.mark.parametrize("dtype", ["f32", "f32a", "f32s", "bf16"])
@pytest.mark.parametrize("model,agg,n,bs,integer", [("l_dgn", "max", 20, 3, False), ("dgn_r", "max", 70, 3, False),
                                                    ("hl_dgn", "mean", 7, 3, False), ("hl_dgn", "max", 70, 3, False),
                                                    ("l_dgn", "max", 20, 128, True), ("dgn_r", "max", 20, 128, True),
                                                    ("hl_dgn", "add", 20, 96, True)])
def test_wide_encoder_forward_matches_oracle(model, agg, n, bs, integer, dtype):
    """(512, 2): every entry point, row lists (ragged, device-side row counts) and the node-feature table (checked through the
    tap), at the fp32 bar for the three fp32-accurate precisions and tests/test_gpu_bf16.py's 2e-2 for bf16 rows."""
    obs = random_obs(n, bs, 900 + n)
    net, sd = make_net(model, n, 512, 2, agg)
    net.set_feature_dtype(dtype)
    check_entry_points(net, sd, model, agg, obs, n, 2, integer, tol=2e-2 if dtype == "bf16" else TOL,
                       expect_table=integer)


@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn"])
def test_wide_encoder_prepared_tables_match_the_per_call_tables(model):
    """prepared_tables at (512, 2): the layer-0 rows pass through the table's own source rows; same logits as the per-call table."""
    n, bs = 20, 128 if model == "l_dgn" else 96
    obs = random_obs(n, bs, 900 + n)
    net, _sd = make_net(model, n, 512, 2)
    mat = torch.from_numpy(obs[:, :-1].copy()).cuda()
    masks, rows = agent_sets(n, bs, 5)

    def forward():
        with torch.no_grad():
            if model == "hl_dgn":
                out = net.hip_forward_envs(mat, integer_features=True).clone()
                assert int(net.hip_tap(3, bs)[0]) == n * 40
            else:
                out = net.hip_forward_agents(mat, torch.from_numpy(masks).cuda(), bs * n, integer_features=True)[0][:len(rows)].clone()
                assert int(net.hip_tap(3, bs, bs * n)[0]) == n * 40
        return out

    per_call = forward()
    net.prepared_tables = True
    assert torch.equal(forward(), per_call)


# ---- dueling heads of other widths (--dueling-q-hidden-sizes / --dueling-v-hidden-sizes), every precision -----------------------
@pytest.mark.parametrize("dtype", ["f32", "f32a", "f32s", "bf16"])
@pytest.mark.parametrize("q_sizes,v_sizes", [([64, 64], [128, 128]), ([128, 128], [64, 64]), ([64, 64], [64, 64]), ([64], [128]),
                                             ([128, 64, 128], [64, 128, 64])])
@pytest.mark.parametrize("model,hidden,heads", [("l_dgn", 64, 6), ("hl_dgn", 128, 4)])
def test_dueling_widths_at_every_precision(model, hidden, heads, q_sizes, v_sizes, dtype):
    """Q and V heads of different widths, 64-wide layers among them: from the second layer on the two heads share one launch,
    and under f32s a layer with K < 128 keeps its fp32 matrix - then its partner in that launch does too (never an fp32
    matrix and bf16 planes in one launch, whichever head comes first)."""
    from melissa_amd.train import build_network
    n, bs = 20, 40
    torch.manual_seed(13)
    net = build_network(model, n, "cuda", hidden=hidden, heads=heads, dueling_q_hidden_sizes=q_sizes, dueling_v_hidden_sizes=v_sizes)
    net.backend = "hip"
    with torch.no_grad():
        for conv in [net.conv1] + ([net.conv2] if model == "l_dgn" else []):
            conv.bias.uniform_(-0.1, 0.1)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    assert sd["Q.model.0.weight"].shape[0] == q_sizes[0] and sd["V.model.0.weight"].shape[0] == v_sizes[0]
    obs = random_obs(n, bs, 77)
    want = oracle_logits(model, sd, obs, n, heads)
    net.set_feature_dtype(dtype)
    with torch.no_grad():
        got = net.hip_forward(torch.from_numpy(obs).cuda()).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"{dtype} max abs error {err:.2e}")
    assert err <= (2e-2 if dtype == "bf16" else TOL)


# ---- 2. learn path -----------------------------------------------------------------------------------------------------
LEARN_CASES = [(m, agg, h, k, n, bs) for m, agg in MODELS for h, k in SHAPES for n, bs in [(20, 5), (70, 3)]] + \
              [(m, "max", 512, 2, 20, 5) for m in ("l_dgn", "dgn_r", "hl_dgn")]


@pytest.mark.parametrize("model,agg,hidden,heads,n,bs", LEARN_CASES)
def test_six_head_autograd_matches_oracle_autograd(model, agg, hidden, heads, n, bs):
    from oracle import net_oracle as no
    obs_np = random_obs(n, bs, 300 + n)
    act_np = np.random.RandomState(5).randint(0, 2, bs)
    target_np = np.random.RandomState(6).uniform(-1, 1, bs).astype(np.float32)
    net, sd = make_net(model, n, hidden, heads, agg, backend="torch")
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    torch.set_num_threads(8)
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    want_logits = {"l_dgn": no.ldgn_forward, "dgn_r": no.dgnr_forward, "hl_dgn": no.hldgn_forward}[model](leaves, obs_np, n, heads=heads, **kw)
    want_loss = (want_logits[torch.arange(bs), torch.from_numpy(act_np)] - torch.from_numpy(target_np)).pow(2).mean()
    want_loss.backward()
    want = {k: v.grad for k, v in leaves.items()}
    net.learn_kernels = "hip"
    logits = net.torch_forward(torch.from_numpy(obs_np).cuda())
    loss = (logits[torch.arange(bs), torch.from_numpy(act_np).cuda()] - torch.from_numpy(target_np).cuda()).pow(2).mean()
    loss.backward()
    torch.testing.assert_close(logits.detach().cpu(), want_logits.detach(), atol=1e-4, rtol=0)
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-4 * max(1.0, abs(float(want_loss.detach())))
    checked = []
    for k, p in net.named_parameters():
        gd, gh = want[k], p.grad
        if gd is None or float(gd.abs().max()) == 0.0:              # lin_skip (unused by TransformerConv), V bias under mean...
            assert gh is None or float(gh.abs().max()) <= 1e-7, k
            continue
        scale = float(gd.abs().max())
        assert gh is not None, k
        err = float((gh.cpu() - gd).abs().max())
        assert err <= 2e-4 * scale + 1e-7, (k, err, scale)
        checked.append(k)
    assert len(checked) >= 10
    # every att / bias / lin_* gradient of the convolutions is present (lin_skip is unused; a key bias shifts every score of a
    # target alike, so its gradient may be exactly zero)
    per_conv = ("lin_key.weight", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias") if model == "dgn_r" \
        else ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")
    for conv in (("conv1",) if model == "hl_dgn" else ("conv1", "conv2")):
        for name in per_conv:
            assert f"{conv}.{name}" in checked, f"{conv}.{name}"


# ---- 3. + 4. no writes past the row, nothing read from beside it ------------------------------------------------------
GUARD = 64          # floats of sentinel / poison before and behind every buffer
SENTINEL = -12345.5


class Guarded:
    """A device buffer of `count` floats with GUARD floats in front of and behind it."""

    def __init__(self, count, fill=None, dtype=torch.float32):
        self.whole = torch.full((count + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
        self.t = self.whole[GUARD:GUARD + count]
        if fill is not None:
            self.t.copy_(fill.reshape(-1))

    def ptr(self):
        return self.t.data_ptr()

    def guards(self, value):
        self.whole[:GUARD] = value
        self.whole[-GUARD:] = value

    def intact(self):
        g = torch.cat([self.whole[:GUARD], self.whole[-GUARD:]])
        return bool((g == SENTINEL).all())


@pytest.mark.parametrize("kind", ["gatv2", "transformer"])
@pytest.mark.parametrize("n,bs", [(20, 3), (70, 2), (7, 3)])
@pytest.mark.parametrize("heads,channels", [(6, 64), (6, 128)])
def test_learn_path_kernels_stay_inside_their_rows(heads, channels, n, bs, kind):
    """mel_gat_forward / mel_gat_backward on caller buffers with 64 floats of sentinel around each: every sentinel holds its value
    (outputs, statistics, partial sums), and with NaN in the 64 floats before and behind every INPUT buffer the results are
    the bits of the clean run - an idle lane neither writes past a row nor lets what lies beside one into a result."""
    from melissa_amd import _lib
    from melissa_amd.networks.autograd_ops import radius_graph
    lib = _lib.load()
    hc, rows = heads * channels, bs * n
    g = torch.Generator(device="cuda").manual_seed(n + channels)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    adj = radius_graph(torch.from_numpy(random_obs(n, bs, 3)).cuda(), n, 5)
    tk = kind == "transformer"
    code = _lib.CONV_TRANSFORMER if tk else _lib.CONV_GATV2
    xl, xr, gout = Guarded(rows * hc, rnd(rows, hc)), Guarded(rows * hc, rnd(rows, hc)), Guarded(rows * hc, rnd(rows, hc))
    xv = Guarded(rows * hc, rnd(rows, hc)) if tk else None
    att = None if tk else Guarded(hc, rnd(hc) * 0.3)
    bias = None if tk else Guarded(hc, rnd(hc) * 0.1)
    inputs = [b for b in (xl, xr, gout, xv, att, bias) if b is not None]
    p = lambda b: b.ptr() if b is not None else None
    stream = _lib.current_stream_ptr()

    def run():
        out, dxl, dxr = Guarded(rows * hc), Guarded(rows * hc), Guarded(rows * hc)
        dxv = Guarded(rows * hc) if tk else None
        datt, dbias = (None, None) if tk else (Guarded(hc), Guarded(hc))
        stats = Guarded(rows * heads * 4 + 256 * 2 * hc)
        _lib.check(lib.mel_gat_forward(xl.ptr(), p(xv), xr.ptr(), p(att), p(bias), adj.data_ptr(), bs, n, heads, channels, code,
                                       out.ptr(), stream), "mel_gat_forward")
        _lib.check(lib.mel_gat_backward(xl.ptr(), p(xv), xr.ptr(), p(att), adj.data_ptr(), out.ptr(), gout.ptr(), bs, n, heads,
                                        channels, code, dxl.ptr(), p(dxv), dxr.ptr(), p(datt), p(dbias), stats.ptr(), stream),
                   "mel_gat_backward")
        torch.cuda.synchronize()
        outs = [b for b in (out, dxl, dxr, dxv, datt, dbias) if b is not None]
        for b in outs + [stats]:
            assert b.intact()
        assert all(torch.isfinite(b.t).all() for b in outs)
        return [b.t.clone() for b in outs]

    for b in inputs:
        b.guards(0.0)
    clean = run()
    for b in inputs:
        b.guards(float("nan"))
    poisoned = run()
    for a, b in zip(clean, poisoned):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(clean[0].abs().max()) > 0


@pytest.mark.parametrize("agg", ["max", "mean", "add"])
def test_learn_path_pool_stays_inside_its_rows(agg):
    from melissa_amd import _lib
    lib = _lib.load()
    n, bs, hc = 20, 3, 384
    x = Guarded(bs * n * hc, torch.randn(bs * n, hc, device="cuda"))
    dm = Guarded(bs * n, (torch.rand(bs * n, device="cuda") > 0.2).float())
    pooled, arg = Guarded(bs * hc), Guarded(bs * hc, dtype=torch.int32)
    outs = []
    for poison in (0.0, float("nan")):
        x.guards(poison), dm.guards(poison)
        _lib.check(lib.mel_pool_forward(x.ptr(), dm.ptr(), bs, n, hc, _lib.AGG[agg], pooled.ptr(), arg.ptr(),
                                        _lib.current_stream_ptr()), "mel_pool_forward")
        torch.cuda.synchronize()
        assert pooled.intact() and bool((torch.cat([arg.whole[:GUARD], arg.whole[-GUARD:]]) == int(SENTINEL)).all())
        outs.append(pooled.t.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and torch.isfinite(outs[0]).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n,bs", [(20, 3), (70, 3)])
@pytest.mark.parametrize("hidden,heads", SHAPES)
@pytest.mark.parametrize("model", ["l_dgn", "dgn_r", "hl_dgn"])
def test_forward_stays_inside_the_workspace_and_ignores_what_lies_in_it(model, hidden, heads, n, bs, dtype):
    """The forward on a caller workspace with one page of sentinel behind it and behind the logits: the page holds.  The
    workspace's buffers lie side by side (rows of 384 / 768 channels, fp32 or bf16), so a forward into a workspace full of NaN
    bit patterns must give the bits of a forward into a zeroed one: nothing beside a row reaches a result."""
    PAGE = 4096
    obs = random_obs(n, bs, 11 + n)
    net, _sd = make_net(model, n, hidden, heads)
    net.set_feature_dtype(dtype)
    mat = torch.from_numpy(obs[:, :-1].copy()).cuda()
    masks, rows = agent_sets(n, bs, 5)
    cap = bs * n
    need = net.agents_workspace_bytes(bs, cap)
    ws = torch.empty(need + PAGE, dtype=torch.uint8, device="cuda")
    results = []
    for fill in (0, 0xFF):
        ws[:need] = fill
        ws[need:] = 0xA5
        out = torch.full((cap * 2 + PAGE // 4,), SENTINEL, dtype=torch.float32, device="cuda")
        with torch.no_grad():
            if model == "hl_dgn":
                net.hip_forward_envs(mat, out=out[:bs * 2].view(bs, 2), workspace=ws[:need])
                used = bs * 2
            else:
                net.hip_forward_agents(mat, torch.from_numpy(masks).cuda(), cap, out=out[:cap * 2].view(cap, 2), workspace=ws[:need])
                used = len(rows) * 2
        torch.cuda.synchronize()
        assert bool((ws[need:] == 0xA5).all())
        assert bool((out[used:] == SENTINEL).all())
        assert torch.isfinite(out[:used]).all()
        results.append(out[:used].clone())
    assert torch.equal(results[0].view(torch.int32), results[1].view(torch.int32))


# ---- 5. the shapes that ran before keep their bits ---------------------------------------------------------------------
@pytest.mark.parametrize("model,agg", PARENT_CASES)
def test_existing_shapes_keep_their_bits(model, agg):
    """(128, 4), n = 20, bs = 3 against the logits recorded at the parent commit (tests/golden/make_head_shapes_golden.py)."""
    with np.load(PARENT_GOLDEN) as z:
        want = z[f"{model}_{agg}"]
    got = parent_case_logits(model, agg)
    assert got.dtype == want.dtype and np.array_equal(got.view(np.int32), want.view(np.int32))


# ---- 6. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn", "dgn_r"])
def test_train_six_heads_end_to_end(model):
    from melissa_amd.train import _param_checksum, build_network, train
    lines = []
    out = train(model, n_nodes=20, envs=8, updates=3, hidden_emb=64, num_heads=6, graphs=16, log=lines.append)
    assert np.isfinite(out["loss_first"]) and np.isfinite(out["loss_last"])
    assert out["errors"] == 0 and out["updates"] == 3 and out["updates_from_hip_graphs"]
    assert (out["hidden_emb"], out["num_heads"]) == (64, 6)
    rec = json.loads(lines[-1])
    assert (rec["hidden_emb"], rec["num_heads"]) == (64, 6)
    torch.manual_seed(9)                                          # train()'s seed: the weights it started from
    start = _param_checksum(build_network(model, 20, "cuda", hidden=64, heads=6))
    assert np.isfinite(out["param_checksum"]) and out["param_checksum"] != start


@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn", "dgn_r"])
def test_captured_six_head_update_equals_the_eager_update(model):
    """As tests/test_gpu_round.py::test_captured_update_equals_the_eager_update, at (64, 6): the update replayed from HIP graphs
    against an eager update on the same batch from the same weights and optimizer state - the loss to the bits."""
    import copy
    from melissa_amd.collect import RoundLoop
    from melissa_amd.env import HipGraphVectorEnv, synthetic_graph_pool
    from melissa_amd.policy import DGNPolicy, DQNPolicy
    from melissa_amd.replay import DGNLearner, DQNLearner, RoundReplay
    from melissa_amd.train import build_network
    n, envs = 20, 16
    policy_cls, learner_cls = (DGNPolicy, DGNLearner) if model == "dgn_r" else (DQNPolicy, DQNLearner)

    def make_policy():
        torch.manual_seed(3)
        net = build_network(model, n, "cuda", hidden=64, heads=6)
        return net, policy_cls(net, torch.optim.Adam(net.parameters(), lr=1e-3), estimation_step=4, target_update_freq=3)

    net, policy = make_policy()
    venv = HipGraphVectorEnv(envs, n, graph_pool=synthetic_graph_pool(n, 8, 0), dynamic_graph=True, device="cuda", max_moves=48,
                             seed=11, construct_like_reference=False)
    replay = RoundReplay(envs, n, 16, "cuda")
    loop = RoundLoop(venv, policy, seed=11, eps=0.1, replay=replay)
    with torch.no_grad():
        loop.run(20)
    learner = learner_cls(policy, replay, batch_size=32, n_step=4, gamma=0.99, seed=2)
    learner.capture()
    twin_net, twin = make_policy()
    for k in range(2):
        twin_net.load_state_dict(net.state_dict())
        twin.model_old.load_state_dict(policy.model_old.state_dict())
        twin.optim.load_state_dict(copy.deepcopy(policy.optim.state_dict()))
        twin._iter = policy._iter
        out = learner.step()
        want = twin.learn({key: v.clone() for key, v in learner.last_batch.items()})
        got_loss, want_loss = np.float32(float(out["loss"])), np.float32(want["loss"])
        print(f"update {k}: captured loss {got_loss!r}, eager loss {want_loss!r}")
        assert np.isfinite(got_loss) and got_loss.tobytes() == want_loss.tobytes()
        for (name, p), q in zip(net.named_parameters(), twin_net.parameters()):
            assert float((p.detach() - q.detach()).abs().max()) <= 2e-6, (k, name)
    assert loop.counters()["errors"] == 0


def test_train_main_takes_the_flags(capsys):
    from melissa_amd import train
    train.main(["--model", "hl_dgn", "--nodes", "20", "--envs", "8", "--updates", "2", "--graphs", "16", "--num-heads", "2",
                "--hidden-emb", "64"])
    rec = json.loads([line for line in capsys.readouterr().out.splitlines() if line.startswith("{")][-1])
    assert (rec["hidden_emb"], rec["num_heads"], rec["updates"], rec["errors"]) == (64, 2, 2, 0)
    assert np.isfinite(rec["loss_last"])


def test_watch_loads_only_checkpoints_of_its_shape(tmp_path):
    from melissa_amd.policy import DQNPolicy
    from melissa_amd.train import build_network
    from melissa_amd.watch import watch
    path = str(tmp_path / "six.pth")
    torch.manual_seed(1)
    torch.save(DQNPolicy(build_network("l_dgn", 20, "cuda", hidden=64, heads=6), target_update_freq=1).state_dict(), path)
    out = watch("l_dgn", 20, envs=2, episodes=2, load=path, hidden_emb=64, num_heads=6)
    assert out["n/ep"] == 2
    with pytest.raises(ValueError, match=r"model\.conv1\.att is \(1, 6, 64\) in the checkpoint and \(1, 4, 64\)"):
        watch("l_dgn", 20, envs=2, episodes=2, load=path, hidden_emb=64, num_heads=4)


# ---- 7. the Python rule and the library agree --------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn"])
@pytest.mark.parametrize("hidden,heads", sorted(SHAPE_TABLE) + [(128, 3), (128, 5)])
def test_shape_rule_and_library_agree(hidden, heads, model):
    """Building the network and running one bs = 1 forward succeeds exactly when hip_shape_supported says so - and the learn
    path's entry point takes the same pairs.  (Head counts the rule refuses - 3, 5 - are refused by the library too.)"""
    from melissa_amd import _lib
    from melissa_amd.networks import hip_shape_supported
    from melissa_amd.train import build_network
    ok, reason = hip_shape_supported(hidden, heads)
    n = 12
    torch.manual_seed(0)
    net = build_network(model, n, "cuda", hidden=hidden, heads=heads)
    net.backend = "hip"
    obs = torch.from_numpy(random_obs(n, 1, 2)).cuda()
    try:
        with torch.no_grad():
            logits = net.hip_forward(obs)
        ran = bool(torch.isfinite(logits).all())
    except RuntimeError as e:
        ran = False
        assert "heads" in str(e) or "encoder" in str(e) or "hidden" in str(e), str(e)
    assert ran == ok, (hidden, heads, reason)
    # the learn path's entry point takes every pair the networks run (its kernels alone take more: they have no encoder)
    x = torch.zeros(n, heads * hidden, device="cuda")
    adj = torch.zeros(n, dtype=torch.int64, device="cuda")
    out = torch.empty_like(x)
    st = _lib.load().mel_gat_forward(x.data_ptr(), x.data_ptr(), x.data_ptr(), None, None, adj.data_ptr(), 1, n, heads, hidden,
                                     _lib.CONV_TRANSFORMER, out.data_ptr(), _lib.current_stream_ptr())
    if ok:
        assert st == 0
    elif st == 0:
        assert hidden < 64 or hidden > 256, (hidden, heads)
