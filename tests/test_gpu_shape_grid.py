"""GPU tests of EVERY (hidden, heads) pair melissa_amd.shapes.hip_shape_supported accepts, against oracle/net_oracle.py evaluated
in float64, under bounds that are 8 times the oracle's own float32 noise (tests/shape_grid_ref.py: the grid, the inputs, the
bounds; tests/test_shape_grid_ref.py: the measurement and the mutants those bounds catch).

The pairs reach different code: attention.hpp's head_sum has one path per lanes-per-head count (64, 32, 16 at compile and at
run time, 8 on 64 and on 48 live lanes, 4), the attention kernels one instance per channels-per-lane count, the GEMM planner
cuts the heads' first layer's split-K from K = hidden (1 + 2 heads), hidden != 128 takes the two-launch node-feature table and
hidden > 256 the encoder's own first-layer launch; grad.hip picks V at compile time and the lanes per head at run time."""
import functools

import numpy as np
import pytest
import torch

from tests import shape_grid_ref as sg

pytestmark = pytest.mark.gpu
IDS = [sg.cell_id(c) for c in sg.CELLS]
POISON = 0xCD                       # every byte of the workspace before a forward: fp32 0xcdcdcdcd (-4.3e8), bf16 0xcdcd
SENTINEL = -12345.5


def duel():
    return ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


def make_net(cell, n, backend="hip"):
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    hidden, heads, model, agg = cell
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    net = cls(5, hidden, 2, heads, n, dueling_param=duel(), device="cuda", backend=backend, **kw)
    net.load_state_dict(sg.weights(model, hidden, heads))
    return net


@functools.lru_cache(maxsize=None)
def exact(cell, name):
    """The float64 oracle of a cell on a case, computed once: (logits, head input, adjacency); L-DGN / DGN-R: the rows of
    sg.case_rows - the index column's first, then the agent sets'."""
    hidden, heads, model, agg = cell
    obs, _live = sg.case_inputs(name)
    rows = None if model == "hl_dgn" else sg.case_rows(name)
    return sg.oracle(model, agg, sg.weights(model, hidden, heads), obs, sg.CASES[name][0], heads, rows=rows)


class Report:
    """Prints every measured difference beside its bound and collects the misses."""

    def __init__(self, label):
        self.label, self.failures = label, []

    def close(self, what, got, want, tol):
        err = float(np.abs(np.asarray(got, dtype=np.float64) - want).max()) if np.size(want) else 0.0
        print(f"{self.label} {what}: {err:.2e} (bound {tol:.1e})")
        if not err <= tol:
            self.failures.append(f"{what}: {err:.3e} > {tol:.1e}")

    def true(self, what, ok):
        if not ok:
            self.failures.append(what)

    def done(self):
        assert not self.failures, self.label + ": " + "; ".join(self.failures)


def bf16_logits(rep, what, got, want):
    """The project's bf16 bar (tests/test_gpu_bf16.py): 2e-2 absolute, the greedy action kept where the float64 gap exceeds it."""
    rep.close(what, got, want, sg.BF16_TOL)
    decided = np.abs(want[:, 0] - want[:, 1]) > 2 * sg.BF16_TOL
    rep.true(what + ": greedy action", bool((got.argmax(1) == want.argmax(1))[decided].all()))


def poisoned(t):
    return bool((t.contiguous().view(torch.uint8) == POISON).all())


def check_entry_points(cell, name, dtype, integer=False, rep=None):
    """Every forward entry point of the cell's model on a case, logits and head input (mel_forward_tap kind 1) against the
    float64 oracle; row offsets and the tap's row counts against the oracle's adjacency; the workspace full of POISON before
    each forward: head-input rows and logits rows past the live count still hold what was there."""
    hidden, heads, model, agg = cell
    key = sg.model_key(model, agg)
    n, bs, _ = sg.CASES[name]
    obs, live = sg.case_inputs(name)
    want_logits, want_head, adj = exact(cell, name)
    net = make_net(cell, n)
    net.set_feature_dtype(dtype)
    rep = rep or Report(f"{sg.cell_id(cell)} {name} {dtype}")
    t = torch.from_numpy(obs).cuda()
    mat = t[:, :-1].contiguous()
    f32 = dtype != "bf16"

    def compare(what, logits, head, want_l, want_h):
        if f32:
            rep.close(what + " logits", logits, want_l, sg.LOGITS_TOL[key])
            rep.close(what + " head input", head, want_h, sg.HEAD_INPUT_TOL[key])
        else:
            bf16_logits(rep, what + " logits", logits, want_l)

    with torch.no_grad():
        net.hip_forward(t, integer_features=integer)                       # (allocates the module's workspace)
        net._ws.fill_(POISON)
        got = net.hip_forward(t, integer_features=integer).cpu().numpy()
        head = net.hip_tap(1, bs).float().cpu().numpy()
        compare("hip_forward", got, head, want_logits[:bs], want_head[:bs])
        if model == "hl_dgn":
            net._ws.fill_(POISON)
            out = torch.full((bs + 8, 2), SENTINEL, device="cuda")
            net.hip_forward_envs(mat, out=out[:bs], integer_features=integer)
            compare("hip_forward_envs", out[:bs].cpu().numpy(), net.hip_tap(1, bs).float().cpu().numpy(), want_logits, want_head)
            rep.true("hip_forward_envs wrote past its logits", bool((out[bs:] == SENTINEL).all()))
        else:
            cap, rows = bs * n, int(live.sum())
            am = torch.from_numpy(sg.agent_words(live)).cuda()
            ws = torch.full((net.agents_workspace_bytes(bs, cap) + 4096,), POISON, dtype=torch.uint8, device="cuda")
            out = torch.full((cap + 8, 2), SENTINEL, device="cuda")
            _, off = net.hip_forward_agents(mat, am, cap, out=out[:cap], workspace=ws[:-4096], integer_features=integer)
            head = net.hip_tap(1, bs, cap, workspace=ws[:-4096])
            compare("hip_forward_agents", out[:rows].cpu().numpy(), head[:rows].float().cpu().numpy(), want_logits[bs:], want_head[bs:])
            rep.true("row offsets", np.array_equal(off.cpu().numpy(), np.concatenate([[0], np.cumsum(live.sum(1))])))
            counts = tuple(int(v) for v in net.hip_tap(2, bs, cap, workspace=ws[:-4096]).cpu())
            rep.true(f"rows processed {counts} != {sg.plan_counts(adj, live, model == 'l_dgn')}",
                     counts == sg.plan_counts(adj, live, model == "l_dgn"))
            rep.true("logits rows past the live count were written", bool((out[rows:] == SENTINEL).all()))
            rep.true("head-input rows past the live count were written", poisoned(head[rows:]))
            rep.true("the page behind the workspace was written", poisoned(ws[-4096:]))
    return net, rep


# ---- forward ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.FORWARD_CASES)
@pytest.mark.parametrize("cell", sg.CELLS, ids=IDS)
def test_forward_f32_matches_the_float64_oracle(cell, name):
    check_entry_points(cell, name, "f32")[1].done()


@pytest.mark.parametrize("dtype", ["f32s", "f32a", "bf16"])
@pytest.mark.parametrize("cell", sg.CELLS, ids=IDS)
def test_forward_at_the_other_precisions(cell, dtype):
    """f32s / f32a: the planner's kernel choice follows the shape; the float64 bounds.  bf16: the project's bf16 bar."""
    check_entry_points(cell, "n40", dtype)[1].done()


@pytest.mark.parametrize("cell", sg.CELLS, ids=IDS)
def test_node_feature_table(cell):
    """Integer features past the batch from which n = 7 takes the table (hidden != 128: the two-launch one), per call and
    prepared: the tap shows the table was taken - a fallback to the row lists would give the right logits too -, the float64
    bounds hold, and the logits are the bits of the row-list forward of the same inputs (per row the table is the row lists'
    arithmetic in the same order: tests/test_gpu_feature_table.py)."""
    hidden, heads, model, agg = cell
    name = sg.TABLE_CASE_HL if model == "hl_dgn" else sg.TABLE_CASE
    n, bs, _ = sg.CASES[name]
    obs, live = sg.case_inputs(name)
    net, rep = check_entry_points(cell, name, "f32", integer=True)
    t = torch.from_numpy(obs).cuda()
    mat = t[:, :-1].contiguous()
    am = torch.from_numpy(sg.agent_words(live)).cuda()
    cap, rows = bs * n, int(live.sum())

    def forwards(integer):
        with torch.no_grad():
            single = net.hip_forward(t, integer_features=integer).clone()
            taken = [int(net.hip_tap(3, bs)[0])]
            if model == "hl_dgn":
                many = net.hip_forward_envs(mat, integer_features=integer).clone()
                taken.append(int(net.hip_tap(3, bs)[0]))
            else:
                many = net.hip_forward_agents(mat, am, cap, integer_features=integer)[0][:rows].clone()
                taken.append(int(net.hip_tap(3, bs, cap)[0]))
        return single, many, taken

    rows_single, rows_many, taken = forwards(False)
    rep.true(f"row lists took the table {taken}", taken == [0, 0])
    for prepared in (False, True):
        net.prepared_tables = prepared
        single, many, taken = forwards(True)
        rep.true(f"prepared {prepared}: the table was not taken {taken}", min(taken) > 0)
        rep.true(f"prepared {prepared}: hip_forward differs from the row lists' bits", torch.equal(single, rows_single))
        rep.true(f"prepared {prepared}: the envs / agents forward differs from the row lists' bits", torch.equal(many, rows_many))
    rep.done()


POOL4_CELLS = [c for c in sg.CELLS if c[2] == "hl_dgn" and c[:2] in sg.POOL4_SHAPES]


@pytest.mark.parametrize("cell", POOL4_CELLS, ids=[sg.cell_id(c) for c in POOL4_CELLS])
def test_pool_launch_of_2048_envs(cell):
    """bs >= 2048: four waves per env instead of eight (NW = 4), one pair per channels-per-lane count."""
    hidden, heads, model, agg = cell
    key = sg.model_key(model, agg)
    n, bs, _ = sg.CASES[sg.POOL4_CASE]
    obs, _ = sg.case_inputs(sg.POOL4_CASE)
    want_logits, want_head, _ = exact(cell, sg.POOL4_CASE)
    net = make_net(cell, n)
    net.set_feature_dtype("f32")
    rep = Report(f"{sg.cell_id(cell)} {sg.POOL4_CASE} f32")
    with torch.no_grad():
        got = net.hip_forward_envs(torch.from_numpy(obs[:, :-1].copy()).cuda())
        rep.close("hip_forward_envs logits", got.cpu().numpy(), want_logits, sg.LOGITS_TOL[key])
        rep.close("hip_forward_envs head input", net.hip_tap(1, bs).cpu().numpy(), want_head, sg.HEAD_INPUT_TOL[key])
    rep.done()


# ---- learn path ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sg.LEARN_CASES)
@pytest.mark.parametrize("cell", sg.CELLS, ids=IDS)
def test_learn_path_matches_float64_autograd(cell, name):
    """torch_forward on the HIP learn kernels, the squared-error loss of tests/test_gpu_grad.py, backward(): logits, loss and
    every parameter's gradient against float64 autograd through the oracle."""
    hidden, heads, model, agg = cell
    key = sg.model_key(model, agg)
    n, bs, _ = sg.CASES[name]
    obs, _ = sg.case_inputs(name)
    want_logits, want_loss, want = sg.oracle_grads(model, agg, sg.weights(model, hidden, heads), obs, n, heads)
    act, target = sg.learn_batch(bs)
    net = make_net(cell, n, backend="torch")
    net.learn_kernels = "hip"
    logits = net.torch_forward(torch.from_numpy(obs).cuda())
    loss = (logits[torch.arange(bs), torch.from_numpy(act).cuda()] - torch.from_numpy(target).cuda()).pow(2).mean()
    loss.backward()
    rep = Report(f"{sg.cell_id(cell)} {name} learn")
    rep.close("logits", logits.detach().cpu().numpy(), want_logits, sg.LOGITS_TOL[key])
    rep.close("loss", float(loss.detach()), np.float64(want_loss), sg.LOSS_TOL[key] * max(1.0, abs(want_loss)))
    got = {k: (None if p.grad is None else p.grad.cpu().numpy()) for k, p in net.named_parameters()}
    assert set(got) == set(want)
    scales = sg.grad_errors({k: np.zeros_like(v) for k, v in want.items() if v is not None}, want)
    kinks, near = sg.kink_allowance(model, agg, sg.weights(model, hidden, heads), obs, n, heads)
    worst = ("", 0.0)
    for k, g in got.items():
        if k not in scales:                # lin_skip (unused by TransformerConv), a gradient that is zero in float64
            rep.true(f"{k}: a zero gradient came back as {0.0 if g is None else np.abs(g).max():.1e}",
                     g is None or float(np.abs(g).max()) <= sg.ZERO_GRAD_TOL)
            continue
        if g is None:
            rep.true(f"{k}: no gradient", False)
            continue
        err, own = float(np.abs(g.astype(np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        bound = sg.grad_bound(key, scales[k][1], own, kinks[k])
        worst = max(worst, (k, err / bound), key=lambda kv: kv[1])
        if not err <= bound:
            rep.failures.append(f"{k}: {err:.3e} > {bound:.1e} (largest entry {own:.1e})")
    print(f"{rep.label} gradients: {len(scales)} tensors, the closest to its bound {worst[0]} at {worst[1]:.2f} of it "
          f"({near} arguments within {sg.KINK_BAND:.1e} of a kink, allowance up to {max(kinks.values()):.1e})")
    rep.true("fewer than 10 gradients checked", len(scales) >= 10)
    # every att / bias / lin_* gradient of the convolutions is present (lin_skip is unused; a key bias shifts every score of a
    # target alike: its gradient is zero)
    per_conv = ("lin_key.weight", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias") if model == "dgn_r" \
        else ("att", "bias", "lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias")
    for conv in (("conv1",) if model == "hl_dgn" else ("conv1", "conv2")):
        for pname in per_conv:
            rep.true(f"{conv}.{pname} has no gradient to check", f"{conv}.{pname}" in scales)
    rep.done()
