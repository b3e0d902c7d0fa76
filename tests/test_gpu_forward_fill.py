"""GPU tests of the agents forward where its row counts outrun the planner's estimates (tests/forward_fill_ref.py: the sizing
rules restated, the cases, the float64 reference, the bounds; tests/test_forward_fill_ref.py: that the cases are in the regime).

Every grid of mel_ldgn_forward_agents / mel_dgnr_forward_agents is sized from estimates fitted to the benchmark workload; with
every node an agent each stage meets more rows than one pass of its grid covers and goes round again: the attention rows
kernel's `r += stride` branch, head_finish_kernel's loop (with select_fused on the looped rows), encoder_layer0_kernel's.  The
other end runs too: no agent at all, one agent in a batch sized for the large kernels, and a rows_cap equal to the row count."""
import numpy as np
import pytest
import torch

from tests import forward_fill_ref as ff
from tests import shape_grid_ref as sg
from tests.test_gpu_shape_grid import POISON, SENTINEL, Report, bf16_logits, make_net, poisoned

pytestmark = pytest.mark.gpu
ACT_FILL = -7
TAIL = 4096


def grid():
    out = []
    for name in ("mid", "tight"):
        out += [(name, model, cell, dtype, False) for model in ff.MODELS for cell in ff.CELLS_MID for dtype in ("f32", "bf16")]
    out += [("two_word", model, ff.CELL_BIG, "f32", False) for model in ff.MODELS]
    for name in ("big", "single", "empty"):
        out += [(name, model, ff.CELL_BIG, dtype, integer) for model in ff.MODELS
                for dtype, integer in (("f32", False), ("f32a", False), ("f32s", False), ("bf16", False), ("f32a", True), ("bf16", True))]
    return out


GRID = grid()
IDS = [f"{name}-{model}-{cell[0]}x{cell[1]}-{dtype}" + ("-integer" if integer else "") for name, model, cell, dtype, integer in GRID]


def forward(net, obs, live, cap, integer):
    """One call on a caller-owned workspace full of POISON with a POISON page behind it, logits and actions of cap + 8 rows
    filled with sentinels, the selection fused (eps = 0) -> (logits, act, row offsets, head input, the tap's counts, workspace)."""
    from melissa_amd import _lib
    bs = live.shape[0]
    mat = torch.from_numpy(np.ascontiguousarray(obs[:, :-1])).cuda()
    am = torch.from_numpy(sg.agent_words(live)).cuda()
    ws = torch.full((net.agents_workspace_bytes(bs, cap) + TAIL,), POISON, dtype=torch.uint8, device="cuda")
    out = torch.full((cap + 8, 2), SENTINEL, device="cuda")
    act = torch.full((cap + 8,), ACT_FILL, dtype=torch.int32, device="cuda")
    sel = _lib.MelSelect()
    sel.act, sel.eps, sel.seed = act.data_ptr(), 0.0, 1
    with torch.no_grad():
        _, off = net.hip_forward_agents(mat, am, cap, out=out[:cap], select=sel, workspace=ws[:-TAIL], integer_features=integer)
        head = net.hip_tap(1, bs, cap, workspace=ws[:-TAIL])
        counts = tuple(int(v) for v in net.hip_tap(2, bs, cap, workspace=ws[:-TAIL]).cpu())
    return out, act, off.cpu().numpy(), head, counts, ws


def close_rows(rep, what, got, want, tol, fill=None):
    """Like Report.close, and names the rows that miss: how many, the first, how many of them still hold the fill."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want).reshape(len(want), -1).max(1) if len(want) else np.zeros(0)
    worst = float(err.max()) if err.size else 0.0
    print(f"{rep.label} {what}: {worst:.2e} (bound {tol:.1e})")
    bad = np.flatnonzero(~(err <= tol))
    if bad.size:
        left = "" if fill is None else f", {int((np.asarray(got)[bad] == fill).all(1).sum())} of them never written"
        rep.failures.append(f"{what}: {worst:.3e} > {tol:.1e} on {bad.size} of {len(want)} rows, the first row {bad[0]}{left}")


@pytest.mark.parametrize("name,model,cell,dtype,integer", GRID, ids=IDS)
def test_agents_forward_past_the_estimates(name, model, cell, dtype, integer):
    hidden, heads = cell
    case = ff.SETS[name]
    n, bs = ff.CASES[case]
    obs = ff.observations(case)
    live, cap = ff.agent_sets(name)
    want_logits, want_head, want_counts = ff.expected(model, hidden, heads, name)
    rows = int(live.sum())
    net = make_net((hidden, heads, model, "max"), n)
    net.set_feature_dtype(dtype)
    rep = Report(f"{name} {model} {hidden}x{heads} {dtype}" + (" integer" if integer else ""))

    out, act, off, head, counts, ws = forward(net, obs, live, cap, integer)
    # the counts tie the run to the regime tests/test_forward_fill_ref.py checks on these inputs
    rep.true(f"row offsets end at {off[-1]}, not {rows}", np.array_equal(off, np.concatenate([[0], np.cumsum(live.sum(1))])))
    rep.true(f"rows processed {counts} != {want_counts}", counts == want_counts)
    got = out[:rows].cpu().numpy()
    if dtype == "bf16":
        if rows:
            bf16_logits(rep, "logits", got, want_logits)
    else:
        tol = (ff.LOGITS_TOL[model], ff.HEAD_INPUT_TOL[model]) if dtype == "f32" else (ff.PLANES_TOL, ff.PLANES_TOL)
        close_rows(rep, "logits", got, want_logits, tol[0], fill=SENTINEL)
        close_rows(rep, "head input", head[:rows].float().cpu().numpy(), want_head, tol[1])
    # the fused selection: the first maximum of the row the kernel itself wrote
    chosen = act[:rows].cpu().numpy()
    wrong = np.flatnonzero(chosen != (got[:, 1] > got[:, 0]))
    rep.true(f"act is not the first maximum of its logits row on {wrong.size} rows, the first row {wrong[:1]} "
             f"({int((chosen[wrong] == ACT_FILL).sum())} never written)", wrong.size == 0)
    # nothing past the rows: logits and actions from row `rows` on (tight: rows == rows_cap, the first guard row), the head
    # input's rows up to rows_cap, the page behind the workspace
    rep.true("logits rows past the row count were written", bool((out[rows:] == SENTINEL).all()))
    rep.true("act entries past the row count were written", bool((act[rows:] == ACT_FILL).all()))
    rep.true("head-input rows past the row count were written", poisoned(head[rows:]))
    rep.true("the page behind the workspace was written", poisoned(ws[-TAIL:]))
    if name == "empty":
        rep.true("offsets of an empty round", not off.any() and counts == (0, 0, 0))

    # the envs in reversed order: every (env, agent) row moves to another slot - between first-pass and later-pass ones where
    # the stages loop - and keeps its bits
    out_r, act_r, off_r, _head, counts_r, ws_r = forward(net, obs[::-1], live[::-1], cap, integer)
    b, a = np.nonzero(live[::-1])
    back = torch.from_numpy(np.argsort((bs - 1 - b) * n + a, kind="stable")).cuda()        # reversed-call row of every row, in row order
    rep.true(f"reversed envs: rows processed {counts_r}", counts_r == want_counts and off_r[-1] == rows)
    same = (out_r[:rows][back] == out[:rows]).all(1)
    rep.true(f"reversed envs: {int((~same).sum())} of {rows} rows changed their bits", bool(same.all()))
    rep.true("reversed envs: actions changed", torch.equal(act_r[:rows][back], act[:rows]))
    rep.true("reversed envs: wrote past the rows", bool((out_r[rows:] == SENTINEL).all()) and bool((act_r[rows:] == ACT_FILL).all())
             and poisoned(ws_r[-TAIL:]))
    rep.done()
