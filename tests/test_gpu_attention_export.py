"""GPU tests of ``mel_forward_attention`` (csrc/attention_export.hpp): conv2's attention coefficients of the inference path,
read back from the workspace the agents forward left, against the references and bounds of tests/attention_record_ref.py - the
source sets bit for bit against the oracle's adjacency, the coefficients against the float64 softmax on the tapped rows, what
they aggregate to against the head input the forward itself wrote, and against the learn path's dense coefficients; guard rows
and a sentinel fill round the outputs; the node-feature table's forward gives the row lists' bits."""
import numpy as np
import pytest
import torch

from tests import attention_record_ref as ar

pytestmark = pytest.mark.gpu
SENTINEL, GUARD_ROWS, POISON = -12345.5, 3, 0xCD


def make_net(cell, dtype="f32"):
    from melissa_amd.networks import DGNRNetwork, LDGNNetwork
    hidden, heads, model, n, _bs = cell
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork}[model]
    duel = ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})
    net = cls(5, hidden, 2, heads, n, dueling_param=duel, device="cuda", backend="hip")
    net.load_state_dict(ar.weights(model, hidden, heads))
    return net.set_feature_dtype(dtype)


def export(net, cell, integer=False):
    """The agents forward on the cell's inputs into a poisoned workspace with a guard page, then mel_forward_attention into
    sentinel-filled buffers with guard rows -> (alpha [cap + guard, 34, H], sources uint64 [cap + guard, W], workspace, rows)."""
    hidden, heads, model, n, bs = cell
    obs, live = ar.cell_inputs(n, bs)
    cap, rows, W = bs * n, int(live.sum()), (n + 63) // 64
    mat = torch.from_numpy(obs[:, :-1].copy()).cuda()
    am = torch.from_numpy(ar.agent_words(live)).cuda()
    ws = torch.full((net.agents_workspace_bytes(bs, cap) + 4096,), POISON, dtype=torch.uint8, device="cuda")
    alpha = torch.full((cap + GUARD_ROWS, ar.MAX_SOURCES, heads), SENTINEL, device="cuda")
    sources = torch.full((cap + GUARD_ROWS, W), -7, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        _, off = net.hip_forward_agents(mat, am, cap, workspace=ws[:-4096], integer_features=integer)
        net.round_attention(ws[:-4096], bs, cap, alpha[:cap], sources[:cap])
    torch.cuda.synchronize()
    assert int(off[-1]) == rows
    assert bool((ws[-4096:] == POISON).all()), "the page behind the workspace was written"
    return alpha.cpu().numpy(), sources.cpu().numpy().view(np.uint64), ws, rows


def u1_rows(adj, live):
    """{(env, node): row of the packed U1 list} - conv1's targets, the agents' closed neighbourhoods, per env in node order."""
    closed = adj | np.eye(adj.shape[1], dtype=bool)[None]
    out, row = {}, 0
    for b in range(len(live)):
        for j in np.flatnonzero(closed[b, live[b]].any(0)):
            out[(b, int(j))] = row
            row += 1
    return out


CASES = [(c, "f32") for c in ar.CELLS] + [(ar.CELLS[0], "f32s"), (ar.CELLS[0], "f32a")]


@pytest.mark.parametrize("cell,dtype", CASES, ids=[f"{ar.cell_id(c)}-{d}" for c, d in CASES])
def test_coefficients_of_the_row_list_forward(cell, dtype):
    hidden, heads, model, n, bs = cell
    gat, hc = model == "l_dgn", hidden * heads
    obs, live = ar.cell_inputs(n, bs)
    net = make_net(cell, dtype)
    alpha, sources, ws, rows = export(net, cell)
    cap = bs * n
    pairs = ar.agent_rows(live)
    assert len(pairs) == rows
    adj = ar.adjacency(obs, n)
    src = ar.source_sets(adj, gat)
    # untouched: the rows from the live count on, the guard rows
    assert (alpha[rows:] == np.float32(SENTINEL)).all() and (sources[rows:].view(np.int64) == -7).all()
    xl2 = net.hip_stage_tap("xl2", bs, cap, workspace=ws[:-4096]).cpu().numpy()
    xr2 = net.hip_stage_tap("xr2", bs, cap, workspace=ws[:-4096]).cpu().numpy()
    head = net.hip_tap(1, bs, cap, workspace=ws[:-4096]).float().cpu().numpy()
    att = net.conv2.att.detach().reshape(-1).cpu().numpy() if gat else None
    bias = net.conv2.bias.detach().cpu().numpy() if gat else None
    u1 = u1_rows(adj, live)
    with torch.no_grad():
        dense = net.attention_weights(torch.from_numpy(obs).cuda(), layout="dense")[1].cpu().numpy()
    err_alpha = err_x3 = err_dense = 0.0
    for r, (b, i) in enumerate(pairs):
        js = np.flatnonzero(src[b, i])
        np.testing.assert_array_equal(sources[r], ar.pack(js, n), err_msg=f"sources of row {r} = env {b} agent {i}")
        c = len(js)
        assert (alpha[r, c:] == 0).all(), f"row {r}: slots past the source count"
        keys = np.stack([xl2[u1[(b, int(j))]] for j in js]) if c else np.zeros((0, xl2.shape[1]), dtype=np.float32)
        want = ar.alpha64(keys[:, :hc], xr2[r], att, heads)
        if c:
            err_alpha = max(err_alpha, float(np.abs(alpha[r, :c].astype(np.float64) - want).max()))
            err_dense = max(err_dense, float(np.abs(alpha[r, :c] - dense[b, i, js]).max()))
        else:
            assert not gat and not dense[b, i].any()
        x3 = ar.x3_64(alpha[r, :c], keys[:, -hc:], bias, heads)
        err_x3 = max(err_x3, float(np.abs(head[r, hidden + hc:] - x3).max()))
    print(f"{ar.cell_id(cell)} {dtype}: alpha - alpha64 {err_alpha:.3e} (bound {ar.ALPHA_TOL:.1e}), aggregated - x_3 {err_x3:.3e} "
          f"(bound {ar.X3_TOL:.1e}), alpha - learn path {err_dense:.3e} (bound {ar.ALPHA_TOL + ar.X3_TOL:.1e})")
    assert err_alpha <= ar.ALPHA_TOL
    assert err_x3 <= ar.X3_TOL
    assert err_dense <= ar.ALPHA_TOL + ar.X3_TOL
    counts = src[tuple(np.asarray(pairs).T)].sum(1) if pairs else np.zeros(0)
    assert counts.max() >= 3 and (n < 64 or counts.max() == ar.MAX_SOURCES)


def test_the_node_feature_table_forward_gives_the_row_lists_bits():
    cell = ar.TABLE_CELL
    _hidden, _heads, _model, n, bs = cell
    net = make_net(cell)
    a_rows, s_rows, ws, rows = export(net, cell, integer=False)
    assert int(net.hip_tap(3, bs, bs * n, workspace=ws[:-4096])[0]) == 0
    a_table, s_table, ws, rows_t = export(net, cell, integer=True)
    assert int(net.hip_tap(3, bs, bs * n, workspace=ws[:-4096])[0]) > 0, "the forward did not take the node-feature table"
    assert rows_t == rows and rows > bs
    np.testing.assert_array_equal(a_table.view(np.uint32), a_rows.view(np.uint32))
    np.testing.assert_array_equal(s_table, s_rows)
    assert (a_rows[:rows].sum(1) > 0.999).all()


def test_hl_dgn_and_bf16_are_refused():
    from melissa_amd.networks import HLDGNNetwork
    cell = ar.CELLS[0]
    net = make_net(cell, "bf16")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    alpha, sources = torch.zeros(48, ar.MAX_SOURCES, 4, device="cuda"), torch.zeros(48, 1, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="bf16"):
        net.round_attention(ws, 4, 48, alpha, sources)
    hl = HLDGNNetwork(5, 128, 2, 4, 12, dueling_param=({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]}), device="cuda",
                      backend="hip")
    with pytest.raises(RuntimeError, match="second convolution"):
        hl.round_attention(ws, 4, 48, alpha, sources)
