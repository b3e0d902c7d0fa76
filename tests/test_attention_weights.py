"""The exported attention coefficients without a GPU: ``GraphQNetwork.attention_weights`` on the torch backend against a float64
reference of alpha evaluated on the network's own projections, the structure of the coefficients (zeros off the sources, rows
that sum to one, zero rows of isolated TransformerConv targets), the dense -> edge conversion, and the two ``watch`` flags.

``alpha_ref`` is the formula of tests/learn_ref.py:attention_ref up to its line ``alpha = ...``; tests/test_gpu_attention_weights.py
holds the kernel to the same function."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from melissa_amd import watch
from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork, common
from tests import learn_ref as lr

MODELS = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}


def alpha_ref(kind, xl, xr, att, adj_bool, heads, dtype):
    """alpha [bs, n (target i), n (source j), H] in ``dtype``: GATv2 over the closed neighbourhood with e_ij = att .
    leaky_relu(x_r[i] + x_l[j], 0.2), Transformer over the open one with e_ij = q[i] . k[j] / sqrt(C) (xl = keys, xr = queries);
    softmax over the sources with 1e-16 added to the denominator, 0 off the sources, a target without a source all zero."""
    bs, n, _ = adj_bool.shape
    c = xl.shape[1] // heads
    xl, xr = xl.detach().to(dtype), xr.detach().to(dtype)
    zero = torch.zeros((), dtype=dtype)
    eye = torch.eye(n, dtype=torch.bool)
    out = []
    for b in range(bs):
        sl = slice(b * n, (b + 1) * n)
        src, tgt = xl[sl].view(n, heads, c), xr[sl].view(n, heads, c)
        if kind == lr.GATV2:
            mask = (adj_bool[b] | eye)[..., None]
            e = (F.leaky_relu(tgt[:, None] + src[None, :], 0.2) * att.detach().to(dtype).view(heads, c)).sum(-1)      # [i, j, H]
        else:
            mask = adj_bool[b][..., None]
            e = torch.einsum("ihc,jhc->ijh", tgt, src) / math.sqrt(c)
        e = e.masked_fill(~mask, -float("inf"))
        top = e.max(dim=1, keepdim=True).values
        top = torch.where(torch.isfinite(top), top, zero)                    # a target without a source
        p = torch.where(mask, torch.exp(e - top), zero)
        out.append(p / (p.sum(dim=1, keepdim=True) + 1e-16))
    return torch.stack(out)


def sources(kind, adj_bool):
    """bool [bs, n, n]: j is a source of i for this conv kind."""
    return adj_bool | torch.eye(adj_bool.shape[1], dtype=torch.bool) if kind == lr.GATV2 else adj_bool


def check_structure(alpha, kind, adj_bool, what=""):
    """Exact zeros off the sources, rows with a source sum to 1 within 1e-6, rows without one are all zero."""
    src = sources(kind, adj_bool)
    alpha = alpha.cpu()
    assert not alpha[~src].any(), f"{what}: a non-source entry is not 0.0"
    has = src.any(dim=2)
    sums = alpha.double().sum(dim=2)                                        # [bs, n, H]
    assert float((sums[has] - 1.0).abs().max() if has.any() else 0.0) <= 1e-6, what
    assert not alpha[~has].any(), f"{what}: a target without a source has a non-zero row"


def random_obs(n, bs, seed):
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


def make_net(model, n, hidden, heads, device="cpu", backend="torch"):
    torch.manual_seed(11 + heads)
    kw = dict(aggregator="max") if model == "hl_dgn" else {}
    net = MODELS[model](5, hidden, 2, heads, n, dueling_param=({"hidden_sizes": [hidden]}, {"hidden_sizes": [hidden]}),
                        device=device, backend=backend, **kw)
    with torch.no_grad():
        for conv in (net.conv1, getattr(net, "conv2", None)):
            if isinstance(conv, common.GATv2Conv):
                conv.bias.uniform_(-0.1, 0.1)
    return net.eval()


def conv_operands(net, obs):
    """Per convolution (kind, xl, xr, att) - the network's own fp32 projections of the full-graph formulation in plain torch
    ops on the network's device - and the bool adjacency, all on the host."""
    obs = torch.as_tensor(obs).to(net.device)
    pos, feats, dm, _g = common.unpack(obs, net.input_dim, net.agents_num)
    bs, n = pos.shape[:2]
    adj = common.radius_adjacency(pos)
    ops = []
    with torch.no_grad():
        x = F.relu(net.encoder.model(feats.reshape(bs * n, -1)))
        for k, conv in enumerate((net.conv1, getattr(net, "conv2", None))):
            if conv is None:
                break
            if k == 1:
                x = common.conv_relu(net.conv1, x, adj, n, False) * dm.reshape(bs * n, 1)
            if isinstance(conv, common.TransformerConv):
                ops.append((lr.TRANSFORMER, conv.lin_key(x), conv.lin_query(x), None))
            else:
                ops.append((lr.GATV2, conv.lin_l(x), conv.lin_r(x), conv.att.reshape(-1)))
    return [tuple(t.cpu() if torch.is_tensor(t) else t for t in op) for op in ops], adj.cpu()


@pytest.mark.parametrize("heads", [2, 6])
@pytest.mark.parametrize("model", list(MODELS))
def test_torch_backend_matches_float64_on_its_own_projections(model, heads):
    n, bs = 20, 6
    net = make_net(model, n, 64, heads)
    obs = random_obs(n, bs, 5)
    got = net.attention_weights(obs)
    ops, adj = conv_operands(net, obs)
    assert len(got) == len(ops) == (1 if model == "hl_dgn" else 2)
    assert int((adj.sum(2) == 0).sum()) > 0 and int(adj.sum()) > 0            # isolated targets and edges both occur
    for k, (alpha, (kind, xl, xr, att)) in enumerate(zip(got, ops)):
        assert alpha.dtype == torch.float32 and tuple(alpha.shape) == (bs, n, n, heads) and not alpha.requires_grad
        want = alpha_ref(kind, xl, xr, att, adj, heads, torch.float64)
        err32 = float((alpha_ref(kind, xl, xr, att, adj, heads, torch.float32).double() - want).abs().max())
        err = float((alpha.double() - want).abs().max())
        limit = lr.bar(want, err32)
        print(f"{model} heads {heads} conv{k + 1}: max error {err:.1e} (reference in fp32: {err32:.1e}, bar {limit:.1e})")
        assert err <= limit
        check_structure(alpha, kind, adj, f"{model} conv{k + 1}")
        if kind == lr.TRANSFORMER:
            assert not alpha[adj.sum(2) == 0].any()                          # isolated targets: all-zero rows
        else:
            assert bool((alpha.diagonal(dim1=1, dim2=2) > 0).all())            # the self-loop always takes part


def test_index_column_and_gradient_mode_do_not_matter():
    net = make_net("l_dgn", 20, 64, 2)
    obs = random_obs(20, 3, 8)
    other = obs.copy()
    other[:, -1] = (other[:, -1] + 7) % 20
    with torch.enable_grad():
        a = net.attention_weights(obs)
    b = net.attention_weights(torch.from_numpy(other))
    for x, y in zip(a, b):
        assert torch.equal(x, y) and not x.requires_grad
    with pytest.raises(ValueError):
        net.attention_weights(obs, layout="coo")


@pytest.mark.parametrize("kind", [lr.GATV2, lr.TRANSFORMER], ids=["gatv2", "transformer"])
def test_dense_formulations_keep_their_bits(kind):
    """``gatv2_dense`` / ``transformer_dense`` share their alpha with the export now: the same bits as the formulation written
    out in one piece (what the functions were)."""
    spec, heads, c = ("radius", 40, 2, 0.25), 4, 8
    adj = lr.graph(spec)
    bs, n, _ = adj.shape
    torch.manual_seed(3)
    x = torch.randn(bs * n, 16)
    if kind == lr.GATV2:
        conv = common.GATv2Conv(16, c, heads)
        with torch.no_grad():
            conv.bias.uniform_(-0.1, 0.1)
        x_l, x_r = conv.lin_l(x).view(bs, n, heads, c), conv.lin_r(x).view(bs, n, heads, c)
        mask = adj | torch.eye(n, dtype=torch.bool)[None]
        e = (F.leaky_relu(x_r[:, :, None] + x_l[:, None, :], 0.2) * conv.att[0]).sum(-1)
        e = e.masked_fill(~mask[..., None], -float("inf"))
        p = torch.exp(e - e.max(dim=2, keepdim=True).values)
        p = torch.where(mask[..., None], p, torch.zeros(()))
        alpha = p / (p.sum(dim=2, keepdim=True) + 1e-16)
        want = torch.einsum("bijh,bjhc->bihc", alpha, x_l).reshape(bs * n, heads * c) + conv.bias
        assert torch.equal(common.gatv2_dense(conv, x, adj), want)
        assert torch.equal(common.gatv2_alpha(conv.att[0], x_l, x_r, adj), alpha)
    else:
        conv = common.TransformerConv(16, c, heads)
        q, k, v = (lin(x).view(bs, n, heads, c) for lin in (conv.lin_query, conv.lin_key, conv.lin_value))
        e = torch.einsum("bihc,bjhc->bijh", q, k) / math.sqrt(c)
        e = e.masked_fill(~adj[..., None], -float("inf"))
        e_max = e.max(dim=2, keepdim=True).values
        e_max = torch.where(torch.isfinite(e_max), e_max, torch.zeros(()))
        p = torch.where(adj[..., None], torch.exp(e - e_max), torch.zeros(()))
        alpha = p / (p.sum(dim=2, keepdim=True) + 1e-16)
        want = torch.einsum("bijh,bjhc->bihc", alpha, v).reshape(bs * n, heads * c)
        assert torch.equal(common.transformer_dense(conv, x, adj), want)
        assert torch.equal(common.transformer_alpha(k, q, adj), alpha)


# ---- edge layout -----------------------------------------------------------------------------------------------------
def scatter_back(edge_index, alpha, bs, n):
    """(edge_index [2, E], alpha [E, H]) -> dense [bs, n, n, H] (zeros elsewhere); every edge must land in its own graph."""
    src, tgt = edge_index
    assert torch.equal(src // n, tgt // n)
    dense = torch.zeros(bs, n, n, alpha.shape[1], dtype=alpha.dtype)
    dense[tgt // n, tgt % n, src % n] = alpha
    return dense


@pytest.mark.parametrize("self_loops", [True, False], ids=["gatv2", "transformer"])
def test_dense_to_edges_on_a_hand_built_graph(self_loops):
    bs, n, h = 2, 3, 2
    adj = torch.zeros(bs, n, n, dtype=torch.bool)
    adj[0, 0, 2] = adj[0, 0, 1] = adj[0, 2, 0] = True                         # graph 0: 1 -> 0, 2 -> 0, 0 -> 2
    adj[1, 1, 0] = adj[1, 2, 1] = True                                       # graph 1: 0 -> 1, 1 -> 2
    alpha = torch.arange(bs * n * n * h, dtype=torch.float32).view(bs, n, n, h) + 1.0
    mask = adj | torch.eye(n, dtype=torch.bool) if self_loops else adj
    alpha = alpha * mask[..., None]
    edge_index, a = common.dense_to_edges(alpha, adj, self_loops)
    src, tgt = [1, 2, 0, 3, 4], [0, 0, 2, 4, 5]                               # by target, then by source; ids offset by b * n
    if self_loops:                                                           # then the bs * n loops in node order
        src, tgt = src + list(range(6)), tgt + list(range(6))
    assert edge_index.dtype == torch.int64 and edge_index.tolist() == [src, tgt]
    assert tuple(a.shape) == (len(src), h)
    for e, (s, t) in enumerate(zip(src, tgt)):
        assert torch.equal(a[e], alpha[t // n, t % n, s % n])
    assert torch.equal(scatter_back(edge_index, a, bs, n), alpha)


@pytest.mark.parametrize("model", list(MODELS))
def test_edge_layout_of_a_network_agrees_with_the_dense_one(model):
    n, bs = 20, 6
    net = make_net(model, n, 64, 2)
    obs = random_obs(n, bs, 6)
    dense, edges = net.attention_weights(obs), net.attention_weights(obs, layout="edges")
    adj = common.radius_adjacency(common.unpack(torch.from_numpy(obs), 5, n)[0])
    b, i, j = adj.nonzero(as_tuple=True)
    loops = torch.arange(bs * n)
    assert len(dense) == len(edges)
    for k, (alpha, (edge_index, a)) in enumerate(zip(dense, edges)):
        gat = isinstance(getattr(net, f"conv{k + 1}"), common.GATv2Conv)
        want_src, want_tgt = b * n + j, b * n + i
        if gat:
            want_src, want_tgt = torch.cat([want_src, loops]), torch.cat([want_tgt, loops])      # self-loops last
        assert torch.equal(edge_index, torch.stack([want_src, want_tgt]))
        body = edge_index[:, :len(b)]
        key = body[1] * (bs * n) + body[0]
        assert bool((key[1:] > key[:-1]).all())                               # sorted by target, then by source
        assert torch.equal(scatter_back(edge_index, a, bs, n), alpha)          # exactly the dense form


# ---- parsers ---------------------------------------------------------------------------------------------------------
# what watch.parse_args([]) gave before the two flags existed
WATCH_DEFAULTS = dict(model="l_dgn", nodes=20, envs=1, episodes=10, load=None, graphs=16, graph_pool=None, dtype="f32",
                      heuristic=None, scripted_agents_ratio=0.0, spread=False, collect_stats="episodes", hidden_emb=128,
                      num_heads=4, dueling_q_hidden_sizes=[128, 128], dueling_v_hidden_sizes=[128, 128],
                      aggregator_function="max")


def test_watch_parsers_take_the_attention_flags():
    for parse in (watch.parse_args, watch.arg_parser().parse_args):
        a = vars(parse([]))
        assert a.pop("attention_out") is None and a.pop("attention_rounds") == 8
        assert a == WATCH_DEFAULTS                                           # without them: what it gave
        a = parse(["--attention-out", "alpha.npz", "--attention-rounds", "3", "--envs", "2"])
        assert (a.attention_out, a.attention_rounds, a.envs) == ("alpha.npz", 3, 2)
        rest = {k: v for k, v in vars(a).items() if k not in ("attention_out", "attention_rounds", "envs")}
        assert rest == {k: v for k, v in WATCH_DEFAULTS.items() if k != "envs"}
    with pytest.raises(SystemExit):
        watch.parse_args(["--attention-out", "alpha.npz", "--attention-rounds", "0"])
