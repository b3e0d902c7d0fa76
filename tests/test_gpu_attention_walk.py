"""GPU tests of the attention launches' source walk (csrc/attention.hpp): the list walk - the target's source list built once,
two row indices per online-softmax step read from it - against the walk it replaces (MEL_FWD_ATT_LEGACY_WALK), in one process.
Both run the same arithmetic on the same sources in the same order, so the bar is BYTE EQUALITY of the logits and of the head
input (mel_forward_tap kind 1): row lists and the node-feature table, fp32 / split / bf16 features, one- and two-word node sets,
DGN-R (a target may have no source) and the HL-DGN pool kernel."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})
TABLE_ENVS = 192        # envs from which the agents forward takes the node-feature table at every n used here (fwd.hip: the
                        # expected row lists reach twice the n * 40 tuples at 40 / 119 / 153 / 168 envs for n = 7 / 20 / 50 / 100)


def make(model, n, agg="max", seed=9):
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    sd = no.init_weights(model, seed=seed, random_conv_bias=True)
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    net = cls(5, 128, 2, 4, n, dueling_param=DUEL(), device="cuda", backend="hip", **kw)
    net.load_state_dict(sd)
    return net


def build_inputs(n, bs, seed):
    """Env-like observation matrices [bs, n, 8] (integer features: the table can take them) and agent sets [bs, words] with
    env 0: a single agent, node 0, ISOLATED in a corner (DGN-R: a target without a source; GATv2: the self loop alone, odd);
    env 1: (n >= 40) nodes 0 .. 35 inside a 0.05 box - a clique past the 32-neighbour cap -, the rest spread out;
    env 2: every node an agent; the others: a random subset, so agent and non-agent rows share an env."""
    rng = np.random.RandomState(seed)
    m = np.zeros((bs, n, 8), dtype=np.float32)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, n, size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.1)
    m[0, :, 0:2] = rng.uniform(0.5, 1, size=(n, 2))
    m[0, 0, 0:2] = 0.0
    if n >= 40:
        m[1, :36, 0:2] = 0.4 + rng.uniform(0, 0.05, size=(36, 2))
    words = (n + 63) // 64
    masks = np.zeros((bs, words), dtype=np.uint64)
    for b in range(bs):
        agents = [0] if b == 0 else (range(n) if b == 2 else rng.choice(n, size=rng.randint(1, max(2, n // 3) + 1), replace=False))
        for a in agents:
            masks[b, int(a) // 64] |= np.uint64(1) << np.uint64(int(a) % 64)
    am = masks.view(np.int64)
    return m, (am[:, 0].copy() if words == 1 else am)


def raw(t):
    """the bits of a tensor (bf16 rows as int16)"""
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu().numpy()


def both_walks(net, run):
    """run() under the list walk and under the legacy flag -> two lists of raw arrays"""
    out = []
    for legacy in (False, True):
        net.attention_legacy_walk = legacy
        with torch.no_grad():
            out.append(run())
    net.attention_legacy_walk = False
    return out


def agents_run(net, mat, am, table):
    bs, n = mat.shape[0], mat.shape[1]
    cap = bs * n
    obs = torch.from_numpy(mat.reshape(bs, n * 8)).cuda()
    amt = torch.from_numpy(am).cuda()

    def run():
        logits, off = net.hip_forward_agents(obs, amt, cap, integer_features=table)
        rows = int(off[-1])
        took_table = int(net.hip_tap(3, bs, cap)[0]) > 0
        return [raw(logits[:rows]), raw(net.hip_tap(1, bs, cap)[:rows])], rows, took_table
    return run


def source_counts(net, bs, cap, gat):
    """sources per target of the last forward, from the adjacency tap (GATv2 adds the self loop)"""
    adj = net.hip_tap(0, bs, cap).cpu().numpy().astype(np.uint64).reshape(bs, net.agents_num, -1)
    cnt = np.zeros(adj.shape[:2], dtype=np.int64)
    for w in range(adj.shape[2]):
        cnt += np.array([[bin(int(x)).count("1") for x in row] for row in adj[:, :, w]])
    return cnt + (1 if gat else 0)


def check_agents(model, dtype, n, bs, table, prepared=False):
    net = make(model, n)
    net.set_feature_dtype(dtype)
    net.prepared_tables = prepared
    mat, am = build_inputs(n, bs, 100 * n + bs)
    (new, rows_new, table_new), (old, rows_old, table_old) = both_walks(net, agents_run(net, mat, am, table))
    assert rows_new == rows_old and rows_new >= n + 1           # env 0: one row, env 2: n rows
    assert table_new == table_old == (table and bs >= TABLE_ENVS)
    cnt = source_counts(net, bs, bs * n, gat=model == "l_dgn")
    assert (cnt % 2 == 1).any() and (cnt % 2 == 0).any()        # odd and even source counts
    assert cnt[0, 0] == (1 if model == "l_dgn" else 0)          # the isolated agent of env 0
    if n >= 40:
        assert cnt[1, :36].max() >= 33                          # a target at the neighbour cap
    for a, b in zip(new, old):
        np.testing.assert_array_equal(a, b)
    assert np.isfinite(new[0].view(np.float32)).all()


@pytest.mark.parametrize("n,bs", [(7, 8), (20, 5), (50, 3), (100, 4)])
def test_ldgn_f32_row_lists(n, bs):
    check_agents("l_dgn", "f32", n, bs, table=False)


@pytest.mark.parametrize("n,bs", [(7, 8), (20, 5), (50, 3), (100, 4)])
def test_ldgn_f32_prepared_tables_small_batches(n, bs):
    """The configurations above with integer features and prepared tables: at this size the forward keeps the row lists."""
    check_agents("l_dgn", "f32", n, bs, table=True, prepared=True)


@pytest.mark.parametrize("prepared", [False, True], ids=["per_call", "prepared"])
@pytest.mark.parametrize("n", [7, 20, 50, 100])
def test_ldgn_f32_table_mode(n, prepared):
    """... and with enough envs for the forward to take the table: the attention gathers its rows by tuple id."""
    check_agents("l_dgn", "f32", n, TABLE_ENVS, table=True, prepared=prepared)


@pytest.mark.parametrize("dtype,n,bs,table", [("f32s", 20, 6, False), ("f32s", 50, 4, False), ("f32a", 50, TABLE_ENVS, True),
                                             ("bf16", 20, 6, False), ("bf16", 100, 3, False), ("bf16", 50, TABLE_ENVS, True)])
def test_ldgn_other_precisions(dtype, n, bs, table):
    check_agents("l_dgn", dtype, n, bs, table)


@pytest.mark.parametrize("dtype,bs,table", [("f32", 6, False), ("bf16", 6, False), ("f32", TABLE_ENVS, True)])
def test_dgnr_with_an_isolated_target(dtype, bs, table):
    check_agents("dgn_r", dtype, 20, bs, table)


@pytest.mark.parametrize("bs,table", [(7, False), (512, True)])
@pytest.mark.parametrize("agg", ["max", "mean"])
def test_hldgn_pool(agg, bs, table):
    n = 20
    net = make("hl_dgn", n, agg=agg)
    mat, _ = build_inputs(n, bs, 31 + bs)
    obs = torch.from_numpy(mat.reshape(bs, n * 8)).cuda()

    def run():
        logits = net.hip_forward_envs(obs, integer_features=table)
        return [raw(logits), raw(net.hip_tap(1, bs))], int(net.hip_tap(3, bs)[0]) > 0
    (new, table_new), (old, table_old) = both_walks(net, run)
    assert table_new == table_old == table
    for a, b in zip(new, old):
        np.testing.assert_array_equal(a, b)


def test_graph_replay_equals_eager():
    n, bs = 20, 6
    net = make("l_dgn", n)
    mat, am = build_inputs(n, bs, 77)
    cap = bs * n
    obs = torch.from_numpy(mat.reshape(bs, n * 8)).cuda()
    amt = torch.from_numpy(am).cuda()
    with torch.no_grad():
        eager, off = net.hip_forward_agents(obs, amt, cap)
        rows = int(off[-1])
        eager, eager_cat = raw(eager[:rows]), raw(net.hip_tap(1, bs, cap)[:rows])
        out = torch.zeros(cap, net.output_dim, device="cuda")
        offsets = torch.zeros(bs + 1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            net.hip_forward_agents(obs, amt, cap, out=out, row_offsets=offsets)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert int(offsets[-1]) == rows
        np.testing.assert_array_equal(raw(out[:rows]), eager)
        np.testing.assert_array_equal(raw(net.hip_tap(1, bs, cap)[:rows]), eager_cat)
