"""GPU tests of the attention launches' source walk (csrc/attention.hpp): the list walk - the target's source list built once,
two row indices per online-softmax step read from it - against the walk it replaced, which picked its sources off the node set
in every step.  Both ran the same arithmetic on the same sources in the same order, so the bar is BYTE EQUALITY of the logits and
of the head input (mel_forward_tap kind 1): row lists and the node-feature table, fp32 / split / bf16 features, one- and two-word
node sets, DGN-R (a target may have no source), the HL-DGN pool kernel, and shapes off the compile-time forms (4 channels per
lane; 16 and 32 lanes per head), which take the generic list walk.

The former walk is gone from the tree; its answer is held by tests/golden/attention_walk_bits.npz: one zlib.crc32 per output row
of every case below, recorded by tests/golden/make_attention_walk_golden.py IN A CHECKOUT OF THE COMMIT BEFORE THE DELETION with
that commit's environment switch for the former walk set (the file names the commit and the switch; NOTES.md, "The attention
launches' source walk").  The recorder imports the cases and input builders of this module and has no walk-specific code of its own.  The fixture is re-recorded only by a change that alters the forward's arithmetic
on purpose, and then from that change's PARENT commit - never from the tree under test.

The generic-form shapes had no GPU test before they were recorded, so their logits are also held to oracle.net_oracle at 1e-4."""
import os
import zlib
from typing import NamedTuple

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})
TABLE_ENVS = 192        # envs from which the agents forward takes the node-feature table at every n used here (fwd.hip: the
                        # expected row lists reach twice the n * 40 tuples at 40 / 119 / 153 / 168 envs for n = 7 / 20 / 50 / 100)
TABLE_FROM = {7: 40, 20: 119, 50: 153, 100: 168}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_walk_bits.npz")
TOL = 1e-4              # the project's bar against the oracle
ARRAYS = ("logits", "head_input")


class Case(NamedTuple):
    model: str
    dtype: str
    n: int
    bs: int
    table: bool             # integer_features: the forward may take the node-feature table
    prepared: bool = False
    hidden: int = 128
    heads: int = 4
    agg: str = "max"        # HL-DGN

    @property
    def key(self):
        return (f"{self.model}-{self.dtype}-h{self.hidden}x{self.heads}-n{self.n}-bs{self.bs}-{'int' if self.table else 'rows'}"
                f"{'-prepared' if self.prepared else ''}{'-' + self.agg if self.model == 'hl_dgn' else ''}")


SIZES = [(7, 8), (20, 5), (50, 3), (100, 4)]
ROW_LISTS = [Case("l_dgn", "f32", n, bs, False) for n, bs in SIZES]
PREPARED_SMALL = [Case("l_dgn", "f32", n, bs, True, prepared=True) for n, bs in SIZES]
TABLE_MODE = [Case("l_dgn", "f32", n, TABLE_ENVS, True, prepared=p) for p in (False, True) for n in (7, 20, 50, 100)]
OTHER_PRECISIONS = [Case("l_dgn", dtype, n, bs, table) for dtype, n, bs, table in
                    [("f32s", 20, 6, False), ("f32s", 50, 4, False), ("f32a", 50, TABLE_ENVS, True),
                     ("bf16", 20, 6, False), ("bf16", 100, 3, False), ("bf16", 50, TABLE_ENVS, True)]]
DGNR = [Case("dgn_r", dtype, 20, bs, table) for dtype, bs, table in [("f32", 6, False), ("bf16", 6, False), ("f32", TABLE_ENVS, True)]]
HLDGN_POOL = [Case("hl_dgn", "f32a", 20, bs, table, agg=agg) for bs, table in [(7, False), (512, True)] for agg in ("max", "mean")]
# 4 channels per lane: the generic list walk (ATT_WALK_GENERIC), with 16 (64 x 4) and 32 (128 x 2) lanes per head.  (7, 48): past
# the 40 envs from which n = 7 takes the table - hidden 64 is not the width the one-launch table is built for, so the two-launch one
GENERIC = ([Case("l_dgn", "f32", n, bs, False, hidden=h, heads=k) for h, k in [(64, 4), (128, 2)] for n, bs in [(7, 8), (20, 5)]] +
           [Case("l_dgn", "f32", 7, 48, True, hidden=64, heads=4), Case("dgn_r", "f32", 20, 6, False, hidden=64, heads=4)])
CASES = ROW_LISTS + PREPARED_SMALL + TABLE_MODE + OTHER_PRECISIONS + DGNR + HLDGN_POOL + GENERIC


def make(model, n, agg="max", seed=9, hidden=128, heads=4):
    """The network with oracle.net_oracle's weights; the dueling heads keep their hidden sizes, their input width follows
    hidden and heads."""
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    sd = no.init_weights(model, hidden=hidden, heads=heads, seed=seed, random_conv_bias=True)
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[model]
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    net = cls(5, hidden, 2, heads, n, dueling_param=DUEL(), device="cuda", backend="hip", **kw)
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


def row_checksums(a):
    """one zlib.crc32 per row of a raw() array"""
    a = np.ascontiguousarray(a)
    return np.array([zlib.crc32(row.tobytes()) for row in a.reshape(a.shape[0], -1)], dtype=np.uint32)


def source_counts(net, bs, cap, gat):
    """sources per target of the last forward, from the adjacency tap (GATv2 adds the self loop)"""
    adj = net.hip_tap(0, bs, cap).cpu().numpy().astype(np.uint64).reshape(bs, net.agents_num, -1)
    cnt = np.zeros(adj.shape[:2], dtype=np.int64)
    for w in range(adj.shape[2]):
        cnt += np.array([[bin(int(x)).count("1") for x in row] for row in adj[:, :, w]])
    return cnt + (1 if gat else 0)


def run_agents(c):
    net = make(c.model, c.n, hidden=c.hidden, heads=c.heads)
    net.set_feature_dtype(c.dtype)
    net.prepared_tables = c.prepared
    n, bs, cap = c.n, c.bs, c.bs * c.n
    mat, am = build_inputs(n, bs, 100 * n + bs)
    obs = torch.from_numpy(mat.reshape(bs, n * 8)).cuda()
    with torch.no_grad():
        logits, off = net.hip_forward_agents(obs, torch.from_numpy(am).cuda(), cap, integer_features=c.table)
        rows = int(off[-1])
        took_table = int(net.hip_tap(3, bs, cap)[0]) > 0
        out = [raw(logits[:rows]), raw(net.hip_tap(1, bs, cap)[:rows])]
    assert rows >= n + 1                                        # env 0: one row, env 2: n rows
    assert took_table == (c.table and bs >= TABLE_FROM[n])
    cnt = source_counts(net, bs, cap, gat=c.model == "l_dgn")
    assert (cnt % 2 == 1).any() and (cnt % 2 == 0).any()        # odd and even source counts
    assert cnt[0, 0] == (1 if c.model == "l_dgn" else 0)        # the isolated agent of env 0
    if n >= 40:
        assert cnt[1, :36].max() >= 33                          # a target at the neighbour cap
    assert np.isfinite(out[0].view(np.float32)).all()
    return out


def run_pool(c):
    net = make("hl_dgn", c.n, agg=c.agg, hidden=c.hidden, heads=c.heads)
    net.set_feature_dtype(c.dtype)
    mat, _ = build_inputs(c.n, c.bs, 31 + c.bs)
    obs = torch.from_numpy(mat.reshape(c.bs, c.n * 8)).cuda()
    with torch.no_grad():
        logits = net.hip_forward_envs(obs, integer_features=c.table)
        out = [raw(logits), raw(net.hip_tap(1, c.bs))]
        assert (int(net.hip_tap(3, c.bs)[0]) > 0) == c.table
    return out


def run_case(c):
    """One forward of the case with its structural assertions -> {array name: raw bits}.  The recorder stores row_checksums()
    of exactly this."""
    return dict(zip(ARRAYS, run_pool(c) if c.model == "hl_dgn" else run_agents(c)))


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def check(c, golden):
    got = run_case(c)
    for name in ARRAYS:
        a = got[name]
        assert list(a.shape) == list(golden[f"{c.key}/{name}/shape"]) and str(a.dtype) == str(golden[f"{c.key}/{name}/dtype"]), \
            (c.key, name, a.shape, a.dtype)
        differ = np.flatnonzero(row_checksums(a) != golden[f"{c.key}/{name}/crc"])
        assert differ.size == 0, (f"{c.key}: {differ.size} of {a.shape[0]} rows of {name} differ from the bits recorded at "
                                  f"{golden['commit']} ({golden['label']}); the first: {differ[:8].tolist()}")
    return got


def ids(fmt):
    return lambda c: fmt.format(c=c, prepared="prepared" if c.prepared else "per_call")


@pytest.mark.parametrize("case", ROW_LISTS, ids=ids("{c.n}-{c.bs}"))
def test_ldgn_f32_row_lists(case, golden):
    check(case, golden)


@pytest.mark.parametrize("case", PREPARED_SMALL, ids=ids("{c.n}-{c.bs}"))
def test_ldgn_f32_prepared_tables_small_batches(case, golden):
    """The configurations above with integer features and prepared tables: at this size the forward keeps the row lists."""
    check(case, golden)


@pytest.mark.parametrize("case", TABLE_MODE, ids=ids("{c.n}-{prepared}"))
def test_ldgn_f32_table_mode(case, golden):
    """... and with enough envs for the forward to take the table: the attention gathers its rows by tuple id."""
    check(case, golden)


@pytest.mark.parametrize("case", OTHER_PRECISIONS, ids=ids("{c.dtype}-{c.n}-{c.bs}-{c.table}"))
def test_ldgn_other_precisions(case, golden):
    check(case, golden)


@pytest.mark.parametrize("case", DGNR, ids=ids("{c.dtype}-{c.bs}-{c.table}"))
def test_dgnr_with_an_isolated_target(case, golden):
    check(case, golden)


@pytest.mark.parametrize("case", HLDGN_POOL, ids=ids("{c.agg}-{c.bs}-{c.table}"))
def test_hldgn_pool(case, golden):
    check(case, golden)


@pytest.mark.parametrize("case", GENERIC, ids=ids("{c.model}-{c.hidden}x{c.heads}-{c.n}-{c.bs}-{c.table}"))
def test_generic_walk_shapes(case, golden):
    """Shapes no other GPU test runs: the recorded bits, and the logits within 1e-4 of the oracle."""
    from oracle import net_oracle as no
    c = case
    got = check(c, golden)["logits"].view(np.float32)
    mat, am = build_inputs(c.n, c.bs, 100 * c.n + c.bs)
    rows = [(b, a) for b in range(c.bs) for a in range(c.n) if (int(am[b]) >> a) & 1]      # n <= 64 here: one word per env
    obs_rows = np.concatenate([mat.reshape(c.bs, -1)[[b for b, _ in rows]], np.array([[a] for _, a in rows], dtype=np.float32)], axis=1)
    sd = no.init_weights(c.model, hidden=c.hidden, heads=c.heads, seed=9, random_conv_bias=True)
    with torch.no_grad():
        want = (no.ldgn_forward if c.model == "l_dgn" else no.dgnr_forward)(sd, obs_rows, c.n, heads=c.heads).numpy()
    err = np.abs(got - want).max()
    print(f"{c.key}: max |logits - oracle| = {err:.3g}")
    assert got.shape == want.shape and err < TOL, (c.key, err)


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
