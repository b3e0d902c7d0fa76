"""GPU test of the forward's HOST side (csrc/fwd.hip: the code that describes each projection's GEMM problem and issues the
launches): every route a forward can take, launch for launch and bit for bit against tests/golden/forward_paths_parent.npz.

The fixture holds what the commit BEFORE the launch sites were merged into shared builders computed and launched (the file names
the commit), recorded by tests/golden/make_forward_paths_golden.py in a checkout of that commit with this module copied in -
never from the tree under test.  It is re-recorded only by a change that alters what a forward launches or computes on purpose,
and then from that change's parent.

Per case and entry point: the logits as int32 words, the row offsets of the agents entry point, the node-feature table rows the
forward used (hip_tap 3: a table case that fell back to the row lists would still give the right logits) and the launch groups
per stage from the library's stage timer.  The cases are the smallest shapes that reach each launch site: row lists at
n = 20 / 3 envs, the table at n = 7 / 96 envs (T = 280 tuples; the L-DGN entries expect 2 * 96 * 7 = 1344 >= 2 T rows, HL-DGN has
672 >= 560), evaluated per call and prepared, two-word node sets (n = 70), the 512-wide encoder, six heads, one head without
dueling."""
import os
from typing import NamedTuple

import numpy as np
import pytest
import torch

from tests.test_gpu_table_fused import agent_sets, env_like_obs, launches_by_stage

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_paths_parent.npz")
MODELS = ("l_dgn", "dgn_r", "hl_dgn")
ROWS, TABLE = (20, 3), (7, 96)          # (n, envs) of the two routes


class Case(NamedTuple):
    model: str
    dtype: str
    n: int
    bs: int
    integer: bool               # integer_features: the forward may take the node-feature table (it does at TABLE, not at ROWS)
    prepared: bool = False
    hidden: int = 128
    heads: int = 4
    dueling: bool = True

    @property
    def key(self):
        return (f"{self.model}-{self.dtype}-h{self.hidden}x{self.heads}-n{self.n}-bs{self.bs}-{'int' if self.integer else 'rows'}"
                f"{'-prepared' if self.prepared else ''}{'' if self.dueling else '-single_head'}")

    @property
    def table_rows(self):
        return 40 * self.n if self.integer else 0


ROWS_ROUTE = [Case(m, d, *ROWS, False) for m in MODELS for d in ("f32", "f32a", "f32s", "bf16")]
TABLE_ROUTE = [Case(m, d, *TABLE, True) for m in MODELS for d in ("f32", "f32a", "f32s", "bf16")]
PREPARED = [Case(m, d, *TABLE, True, prepared=True) for m in MODELS for d in ("f32", "bf16")]
TWO_WORDS = [Case(m, "f32a", 70, 3, False) for m in MODELS]
WIDE = [Case(m, d, *size, integer, prepared=p, hidden=512, heads=2) for m in ("l_dgn", "hl_dgn") for d in ("f32", "bf16")
        for size, integer, p in [(ROWS, False, False), (TABLE, True, False), (TABLE, True, True)]]
SIX_HEADS = [Case("l_dgn", "f32a", *ROWS, False, hidden=64, heads=6), Case("l_dgn", "f32a", *TABLE, True, hidden=64, heads=6)]
SINGLE_HEAD = [Case("l_dgn", "f32", *ROWS, False, dueling=False)]
CASES = ROWS_ROUTE + TABLE_ROUTE + PREPARED + TWO_WORDS + WIDE + SIX_HEADS + SINGLE_HEAD


def make(c):
    from melissa_amd.networks import DGNRNetwork, HLDGNNetwork, LDGNNetwork
    from oracle import net_oracle as no
    sd = no.init_weights(c.model, hidden=c.hidden, heads=c.heads, seed=17, random_conv_bias=True, dueling=c.dueling)
    cls = {"l_dgn": LDGNNetwork, "dgn_r": DGNRNetwork, "hl_dgn": HLDGNNetwork}[c.model]
    kw = dict(aggregator="max") if c.model == "hl_dgn" else {}
    duel = ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]}) if c.dueling else None
    net = cls(5, c.hidden, 2, c.heads, c.n, dueling_param=duel, device="cuda", backend="hip", **kw)
    net.load_state_dict(sd)
    net.set_feature_dtype(c.dtype)
    net.prepared_tables = c.prepared
    return net


def run_case(c):
    """Both entry points of the case's model, each run once and then once more under the stage timer
    -> {"<entry>/<array>": int32 array}."""
    from melissa_amd import _lib
    net = make(c)
    n, bs, cap = c.n, c.bs, c.bs * c.n
    obs = torch.from_numpy(env_like_obs(n, bs, 5 + n)).cuda()
    mat = torch.from_numpy(env_like_obs(n, bs, 6 + n, index_col=False)).cuda()
    am = torch.from_numpy(agent_sets(n, bs, 7 + n)).cuda()
    out = {}

    def record(entry, forward, tap_cap):
        got = {}
        forward()                                       # (workspaces and prepared buffers allocated before the timer is attached)
        stages = launches_by_stage(lambda: got.update(r=forward()))
        logits, off = got["r"] if isinstance(got["r"], tuple) else (got["r"], None)
        if off is not None:
            out[f"{entry}/row_offsets"] = off.cpu().numpy().astype(np.int32)
            logits = logits[:int(off[-1])]
        out[f"{entry}/logits"] = logits.contiguous().view(torch.int32).cpu().numpy()
        out[f"{entry}/table_rows"] = np.array([int(net.hip_tap(3, bs, tap_cap)[0])], dtype=np.int32)
        out[f"{entry}/launches"] = np.array([stages[name] for name in _lib.STAGE_NAMES], dtype=np.int32)

    with torch.no_grad():
        record("forward", lambda: net.hip_forward(obs, integer_features=c.integer), 0)
        if c.model == "hl_dgn":
            record("envs", lambda: net.hip_forward_envs(mat, integer_features=c.integer), 0)
        else:
            record("agents", lambda: net.hip_forward_agents(mat, am, cap, integer_features=c.integer), cap)
    return out


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.key)
def test_forward_launches_and_bits_are_the_parents(case, golden):
    from melissa_amd import _lib
    c = case
    got = run_case(c)
    assert list(golden["stage_names"]) == list(_lib.STAGE_NAMES)
    assert sorted(got) == sorted(k[len(c.key) + 1:] for k in golden if k.startswith(c.key + "/"))
    for name, a in got.items():
        want = golden[f"{c.key}/{name}"]
        where = f"{c.key}, {name} (recorded at {golden['commit']})"
        if name.endswith("/table_rows"):
            assert int(a[0]) == c.table_rows, f"{where}: the forward used {int(a[0])} table rows, the case is built for {c.table_rows}"
        if name.endswith("/launches"):
            assert a.tolist() == want.tolist(), \
                f"{where}: launches per stage {dict(zip(_lib.STAGE_NAMES, a.tolist()))}, recorded {dict(zip(_lib.STAGE_NAMES, want.tolist()))}"
            continue
        assert a.shape == want.shape and a.dtype == want.dtype, (where, a.shape, a.dtype, want.shape, want.dtype)
        differ = np.flatnonzero((a != want).reshape(a.shape[0], -1).any(axis=1))
        assert differ.size == 0, f"{where}: {differ.size} of {a.shape[0]} rows differ, the first: {differ[:8].tolist()}"
