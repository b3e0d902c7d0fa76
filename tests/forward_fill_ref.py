"""The agents forward (mel_ldgn_forward_agents / mel_dgnr_forward_agents) where its row counts outrun what the host expected:
the sizing rules of csrc/ restated in plain Python, the cases that put more rows into a stage than one pass of its grid covers,
the float64 reference and the bounds - shared by tests/test_forward_fill_ref.py (CPU: the regime as a condition on the inputs,
the reference, the measurement behind every bound) and tests/test_gpu_forward_fill.py (the kernels).  No GPU, no project kernel.

The library learns its three row counts (agent rows nL, conv1 targets n1, encoder rows n2) on the device only; the host sizes
every grid from estimates fitted to the benchmark workload, and a stage that meets more rows than its grid covers goes round
again.  The library does not report its grids, so that the loops run is known from the restated rules alone."""
import functools
from collections import namedtuple

import numpy as np
import torch

from tests import shape_grid_ref as sg

# ---- the sizing rules, restated --------------------------------------------------------------------------------------
FEATURE_TUPLES_PER_DEGREE = 40      # plan_masks.hpp:50
PLANES_FROM = 129                   # gemm_launch.hpp:16 (MEL_PLANES_FROM): expected 128 x 256 work items
GEMP_BN = 256                       # gemm_split.hpp:507


def expected_rows(bs, n):
    """-> (hintL, hint1, hint2), the round-batched estimates of ldgn_forward_impl (fwd.hip:691-693, agent_mask given)."""
    if n < 10:
        return bs, bs * n, bs * n
    return bs * (36 + n) // 18, bs * 2 * (18 + n) // 13, bs * 3 * (8 + n) // 11


Pass = namedtuple("Pass", "rows mb")            # rows one pass of a stage's grid covers; finish: MB of head_finish_kernel<MB>
STAGES = ("att1", "att2", "finish", "enc0")


def one_pass(stage, bs, n, rows_cap):
    hint_l, hint1, hint2 = expected_rows(bs, n)
    if stage in ("att1", "att2"):               # launch_attend, attention.hpp:614-623; the kernel's stride: attention.hpp:440
        hint, cap = (hint1, bs * n) if stage == "att1" else (hint_l, rows_cap)          # (fwd.hip:776, :794)
        want = ((hint if hint > 0 else cap) * 5 // 4 + 3) // 4
        want = max(min(want, (cap + 3) // 4), 256)
        return Pass(4 * ((want + 7) & ~7), None)
    if stage == "finish":                       # run_heads, fwd.hip:461 and :476-483; the kernel's stride: heads.hpp:225
        hint = min(hint_l, rows_cap)
        per = 32 if hint > 16 * 256 else 16
        need, likely = -(-rows_cap // per), -(-hint // per)
        blocks = max(min(2 * likely + 8, need), 1)
        return Pass(blocks * per, per // 16)
    if stage == "enc0":                         # launch_encoder, fwd.hip:82-84 (hidden > 256 only); the stride: fwd.hip:60
        rows = hint2 if 0 < hint2 < bs * n else bs * n
        return Pass(4 * max(min((rows + 3) // 4, 8192), 1), None)
    raise KeyError(stage)


def passes(stage, bs, n, rows_cap, rows):
    """How often the stage's grid goes over ``rows`` rows."""
    return -(-rows // one_pass(stage, bs, n, rows_cap).rows)


def conv2_wide_items(model, bs, n, hc):
    """The expected 128 x 256 work items of conv2's grouped launch (`wide`, gemm_launch.hpp:227; the problems: fwd.hip:709-715):
    lin_l (DGN-R: key | value) on the hint1 rows, lin_r on the hintL rows."""
    hint_l, hint1, _ = expected_rows(bs, n)
    srcw = 2 * hc if model == "dgn_r" else hc
    return -(-hint1 // 128) * (srcw // GEMP_BN) + -(-hint_l // 128) * (hc // GEMP_BN)


def takes_table(bs, n):
    """takes_table (fwd.hip:628-630, called at :695) for integer features."""
    _, hint1, hint2 = expected_rows(bs, n)
    return hint1 + hint2 >= 2 * n * FEATURE_TUPLES_PER_DEGREE


# ---- the cases -------------------------------------------------------------------------------------------------------
# name -> (n, bs); every node an agent: bs * n rows in all three lists.
#   mid:      1600 rows.  Both attention launches cover 1024 rows a pass (the minimum grid of 256 workgroups), head_finish<1>
#             448 (hintL = 152: 2 * 10 + 8 workgroups of 16), the stand-alone encoder layer 0 of (512, 2) 508 (hint2 = 506).
#   two_word: 1680 rows, the same with two-word node sets (W = 2 descriptors); hintL = 141: head_finish<1> covers 416 a pass.
#   big:      16 080 rows.  hintL = 4109 > 4096: head_finish<2>, 266 workgroups of 32 rows = 8512 a pass; the attention grids
#             (hint1 = 6926: 2168 workgroups, hintL: 1288) cover 8672 and 5152.  176 expected wide items >= 129: the planner
#             offers conv2 the 128 x 256 kernels; hint1 + hint2 = 14 819 >= 800: integer features take the table.
CASES = {"mid": (50, 32), "two_word": (70, 24), "big": (10, 1608)}
# stage -> the passes the case is for (the cells with hidden > 256 add enc0)
REACHES = {"mid": {"att1": 2, "att2": 2, "finish": 4}, "two_word": {"att1": 2, "att2": 2, "finish": 5},
           "big": {"att1": 2, "att2": 4, "finish": 2}}
MID_ENC0_PASSES = 4
# further agent sets on the same observations: name -> the case whose observations it takes
SETS = {"mid": "mid", "two_word": "two_word", "big": "big", "empty": "big", "single": "big", "tight": "mid"}
ALL_AGENT = ("mid", "two_word", "big")
SINGLE_NODE = 7                      # the one agent of `single`, in the last env
TIGHT_SEED = 3                       # 3 - 30 agents per env; the sum: tests/test_forward_fill_ref.py

CELLS_MID = ((128, 4), (64, 6), (512, 2))       # (64, 6): 48 live lanes; (512, 2): encoder layer 0 in its own launch
CELL_BIG = (128, 4)
MODELS = ("l_dgn", "dgn_r")


@functools.lru_cache(maxsize=None)
def observations(name):
    """-> obs [bs, 8 n + 1] float32 of a case of CASES, built like shape_grid_ref.case_inputs: integer features (inside the
    node-feature table's range), flags 0 on about a fifth of the nodes, positions on [0, 0.6]^2; the index column is 0 (the
    agents forward does not read it)."""
    n, bs = CASES[name]
    rng = np.random.RandomState(2000 + n)
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, 0.6, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, min(n, 9), size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = rng.uniform(size=(bs, n)) >= 0.2
    obs.setflags(write=False)
    return obs


@functools.lru_cache(maxsize=None)
def agent_sets(name):
    """-> (agent sets bool [bs, n], rows_cap) of an entry of SETS."""
    n, bs = CASES[SETS[name]]
    live = np.zeros((bs, n), dtype=bool)
    if name in ALL_AGENT:
        live[:] = True
    elif name == "single":
        live[bs - 1, SINGLE_NODE] = True
    elif name == "tight":
        rng = np.random.RandomState(TIGHT_SEED)
        for b in range(bs):
            live[b, rng.choice(n, size=rng.randint(3, 31), replace=False)] = True
    elif name != "empty":
        raise KeyError(name)
    live.setflags(write=False)
    return live, (int(live.sum()) if name == "tight" else bs * n)


def rows_of(live):
    """The (env, agent) pairs of the logits rows, by env and agent id."""
    return [(int(b), int(a)) for b, a in zip(*np.nonzero(live))]


# ---- the float64 oracle ----------------------------------------------------------------------------------------------
def oracle_all(model, hidden, heads, case, dtype=torch.float64, formulation="edges"):
    """oracle/net_oracle.py on EVERY (env, node) of a case as an agent row -> (logits [bs n, A], head input [bs n, latent],
    adjacency), row b * n + a.  A row depends on its env's observation and its agent alone, never on which other agents are
    in the set: every entry of SETS on these observations takes its rows from here."""
    n, bs = CASES[case]
    pairs = [(b, a) for b in range(bs) for a in range(n)]
    return sg.oracle(model, "max", sg.weights(model, hidden, heads), observations(case).copy(), n, heads, dtype=dtype,
                     formulation=formulation, rows=pairs)


@functools.lru_cache(maxsize=None)
def exact(model, hidden, heads, case):
    """The float64 oracle, once per process; its arrays are shared and read-only."""
    out = oracle_all(model, hidden, heads, case)
    for a in out:
        a.setflags(write=False)
    return out


def expected(model, hidden, heads, name):
    """-> (logits, head input) of the rows of an entry of SETS in row order, (n1, n2, nL) as mel_forward_tap kind 2 gives them."""
    live, _ = agent_sets(name)
    logits, head, adj = exact(model, hidden, heads, SETS[name])
    flat = np.flatnonzero(live.reshape(-1))
    return logits[flat], head[flat], sg.plan_counts(adj, live, model == "l_dgn")


# ---- the bounds ------------------------------------------------------------------------------------------------------
# f32: the shape grid's rule - 8 x the largest |float32 - float64| of the oracle on THESE inputs (every cell and case of
# grid_cells() below, both formulations), measured and held to the constants by
# tests/test_forward_fill_ref.py::test_bounds_are_eight_times_the_measured_noise (a fifth less at the most, never more than
# twice as much).  None exceeds the suite's 1e-4.
LOGITS_TOL = {               # absolute
    "l_dgn": 3.5e-7,           # measured 4.41e-08
    "dgn_r": 3.8e-7,           # measured 4.74e-08
}
HEAD_INPUT_TOL = {           # absolute, x_cat
    "l_dgn": 1.05e-5,          # measured 1.31e-06 (x_1 of (512, 2): encoder rows reach 3.3)
    "dgn_r": 1.05e-5,          # measured 1.31e-06 (the same x_1)
}
# f32a / f32s on `big`: the three-plane kernels' dropped partial products are not in the oracle's float32 noise; the bar the
# project keeps for them on forward logits (tests/test_gpu_round.py TOL).  The head input is held to the same figure: its
# entries reach 2.5 there, so 1e-4 is 4e-5 of the largest - some 670 units of 2^-24, where a K = 512 sum of three-plane
# products that drops the terms below 2^-24 of a product stays within a few dozen.
PLANES_TOL = 1e-4
BF16_TOL = sg.BF16_TOL


def grid_cells():
    """(hidden, heads, case) of every f32 reference the GPU grid uses."""
    return [(h, k, "mid") for h, k in CELLS_MID] + [CELL_BIG + ("two_word",), CELL_BIG + ("big",)]
