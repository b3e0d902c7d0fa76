"""CPU tests of tests/forward_fill_ref.py: that the cases ARE in the regime they are for - more rows than one pass of each
stage's grid covers under the restated sizing rules, the only way to know the kernels' loops run, since the library does not
report its grids -, the expected row counts, the float64 reference, and the measurement every f32 bound is 8 times of."""
import functools

import numpy as np
import pytest
import torch

from oracle import net_oracle as no
from tests import forward_fill_ref as ff
from tests import shape_grid_ref as sg


def test_the_restated_rules_on_the_sizes_the_source_comments_quote():
    # fwd.hip:689-690: per env |L| = 3.1 / 4.7, |U1| = 5.8 / 10.4, |U2| = 7.6 / 15.8 at N = 20 / 50 - the fits give these back
    assert ff.expected_rows(1000, 20) == (3111, 5846, 7636) and ff.expected_rows(1000, 50) == (4777, 10461, 15818)
    assert ff.expected_rows(7, 9) == (7, 63, 63)
    # the benchmark batch (1024 x 50): the attention grids follow the hint, the finish takes MB = 2
    assert ff.one_pass("att1", 1024, 50, 51200).rows == 4 * 3352 and ff.one_pass("att2", 1024, 50, 51200).rows == 4 * 1536
    assert ff.one_pass("finish", 1024, 50, 51200) == (32 * (2 * 153 + 8), 2)
    # below 1024 rows no attention launch can loop: the minimum grid
    assert ff.one_pass("att2", 4, 40, 160).rows == 1024 and ff.one_pass("att1", 48, 7, 336).rows == 1024
    # a rows_cap below the estimate bounds the finish's grid by `need`
    assert ff.one_pass("finish", 32, 50, 100) == (112, 1)


@pytest.mark.parametrize("case", ff.ALL_AGENT)
def test_every_all_agent_case_outruns_one_pass_of_each_stage_it_is_for(case):
    n, bs = ff.CASES[case]
    live, cap = ff.agent_sets(case)
    rows = bs * n
    assert live.all() and cap == rows
    for stage, want in ff.REACHES[case].items():
        one = ff.one_pass(stage, bs, n, cap)
        print(f"{case} {stage}: {rows} rows, {one.rows} a pass, {ff.passes(stage, bs, n, cap, rows)} passes")
        assert rows > one.rows and ff.passes(stage, bs, n, cap, rows) == want >= 2
        # the last pass is a partial one: some workgroups go round once more than others
        assert rows % one.rows
    mb = ff.one_pass("finish", bs, n, cap).mb
    assert mb == (2 if case == "big" else 1)
    # at least twice one pass wherever the sizes allow: the finish of the two small cases (a third and a fourth pass)
    if case != "big":
        assert rows >= 2 * ff.one_pass("finish", bs, n, cap).rows
    if case == "mid":
        assert ff.passes("enc0", bs, n, cap, rows) == ff.MID_ENC0_PASSES and rows >= 2 * ff.one_pass("enc0", bs, n, cap).rows
    if case == "two_word":
        assert n > 64
    if case == "big":
        hint_l, hint1, hint2 = ff.expected_rows(bs, n)
        assert hint_l == 4109 > 16 * 256
        hc = ff.CELL_BIG[0] * ff.CELL_BIG[1]
        assert ff.conv2_wide_items("l_dgn", bs, n, hc) == 2 * (-(-hint1 // 128) + -(-hint_l // 128)) == 176 >= ff.PLANES_FROM
        assert ff.conv2_wide_items("dgn_r", bs, n, hc) >= ff.PLANES_FROM
        assert ff.takes_table(bs, n) and not ff.takes_table(*reversed(ff.CASES["mid"]))


def test_the_further_agent_sets():
    n, bs = ff.CASES["big"]
    empty, cap = ff.agent_sets("empty")
    assert not empty.any() and cap == bs * n
    single, cap = ff.agent_sets("single")
    assert single.sum() == 1 and single[bs - 1, ff.SINGLE_NODE] and cap == bs * n
    # (the estimates know nothing of the agent sets: `single` and `empty` get the large kernels `big` gets)
    assert ff.one_pass("finish", bs, n, cap).mb == 2
    n, bs = ff.CASES["mid"]
    tight, cap = ff.agent_sets("tight")
    per_env = tight.sum(1)
    assert per_env.min() >= 3 and per_env.max() <= 30 and cap == tight.sum() == 545
    one = ff.one_pass("finish", bs, n, cap)
    assert cap > one.rows == 448 and cap % 16 and one.mb == 1
    assert ff.one_pass("att2", bs, n, cap).rows == 1024 > cap          # (no attention loop here: the finish's alone)


@pytest.mark.parametrize("case", sorted(ff.CASES))
def test_inputs_hold_what_the_cases_need(case):
    n, bs = ff.CASES[case]
    obs = ff.observations(case)
    m = obs[:, :-1].reshape(bs, n, 8)
    assert np.array_equal(m[:, :, 2:], np.round(m[:, :, 2:])) and m[:, :, 2].max() < 9 and m[:, :, 3].max() < 5
    assert 0 <= m[:, :, :2].min() and m[:, :, :2].max() <= 0.6
    assert 0.1 < (m[:, :, 7] == 0).mean() < 0.3
    adj = no.radius_adjacency(torch.from_numpy(m[:, :, :2].copy())).numpy()
    assert adj.any() and (adj.sum(2) == 0).any() == (case == "big")          # n = 10: isolated targets too


@pytest.mark.parametrize("model", ff.MODELS)
def test_expected_counts(model):
    for case in ff.ALL_AGENT:
        n, bs = ff.CASES[case]
        assert ff.expected(model, *ff.CELL_BIG, case)[2] == (bs * n, bs * n, bs * n)
    assert ff.expected(model, *ff.CELL_BIG, "empty")[2] == (0, 0, 0)
    n1, n2, n_l = ff.expected(model, *ff.CELL_BIG, "single")[2]
    assert n_l == 1 and 1 <= n1 <= n2 <= ff.CASES["big"][0]
    n1, n2, n_l = ff.expected(model, *ff.CELL_BIG, "tight")[2]
    assert n_l == 545 <= n1 <= n2 <= 1600


@pytest.mark.parametrize("model", ff.MODELS)
def test_oracle_rows_equal_the_oracle_on_explicit_observation_rows(model):
    """A sample of rows of every set: the same (env, agent) pairs as observation rows with the index column, through
    net_oracle's own entry point in float64."""
    fwd = no.ldgn_forward if model == "l_dgn" else no.dgnr_forward
    hidden, heads = ff.CELL_BIG
    sd = sg.weights(model, hidden, heads)
    for name in ("mid", "two_word", "big", "single", "tight"):
        n, _bs = ff.CASES[ff.SETS[name]]
        live, _ = ff.agent_sets(name)
        pairs = ff.rows_of(live)
        want_logits, want_head, _ = ff.expected(model, hidden, heads, name)
        assert len(pairs) == len(want_logits) == len(want_head)
        pick = sorted(set(np.random.RandomState(1).randint(0, len(pairs), 12)) | {0, len(pairs) - 1})
        obs = ff.observations(ff.SETS[name])
        rows = np.stack([np.concatenate([obs[pairs[i][0], :-1], [pairs[i][1]]]) for i in pick]).astype(np.float32)
        with torch.no_grad():
            got, mid = fwd(sd, rows, n, heads=heads, dtype=torch.float64, return_intermediates=True)
        assert np.abs(got.numpy() - want_logits[pick]).max() <= 1e-12
        assert np.abs(mid["x_cat"].numpy() - want_head[pick]).max() <= 1e-12


@functools.lru_cache(maxsize=None)
def measured(model):
    """The largest |float32 - float64| of the oracle over the grid's cells and cases, both formulations: (logits, head input);
    the largest difference of the two formulations in float64."""
    worst = [0.0, 0.0, 0.0]
    for hidden, heads, case in ff.grid_cells():
        want = ff.exact(model, hidden, heads, case)
        dense = ff.oracle_all(model, hidden, heads, case, formulation="dense")
        worst[2] = max(worst[2], np.abs(dense[0] - want[0]).max(), np.abs(dense[1] - want[1]).max())
        for form in ("edges", "dense"):
            got = ff.oracle_all(model, hidden, heads, case, dtype=torch.float32, formulation=form)
            assert np.array_equal(got[2], want[2])
            worst[0] = max(worst[0], np.abs(got[0] - want[0]).max())
            worst[1] = max(worst[1], np.abs(got[1] - want[1]).max())
    return tuple(float(v) for v in worst)


@pytest.mark.parametrize("model", ff.MODELS)
def test_bounds_are_eight_times_the_measured_noise(model):
    logits, head, formulations = measured(model)
    print(f"{model}: largest |float32 - float64| logits {logits:.2e}, head input {head:.2e}; formulations apart {formulations:.1e}")
    assert formulations <= 1e-12
    # (a fifth of slack downwards: the float32 evaluation's summation order is the BLAS build's)
    assert 6.4 * logits <= ff.LOGITS_TOL[model] <= 16 * logits
    assert 6.4 * head <= ff.HEAD_INPUT_TOL[model] <= 16 * head
    assert ff.LOGITS_TOL[model] <= sg.OLD_LOGITS_BAR and ff.HEAD_INPUT_TOL[model] <= sg.OLD_LOGITS_BAR
    assert ff.PLANES_TOL == sg.OLD_LOGITS_BAR and ff.BF16_TOL == sg.BF16_TOL
