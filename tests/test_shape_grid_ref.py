"""CPU tests of tests/shape_grid_ref.py: the float64 evaluation of the oracle, the measurement every bound of the shape grid is 8
times of, and the sharpness of those bounds - six mistakes seeded into the float64 reference, each of which must leave a bound
on every (shape, model) cell it applies to.  Beside each mutant: how many cells it would have passed at the former 1e-4 bar."""
import functools

import numpy as np
import pytest
import torch

from oracle import net_oracle as no
from tests import shape_grid_ref as sg

IDS = [sg.cell_id(c) for c in sg.CELLS]


def cases_of(cell):
    hidden, heads, model, _agg = cell
    pool4 = [sg.POOL4_CASE] if model == "hl_dgn" and (hidden, heads) in sg.POOL4_SHAPES else []
    return list(sg.FORWARD_CASES + (sg.TABLE_CASE_HL if model == "hl_dgn" else sg.TABLE_CASE,) + sg.LEARN_CASES) + pool4


def rows_of(model, name):
    return None if model == "hl_dgn" else sg.case_rows(name)


@functools.lru_cache(maxsize=None)
def exact(cell, name):
    """The float64 oracle (edges) of a cell on a case: (logits, head input, adjacency)."""
    hidden, heads, model, agg = cell
    obs, _live = sg.case_inputs(name)
    return sg.oracle(model, agg, sg.weights(model, hidden, heads), obs, sg.CASES[name][0], heads, rows=rows_of(model, name))


@functools.lru_cache(maxsize=None)
def measured(cell):
    """Per tensor the largest |float32 - float64| of the oracle over the cell's cases, both formulations; the largest difference
    of the two formulations in float64."""
    hidden, heads, model, agg = cell
    sd = sg.weights(model, hidden, heads)
    worst = {"logits": 0.0, "head_input": 0.0, "loss": 0.0, "grad": 0.0, "formulations": 0.0}
    for name in cases_of(cell):
        obs, _live = sg.case_inputs(name)
        n, rows = sg.CASES[name][0], rows_of(model, name)
        want = exact(cell, name)
        dense = sg.oracle(model, agg, sd, obs, n, heads, formulation="dense", rows=rows)
        worst["formulations"] = max(worst["formulations"], np.abs(dense[0] - want[0]).max(), np.abs(dense[1] - want[1]).max())
        for form in ("edges", "dense"):
            got = sg.oracle(model, agg, sd, obs, n, heads, dtype=torch.float32, formulation=form, rows=rows)
            assert np.array_equal(got[2], want[2])
            worst["logits"] = max(worst["logits"], np.abs(got[0] - want[0]).max())
            worst["head_input"] = max(worst["head_input"], np.abs(got[1] - want[1]).max())
        if name in sg.LEARN_CASES:
            _l64, loss64, g64 = sg.oracle_grads(model, agg, sd, obs, n, heads)
            _ld, lossd, gd = sg.oracle_grads(model, agg, sd, obs, n, heads, formulation="dense")
            worst["formulations"] = max([worst["formulations"], abs(lossd - loss64)] +
                                        [e / s for e, s in sg.grad_errors(gd, g64).values()])
            kinks, near = sg.kink_allowance(model, agg, sd, obs, n, heads)
            worst["near_kinks"] = worst.get("near_kinks", 0) + near
            for form in ("edges", "dense"):
                _l32, loss32, g32 = sg.oracle_grads(model, agg, sd, obs, n, heads, dtype=torch.float32, formulation=form)
                worst["loss"] = max(worst["loss"], abs(loss32 - loss64) / max(1.0, abs(loss64)))
                worst["grad"] = max([worst["grad"]] + [max(0.0, e - kinks[k]) / s for k, (e, s) in sg.grad_errors(g32, g64).items()])
    return {k: float(v) for k, v in worst.items()}


def test_the_rule_accepts_the_listed_pairs_and_every_cell_is_in_the_grid():
    assert sg.SHAPES == sg.ACCEPTED and len(sg.CELLS) == 3 * len(sg.SHAPES) + 2 * len(sg.ALL_AGGREGATORS)
    assert set(sg.ALL_AGGREGATORS) | set(sg.POOL4_SHAPES) <= set(sg.SHAPES)
    lanes = {s: sg.head_lanes(s[1], s[0])[:3] for s in sg.SHAPES}
    assert {v[2] for s, v in lanes.items() if s in sg.POOL4_SHAPES} == {2, 4, 8, 16}
    # every lanes-per-head count of attention.hpp's head_sum occurs: 64 (one head), 32, 16, 8 (full and 48 live lanes), 4
    assert {v[0] for v in lanes.values()} == {64, 32, 16, 8, 4} and lanes[(256, 4)] == (16, 64, 16)


@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_inputs_hold_what_the_cases_are_for(name):
    obs, live = sg.case_inputs(name)
    n, bs, _ = sg.CASES[name]
    m = obs[:, :-1].reshape(bs, n, 8)
    adj = no.radius_adjacency(torch.from_numpy(m[:, :, :2].copy())).numpy()
    assert np.array_equal(m[:, :, 2:], np.round(m[:, :, 2:]))                                  # the table can take them
    assert live[0].sum() == 1 and live[0, 0] and not adj[0, 0].any() and not adj[0, :, 0].any()    # the isolated single agent
    assert live[1].all() and obs[1, -1] == n - 1 and m[1, n - 1, 7] == 0                          # x_2 of a masked agent
    assert 0.1 < (m[:, :, 7] == 0).mean() < 0.35 and (m[1:, :, 7] == 0).any(1).all() and (m[:, :, 7] == 1).any(1).all()
    assert all(live[b, int(obs[b, -1])] for b in range(bs))
    if n > sg.CAP_ROW:
        cnt = adj.sum(2)
        assert cnt.max() == 33 and (adj != adj.transpose(0, 2, 1)).any()
        if name in sg.FORWARD_CASES:
            assert (cnt[1, :33] == 32).all() and (cnt[1, 33:] == 33).all()                      # cut rows, with and without self
    if n > 64:
        assert live[1:, 64:].any(1).all() and adj[2:, :, 64:].any()


@pytest.mark.parametrize("cell", sg.CELLS, ids=IDS)
def test_float64_evaluation_and_its_two_formulations(cell):
    """edges and dense agree in float64 to 1e-12 on every case (logits, head input, loss, gradients relative to their scale);
    reference64 - the formulation the mutants are seeded into - is the same function; the float32 default is untouched."""
    hidden, heads, model, agg = cell
    m = measured(cell)
    print(f"{sg.cell_id(cell)}: " + ", ".join(f"{k} {v:.2e}" for k, v in m.items()))
    assert m["formulations"] <= 1e-12
    sd = sg.weights(model, hidden, heads)
    for name in sg.FORWARD_CASES:
        obs, _ = sg.case_inputs(name)
        logits, head = sg.reference64(model, agg, sd, obs, sg.CASES[name][0], heads, rows_of(model, name))
        want = exact(cell, name)
        assert np.abs(logits - want[0]).max() <= 1e-12 and np.abs(head - want[1]).max() <= 1e-12 * max(1.0, np.abs(want[1]).max())
    obs, _ = sg.case_inputs("l20")
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    fwd = {"l_dgn": no.ldgn_forward, "dgn_r": no.dgnr_forward, "hl_dgn": no.hldgn_forward}[model]
    with torch.no_grad():
        default, explicit = fwd(sd, obs, 20, heads=heads, **kw), fwd(sd, obs, 20, heads=heads, dtype=torch.float32, **kw)
        assert default.dtype == torch.float32 and torch.equal(default, explicit)
        assert fwd(sd, obs, 20, heads=heads, dtype=torch.float64, **kw).dtype == torch.float64


def test_autograd_runs_through_the_double_evaluation_from_double_leaves():
    sd = sg.weights("l_dgn", 64, 2)
    obs, _ = sg.case_inputs("l20")
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    for form in ("edges", "dense"):
        out = no.ldgn_forward(leaves, obs, 20, heads=2, dtype=torch.float64, formulation=form)
        out.pow(2).sum().backward()
    assert all(v.grad is not None and v.grad.dtype == torch.float64 and torch.isfinite(v.grad).all() for v in leaves.values())


def test_bounds_are_eight_times_the_measured_noise():
    worst = {}
    for cell in sg.CELLS:
        key = sg.model_key(cell[2], cell[3])
        for k, v in measured(cell).items():
            worst[(k, key)] = max(worst.get((k, key), 0.0), v)
    tables = {"logits": sg.LOGITS_TOL, "head_input": sg.HEAD_INPUT_TOL, "loss": sg.LOSS_TOL, "grad": sg.GRAD_TOL}
    for (k, key), v in sorted(worst.items()):
        print(f"{k} {key}: largest |float32 - float64| {v:.2e}")
    for (k, key), v in worst.items():
        if k in ("formulations", "near_kinks"):
            continue
        # (a fifth of slack downwards: the float32 evaluation's summation order is the BLAS build's)
        assert 6.4 * v <= tables[k][key] <= 16 * v, (k, key, v, tables[k].get(key))
    assert all(set(t) == {sg.model_key(c[2], c[3]) for c in sg.CELLS} for t in tables.values())
    assert max(sg.LOGITS_TOL.values()) <= sg.OLD_LOGITS_BAR and max(sg.GRAD_TOL.values()) <= sg.OLD_GRAD_BAR


@functools.lru_cache(maxsize=None)
def mutant_margins(mutant):
    """{cell: (logits move / bound, head input move / bound, logits move)} on the n40 case - or None where the mutant has no
    meaning for the cell."""
    name = "n40"
    n = sg.CASES[name][0]
    obs, _ = sg.case_inputs(name)
    out = {}
    for cell in sg.CELLS:
        hidden, heads, model, agg = cell
        if not sg.mutant_applies(mutant, model, agg, heads, n):
            continue
        key = sg.model_key(model, agg)
        good = sg.reference64(model, agg, sg.weights(model, hidden, heads), obs, n, heads, rows_of(model, name))
        bad = sg.run_mutant(model, agg, sg.weights(model, hidden, heads), obs, n, hidden, heads, rows_of(model, name), mutant)
        dl, dh = np.abs(bad[0] - good[0]).max(), np.abs(bad[1] - good[1]).max()
        out[cell] = (dl / sg.LOGITS_TOL[key], dh / sg.HEAD_INPUT_TOL[key], dl)
    return out


@pytest.mark.parametrize("mutant", sg.MUTANTS)
def test_bounds_catch_the_mutant_on_every_cell(mutant):
    margins = mutant_margins(mutant)
    assert len(margins) >= 4
    passed_before = sum(1 for _, _, dl in margins.values() if dl <= sg.OLD_LOGITS_BAR)
    weakest = min(margins, key=lambda c: max(margins[c][:2]))
    print(f"{mutant}: {len(margins)} cells, {passed_before} of them inside the former 1e-4 logits bar; weakest cell "
          f"{sg.cell_id(weakest)}: logits at {margins[weakest][0]:.1f} x their bound, head input at {margins[weakest][1]:.1f} x")
    missed = [sg.cell_id(c) for c, (a, b, _) in margins.items() if max(a, b) <= 1.0]
    assert not missed, missed
