"""CPU tests of tests/bf16_ref.py, the stage-by-stage reference of the bf16 feature path: its rounding against torch's, its
chained stages against oracle/net_oracle.py with the roundings switched off, the fp32 noise its tolerances are derived from,
and the power of the per-stage rule against three seeded mistakes (evaluated IN the reference)."""
import functools

import numpy as np
import pytest
import torch

from oracle import net_oracle as no
from tests import bf16_ref as br


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_to_bf16_is_round_to_nearest_even_bit_for_bit():
    bits = []
    for base in (0x3F80, 0x3F81, 0x0001, 0x0000, 0x7F7F, 0x0080, 0x4049):       # even / odd last bits, subnormal, zero, largest
        for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):            # exact, just above, around the tie, the tie
            for sign in (0, 0x80000000):
                bits.append(sign | (base << 16) | low)
    bits += [0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000, 0x00000001, 0x80000001]
    x = f32(bits)
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = br.to_bf16(x)
    np.testing.assert_array_equal(got, want)
    assert br.to_bf16(f32([0x3F808000]))[0] == 0x3F80 and br.to_bf16(f32([0x3F818000]))[0] == 0x3F82       # ties, both parities
    assert br.to_bf16(f32([0x7F7FFFFF]))[0] == 0x7F80                                                      # rounds to inf
    # NaN stays NaN (IEEE leaves its payload open and torch's builds differ in it: the class is compared, not the payload)
    nan = br.to_bf16(f32([0x7FC00000, 0xFFC00001, 0x7F800001]))
    assert ((nan & 0x7F80) == 0x7F80).all() and ((nan & 0x007F) != 0).all()
    assert np.isnan(br.from_bf16(nan)).all()
    # a large random sweep over all exponents
    rng = np.random.RandomState(0)
    r = rng.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    r = r[~np.isnan(r)]
    np.testing.assert_array_equal(br.to_bf16(r), torch.from_numpy(r).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_to_bf16_rounds_a_float64_once():
    tie = float(f32([0x3F808000])[0])                        # exactly between 0x3f80 and 0x3f81
    below, above = np.nextafter(tie, 0.0), np.nextafter(tie, 2.0)
    assert np.float32(below) == np.float32(tie) == np.float32(above)          # float32 cannot tell them apart
    np.testing.assert_array_equal(br.to_bf16(np.array([below, tie, above, -below, -above])),
                                  np.array([0x3F80, 0x3F80, 0x3F81, 0xBF80, 0xBF81], dtype=np.uint16))
    np.testing.assert_array_equal(br.trunc_bf16(f32([0x3F80FFFF, 0xBF80FFFF])), np.array([0x3F80, 0xBF80], dtype=np.uint16))
    np.testing.assert_array_equal(br.bf16_ulp(np.array([1.0, 1.99, 2.0, 0.0])), [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133])


# (model, n, bs, spread, hidden, heads, dueling hidden sizes or None, aggregator): GATv2, TransformerConv, the three
# aggregators, dueling and out_linear heads
ORACLE_CASES = (("l_dgn", 20, 5, 0.6, 128, 4, (128, 128), None), ("l_dgn", 40, 2, 0.25, 64, 2, None, None),
                ("dgn_r", 20, 5, 0.6, 128, 4, (128, 128), None), ("dgn_r", 7, 3, 1.0, 64, 6, None, None),
                ("hl_dgn", 20, 4, 0.6, 128, 4, (128, 128), "max"), ("hl_dgn", 20, 4, 0.6, 64, 2, (64,), "mean"),
                ("hl_dgn", 40, 2, 0.25, 128, 2, None, "add"))


ORACLE_BAR = 4e-7          # times the largest logit: the fp32 oracle's own rounding (float32 eps 1.2e-7, a few operations deep)


@pytest.mark.parametrize("model,n,bs,spread,hidden,heads,duel,agg", ORACLE_CASES)
def test_chain_without_roundings_is_the_oracle(model, n, bs, spread, hidden, heads, duel, agg):
    kw = dict(dueling_hidden=duel) if duel else dict(dueling=False)
    sd = no.init_weights(model, hidden=hidden, heads=heads, seed=5, random_conv_bias=True, **kw)
    obs = br.make_obs(n, bs, spread, 11 + n)
    c = br.Chain(model, sd, obs, n, heads, agg=agg or "max", rnd=None, wrnd=None)
    fwd = {"l_dgn": no.ldgn_forward, "dgn_r": no.dgnr_forward, "hl_dgn": no.hldgn_forward}[model]
    want = fwd(sd, obs, n, heads=heads, **({"aggregator": agg} if agg else {})).numpy()
    err = np.abs(c.logits - want).max()
    print(f"{model} n={n} {hidden}x{heads}: float64 chain without roundings vs the fp32 oracle {err:.1e} (largest logit {np.abs(want).max():.2f})")
    assert err <= ORACLE_BAR * max(1.0, float(np.abs(want).max()))


def stage_key(c, name):
    """Chain stage -> its entry of A_STAGE / F32_TOL (the last hidden head layer is stored fp32)."""
    return ("hq0" if c.rounded[name] else "hq_last") if name.startswith("hq") else name


@functools.lru_cache(maxsize=None)
def measured(cid):
    case = br.CASES[br.CASE_IDS.index(cid)]
    _, model, n, _, _, _, heads, _, duel, agg, _ = case
    return br.Chain(model, br.case_weights(case), br.case_obs(case), n, heads, agg=agg or "max", measure=True)


def test_tolerances_are_eight_times_the_measured_noise():
    """A_STAGE / F32_TOL of bf16_ref.py against the float32-vs-float64 difference of every reference stage before its rounding,
    on the inputs of every committed case."""
    worst = {}
    for cid in br.CASE_IDS:
        c = measured(cid)
        for name, (err, _, _) in c.noise.items():
            worst[stage_key(c, name)] = max(worst.get(stage_key(c, name), 0.0), err)
    for key in sorted(worst):
        print(f"{key}: largest |float32 - float64| before the rounding {worst[key]:.2e}")
    table = {**br.A_STAGE, **br.F32_TOL}
    assert set(worst) == set(table)
    for key, err in worst.items():
        # (a fifth of slack downwards: the float32 evaluation's summation order is the BLAS build's)
        assert 6.4 * err <= table[key] <= 16 * err, (key, err, table[key])


def test_reference_noise_flips_at_most_a_thousandth_of_a_stage():
    """float32 and float64 evaluations of every stage round to different bf16 bits on at most 0.1 % of its elements: the
    reference alone stays an order of magnitude inside the 1 % the device test allows."""
    for cid in br.CASE_IDS:
        for name, (_, flips, size) in measured(cid).noise.items():
            if size >= 1000:
                assert flips <= 1e-3 * size, (cid, name, flips, size)
            else:                       # a stage of a few hundred elements: a thousandth of it is less than one element
                assert flips <= 1, (cid, name, flips, size)


@functools.lru_cache(maxsize=None)
def power_case(cid):
    case = br.CASES[br.CASE_IDS.index(cid)]
    return case, br.case_weights(case), br.case_obs(case)


@pytest.mark.parametrize("cid", ["ldgn-n40-some", "ldgn-n40-6x128-unequal", "dgnr-n40-some", "hldgn-add-n40-6x64"])
def test_rule_catches_truncating_stores(cid):
    """Every bf16 stage output truncated instead of rounded, on the reference's own inputs: over 10 % of its elements
    leave the reference's bits (about half do)."""
    c = measured(cid)
    for name, pre in c.pre.items():
        if not c.rounded.get(name, False):
            continue
        share, outside, _ = br.compare_bf16(br.trunc_bf16(pre), pre, br.A_STAGE[stage_key(c, name)])
        nonzero = float((pre != 0).mean())
        print(f"{cid} {name}: truncation leaves {share * 100:.1f} % of the elements off the reference's bits ({nonzero * 100:.0f} % nonzero)")
        assert share > 0.10, (name, share, nonzero)


@pytest.mark.parametrize("cid", ["ldgn-n40-some", "ldgn-n40-6x128-unequal", "dgnr-n40-some", "hldgn-add-n40-6x64"])
def test_rule_catches_unrounded_projection_weights(cid):
    """Every projection evaluated with the fp32 weights instead of their bf16 copies, on the same inputs."""
    c = measured(cid)
    for name, alt in c.alt.items():
        if name.startswith("hid0"):     # the standard heads keep fp32 here: their test is below
            continue
        if not c.rounded[name]:         # the last hidden layer, stored fp32
            err = np.abs(alt - c.pre[name]).max()
            assert err > 10 * br.F32_TOL["hq_last"], (name, err)
            continue
        share, outside, _ = br.compare_bf16(br.to_bf16(alt), c.pre[name], br.A_STAGE[stage_key(c, name)])
        print(f"{cid} {name}: unrounded weights leave {share * 100:.1f} % of the elements off the reference's bits, {outside} outside the rule")
        assert share > 0.10, (name, share)


def test_rule_catches_unrounded_weights_in_the_standard_heads():
    """The standard heads store nothing in bf16 after the head input: their first layer's weights show in the logits, far
    above the fp32 bound."""
    case, sd, obs = power_case("ldgn-n40-some")
    good = measured("ldgn-n40-some")
    bad = br.Chain(case[1], sd, obs, case[2], case[6], wrnd=None)
    w = br.net_weights(sd, case[1])
    # the same head input, the first layer's weights unrounded
    hid = [br.linear(br.linear(good.xcat, w[h][0][0], w[h][0][1], True), w[h][1][0], w[h][1][1], True) for h in ("q", "v")]
    logits = br.dueling_tail(hid[0], hid[1], *w["q"][-1], *w["v"][-1], True)
    err = np.abs(logits - good.logits).max()
    print(f"standard heads with unrounded first-layer weights: logits move by {err:.1e} (bound {br.F32_TOL['logits']:.1e})")
    assert err > 10 * br.F32_TOL["logits"]
    assert np.abs(bad.logits - good.logits).max() > 10 * br.F32_TOL["logits"]


@pytest.mark.parametrize("cid", ["ldgn-n40-some", "dgnr-n40-some", "ldgn-n7-2x64-all"])
def test_rule_catches_x2_taken_after_the_mask(cid):
    """x_2 read from the masked conv1 rows: an agent whose decision-maker flag is 0 gets zeros - more than one ulp away."""
    case, sd, obs = power_case(cid)
    _, model, n, bs, _, _, heads, _, _, _, _ = case
    good = measured(cid)
    # the controlling agents of the chain: the index column; make sure one of them is masked
    agent = np.clip(obs[:, -1], 0, n - 1).astype(np.int64)
    dm = obs[:, :-1].reshape(bs, n, 8)[np.arange(bs), agent, 7]
    assert (dm == 0).any(), "the case needs a controlling agent with flag 0"
    bad = br.Chain(model, sd, obs, n, heads, x2_after_mask=True)
    hidden = good.pre["h0"].shape[1]
    hc = good.pre["x2"].shape[1]
    got = br.to_bf16(bad.xcat[:, hidden:hidden + hc])
    share, outside, worst = br.compare_bf16(got, good.pre["x2"], br.A_STAGE["x2"])
    print(f"{cid}: x_2 after the mask: {share * 100:.1f} % of x_2 off the reference's bits, {outside} outside the rule, largest {worst:.2e}")
    assert outside > 0 and share > br.SHARE_CAP
