"""A bf16-faithful CPU reference of the bf16 feature path (MEL_PREC_BF16, include/melissa_hip.h), ONE FUNCTION PER STAGE, and
the cases, observations and comparison rule its two test modules share.  numpy only; no project kernel and none of the
project's dense formulations is used in the stage functions (the rule of tests/learn_ref.py): tests/test_bf16_ref.py compares
this module with ``oracle/net_oracle.py`` (roundings off) and measures its own fp32 noise, tests/test_gpu_bf16_stages.py
compares the kernels with it stage by stage, every stage fed with what the device itself stored for the previous one.

A stage function takes its inputs as the device holds them - bf16 BIT PATTERNS (uint16 arrays) or fp32 / float64 values - and
returns the result BEFORE the stage's rounding, evaluated in ``dtype`` (float64: the reference; float32: its noise model).
``to_bf16`` rounds to nearest even on bit patterns.  The rounding points are those of csrc/fwd.hip (NOTES.md lists them).
"""
import math

import numpy as np

GATV2, TRANSFORMER = 0, 1

# ---- bf16 bit patterns -----------------------------------------------------------------------------------------------


def to_bf16(x):
    """float32 or float64 array -> uint16 bf16 bit patterns, round to nearest even.  A float64 is rounded ONCE (its way through
    float32 may land exactly on a bf16 tie it was not on: the residue then decides).  NaN -> 0x7fc0 with the sign."""
    x = np.ascontiguousarray(x)
    if x.dtype not in (np.float32, np.float64):
        raise TypeError(x.dtype)
    f = np.ascontiguousarray(x.astype(np.float32))
    bits = f.view(np.uint32)
    hi, low = bits >> np.uint32(16), bits & np.uint32(0xFFFF)
    tie = low == 0x8000
    up = (low > 0x8000) | (tie & ((hi & np.uint32(1)) == 1))
    if x.dtype == np.float64:
        with np.errstate(invalid="ignore"):
            back = f.astype(np.float64)
            moved = tie & (back != x) & np.isfinite(back)
            up = np.where(moved, np.abs(x) > np.abs(back), up)
    out = (hi + up.astype(np.uint32)).astype(np.uint16)
    nan = np.isnan(f)
    return np.where(nan, (hi & np.uint32(0x8000)).astype(np.uint16) | np.uint16(0x7FC0), out)


def trunc_bf16(x):
    """The seeded mistake "a truncating store": the upper 16 bits of the float32."""
    return (np.ascontiguousarray(np.asarray(x).astype(np.float32)).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def from_bf16(bits):
    """uint16 bf16 bit patterns -> float64 values (exact)."""
    b = np.ascontiguousarray(bits)
    assert b.dtype == np.uint16, b.dtype
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def vals(x, dtype=np.float64):
    """An operand as the device holds it -> its values in ``dtype`` (bf16 bits decode exactly into either)."""
    x = np.asarray(x)
    return (from_bf16(x) if x.dtype == np.uint16 else x).astype(dtype)


def bf16_ulp(mag):
    """One bf16 unit in the last place at magnitude ``mag`` (8 significant bits; the smallest subnormal below 2^-126)."""
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(np.abs(mag), 2.0 ** -126)))
    return 2.0 ** (np.maximum(e, -126.0) - 7.0)


# ---- the stages ------------------------------------------------------------------------------------------------------
def encoder_layer0(x, w0, b0, dtype=np.float64):
    """relu(W0 x + b0): fp32 node features [rows, in], the fp32 PARAMETERS (this layer's weights are never rounded); its
    output is rounded to bf16 as it becomes the operand of layer 1."""
    return np.maximum(vals(x, dtype) @ vals(w0, dtype).T + vals(b0, dtype), 0)


def linear(a, w, bias, relu, dtype=np.float64):
    """act(a W^T + bias): encoder layer 1, lin_l / lin_r / query / key / value, a head layer.  ``a`` [rows, K] and ``w``
    [N, K] as the device holds them (bf16 bits on this path; the standard heads' second layer: fp32), fp32 bias or None."""
    y = vals(a, dtype) @ vals(w, dtype).T
    if bias is not None:
        y = y + vals(bias, dtype)
    return np.maximum(y, 0) if relu else y


def attend(kind, xl, xr, att, bias, sources, xr_rows, heads, dtype=np.float64):
    """relu(conv + bias) of GATv2Conv / TransformerConv for a list of targets.  ``xl`` [S, hc] source rows (TransformerConv:
    [S, 2 hc], key | value), ``xr`` [*, hc] target rows (lin_r / query); target t reads xr[xr_rows[t]] and the rows
    ``sources[t]`` of xl - for GATv2 the caller includes the self-loop, for TransformerConv it does not, and a target without
    a source aggregates 0.  e = att . leaky_relu(x_r + x_l, 0.2) (GATv2) or q . k / sqrt(C); softmax over the sources with
    1e-16 added to the denominator; fp32 ``att`` [hc] and ``bias`` [hc] (None for TransformerConv)."""
    xl, xr = vals(xl, dtype), vals(xr, dtype)
    hc = xr.shape[1]
    c = hc // heads
    out = np.zeros((len(sources), hc), dtype=dtype)
    a = vals(att, dtype).reshape(heads, c) if kind == GATV2 else None
    for t, src in enumerate(sources):
        if len(src) == 0:
            continue
        k = xl[src, :hc].reshape(-1, heads, c)
        q = xr[xr_rows[t]].reshape(heads, c)
        if kind == GATV2:
            z = q[None] + k
            e = (np.where(z > 0, z, dtype(0.2) * z) * a).sum(-1)
            v = k
        else:
            e = (k * q[None]).sum(-1) / dtype(math.sqrt(c))
            v = xl[src, hc:].reshape(-1, heads, c)
        p = np.exp(e - e.max(0))
        alpha = p / (p.sum(0) + dtype(1e-16))
        out[t] = (alpha[:, :, None] * v).sum(0).reshape(hc)
    if bias is not None:
        out = out + vals(bias, dtype)
    return np.maximum(out, 0)


def pool(o, dm, n, agg, dtype=np.float64):
    """HL-DGN: o [bs * n, hc] (the UNROUNDED conv rows) times the decision-maker flag, then max / mean / add over the graph."""
    v = (vals(o, dtype) * vals(dm, dtype).reshape(-1, 1)).reshape(-1, n, o.shape[1])
    if agg == "max":
        return v.max(1)
    return v.sum(1) / dtype(n) if agg == "mean" else v.sum(1)


def dueling_tail(hq, hv, wq, bq, wv, bv, dueling, dtype=np.float64):
    """The last Linear of Q (and V) on the fp32 parameters and q - mean(q) + v; ``dueling`` False: q alone (out_linear)."""
    q = vals(hq, dtype) @ vals(wq, dtype).T + vals(bq, dtype)
    if not dueling:
        return q
    v = vals(hv, dtype) @ vals(wv, dtype).T + vals(bv, dtype)
    return q - q.mean(1, keepdims=True) + v


# ---- the comparison rule ---------------------------------------------------------------------------------------------
def compare_bf16(got_bits, pre, a_stage, extra=0.0):
    """The rule for a bf16 stage output: every element is bit-equal to the reference's rounded value or within
    max(one bf16 ulp of the larger magnitude, a_stage) of it.  Returns (share of elements not bit-equal, number of elements
    outside the rule, largest |got - ref| among the not-bit-equal).  +0 and -0 count as equal.  ``extra`` (per element, zero
    almost everywhere) is added to the bound where an INPUT of the stage may legitimately have been rounded the other way
    inside the same launch (the encoder's first layer)."""
    got_bits = np.asarray(got_bits)
    want_bits = to_bf16(np.asarray(pre))
    got, want = from_bf16(got_bits), from_bf16(want_bits)
    differ = (got_bits != want_bits) & ~((got == 0) & (want == 0))
    with np.errstate(invalid="ignore"):
        diff = np.abs(got - want)
    allowed = np.maximum(bf16_ulp(np.maximum(np.abs(got), np.abs(want))), a_stage) + extra
    outside = differ & ~(diff <= allowed)
    return float(differ.mean()) if differ.size else 0.0, int(outside.sum()), float(diff[differ].max()) if differ.any() else 0.0


SHARE_CAP = 0.01            # of a stage output's elements may differ from the reference's bits (the issue's condition)


# ---- weights ---------------------------------------------------------------------------------------------------------
def net_weights(sd, model):
    """The oracle's state dict as numpy float32 under one naming for the three models: enc0 / enc1 = (w, b); c1 / c2 = dict
    l, r, v (TransformerConv: l = key, r = query, v = value, each (w, b)), att [hc], bias [hc] or None; q / v = lists of
    (w, b); dueling."""
    g = lambda k: sd[k].numpy().astype(np.float32)
    lin = lambda p: (g(p + ".weight"), g(p + ".bias"))
    w = {"enc0": lin("encoder.model.0"), "enc1": lin("encoder.model.2"), "kind": TRANSFORMER if model == "dgn_r" else GATV2}
    for c in ("conv1", "conv2"):
        if c + ".lin_l.weight" in sd:
            w["c" + c[-1]] = {"l": lin(c + ".lin_l"), "r": lin(c + ".lin_r"), "v": None, "att": g(c + ".att").reshape(-1),
                              "bias": g(c + ".bias")}
        elif c + ".lin_key.weight" in sd:
            w["c" + c[-1]] = {"l": lin(c + ".lin_key"), "r": lin(c + ".lin_query"), "v": lin(c + ".lin_value"), "att": None,
                              "bias": None}
    w["dueling"] = "out_linear.weight" not in sd
    if w["dueling"]:
        for h in ("Q", "V"):
            k, layers = 0, []
            while f"{h}.model.{2 * k}.weight" in sd:
                layers.append(lin(f"{h}.model.{2 * k}"))
                k += 1
            w[h.lower()] = layers
    else:
        w["q"] = w["v"] = [lin("out_linear")]
    return w


def source_side(conv):
    """The source-side projection of a conv as ONE matrix: lin_l, or key | value stacked along the outputs."""
    if conv["v"] is None:
        return conv["l"]
    return np.concatenate([conv["l"][0], conv["v"][0]]), np.concatenate([conv["l"][1], conv["v"][1]])


def standard_heads(w):
    """fwd.hip run_heads: two hidden layers of 128 for Q and for V take the split first layer + one finishing launch."""
    return w["dueling"] and all([l[0].shape[0] for l in w[h][:-1]] == [128, 128] for h in ("q", "v")) and w["q"][-1][0].shape[0] <= 4


# ---- the chained forward on the WHOLE graph (the CPU tests; the device test packs rows itself) ------------------------
def radius_sets(pos):
    """bool [bs, n, n], [b, i, j] = j is a source of i: the radius rule via networks.common.radius_adjacency."""
    import torch
    from melissa_amd.networks import common
    return common.radius_adjacency(torch.from_numpy(np.ascontiguousarray(pos, dtype=np.float32))).numpy()


class Chain:
    """One forward of the bf16 path on every node of every graph, stage by stage.  ``rnd`` / ``wrnd``: the rounding of the
    stores / of the projection weights (to_bf16, trunc_bf16 or None = none at all); ``x2_after_mask``: the seeded mistake.
    ``self.pre[stage]``: the float64 result before the stage's rounding (``self.rounded[stage]``: it is stored as bf16); ``self.noise[stage]`` = (largest |float32 - float64|
    before the rounding, elements whose rounded bits differ, elements) with ``measure``; ``self.alt``: what a stage gives with
    UNROUNDED projection weights on the same inputs (the power test)."""

    def __init__(self, model, sd, obs, n, heads, agg="max", rnd=to_bf16, wrnd=to_bf16, x2_after_mask=False, measure=False):
        self.pre, self.noise, self.alt, self.rounded, self.measure, self.rnd = {}, {}, {}, {}, measure, rnd
        w = net_weights(sd, model)
        obs = np.asarray(obs, dtype=np.float32)
        bs = obs.shape[0]
        in_dim = w["enc0"][0].shape[1]
        node = obs[:, :n * (in_dim + 3)].reshape(bs, n, in_dim + 3)
        feats, dm = node[:, :, 2:2 + in_dim].reshape(bs * n, in_dim), node[:, :, -1].reshape(bs * n)
        adj = radius_sets(node[:, :, :2])
        W = (lambda m: m) if wrnd is None else (lambda m: from_bf16(wrnd(m)))
        kind = w["kind"]
        closed = adj | np.eye(n, dtype=bool)[None] if kind == GATV2 else adj
        sources = [b * n + np.flatnonzero(closed[b, i]) for b in range(bs) for i in range(n)]
        rows = np.arange(bs * n)

        def lin(name, a, wb, relu, rounded=True):
            self.alt[name] = linear(a, wb[0], wb[1], relu)
            return self.stage(name, lambda dt: linear(a, W(wb[0]), wb[1], relu, dt), rounded)

        a0 = self.stage("enc0", lambda dt: encoder_layer0(feats, *w["enc0"], dt))
        h0 = lin("h0", a0, w["enc1"], True)
        if model == "hl_dgn":
            hc = w["c1"]["l"][0].shape[0]
            x = lin("xl1", h0, (np.concatenate([w["c1"]["l"][0], w["c1"]["r"][0]]), np.concatenate([w["c1"]["l"][1], w["c1"]["r"][1]])), False)
            xcat = self.stage("pool", lambda dt: pool(attend(GATV2, x[:, :hc], x[:, hc:], w["c1"]["att"], w["c1"]["bias"], sources,
                                                              rows, heads, dt), dm, n, agg, dt))
        else:
            agent = np.clip(obs[:, -1], 0, n - 1).astype(np.int64) + np.arange(bs) * n
            xl1 = lin("xl1", h0, source_side(w["c1"]), False)
            xr1 = lin("xr1", h0, w["c1"]["r"], False)
            o1 = lambda dt: attend(kind, xl1, xr1, w["c1"]["att"], w["c1"]["bias"], sources, rows, heads, dt)
            h1 = self.stage("h1", lambda dt: o1(dt) * dm.astype(dt)[:, None])
            x2 = h1[agent] if x2_after_mask else self.stage("x2", lambda dt: o1(dt)[agent])
            xl2 = lin("xl2", h1, source_side(w["c2"]), False)
            xr2 = lin("xr2", h1, w["c2"]["r"], False)
            x3 = self.stage("x3", lambda dt: attend(kind, xl2, xr2, w["c2"]["att"], w["c2"]["bias"], sources, rows, heads, dt)[agent])
            xcat = np.concatenate([h0[agent], x2, x3], axis=1)
        self.xcat = xcat
        nl = len(w["q"])
        if standard_heads(w):           # products of the bf16 operands kept in fp32; the rest on the fp32 parameters
            hid = [None, None]
            for k, h in enumerate(("q", "v")):
                (w0, b0), (w1, b1) = w[h][0], w[h][1]
                self.alt["hid0" + h] = linear(xcat, w0, b0, True)
                self.pre["hid0" + h] = linear(xcat, W(w0), b0, True)
                hid[k] = lambda dt, w0=w0, b0=b0, w1=w1, b1=b1: linear(linear(xcat, W(w0), b0, True, dt), w1, b1, True, dt)
        else:
            hq = hv = xcat
            for i in range(nl - 1):
                last = i + 2 == nl
                hq = lin(f"hq{i}q", hq, w["q"][i], True, rounded=not last)
                if w["dueling"]:
                    hv = lin(f"hq{i}v", hv, w["v"][i], True, rounded=not last)
            hid = [lambda dt: hq.astype(dt), lambda dt: hv.astype(dt)]
        self.logits = self.stage("logits", lambda dt: dueling_tail(hid[0](dt), hid[1](dt) if w["dueling"] else None, *w["q"][-1],
                                                                   *(w["v"][-1] if w["dueling"] else (None, None)), w["dueling"], dt),
                                 rounded=False)

    def stage(self, name, fn, rounded=True):
        pre = fn(np.float64)
        self.pre[name], self.rounded[name] = pre, rounded
        if self.measure:
            pre32 = fn(np.float32).astype(np.float64)
            flips = int((to_bf16(pre32) != to_bf16(pre)).sum()) if rounded else 0
            self.noise[name] = (float(np.abs(pre32 - pre).max()) if pre.size else 0.0, flips, pre.size)
        return pre if (self.rnd is None or not rounded) else from_bf16(self.rnd(pre))


# ---- cases -----------------------------------------------------------------------------------------------------------
def make_obs(n, bs, spread, seed, dm_zeros=0.2, zero_env=None, in_dim=5):
    """Observations [bs, n (in_dim + 3) + 1]: positions uniform on [0, spread]^2, the env's integer features, decision-maker
    flags with a share ``dm_zeros`` of zeros (env ``zero_env``: all zero), a random controlling index."""
    rng = np.random.RandomState(seed)
    obs = np.zeros((bs, (in_dim + 3) * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, in_dim + 3)
    m[:, :, 0:2] = rng.uniform(0, spread, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, max(n - 1, 1), size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = rng.uniform(size=(bs, n)) >= dm_zeros
    if zero_env is not None:
        m[zero_env, :, 7] = 0
    obs[:, -1] = rng.randint(0, n, size=bs)
    return obs


def agent_sets(n, bs, mode, seed):
    """bool [bs, n]: "all" = every node an agent, "some" = 1 - 8 agents per env."""
    if mode == "all":
        return np.ones((bs, n), dtype=bool)
    rng = np.random.RandomState(seed)
    live = np.zeros((bs, n), dtype=bool)
    for b in range(bs):
        live[b, rng.choice(n, size=min(n, rng.randint(1, 9)), replace=False)] = True
    return live


STD = ((128, 128), (128, 128))
# (id, model, n, bs, spread, hidden, heads, agents, (Q hidden, V hidden) or None = out_linear, aggregator, zero-flag env)
#   graphs: n = 1; n = 7 with isolated targets; n = 40 on [0, 0.25]^2: rows cut at 33 sources, asymmetric; n = 70 on [0, 0.3]^2:
#   two set words, capped.  agents: "index" = mel_ldgn_forward (one per row, the index column), "some" / "all" =
#   mel_ldgn_forward_agents.  (hidden, heads): (128, 4) LIST_16, V = 8; (128, 6) / (64, 6) GENERIC_48, V = 16 / 8; (128, 2) V = 4
#   and (64, 2) V = 2 GENERIC; (512, 2) V = 16 GENERIC.  HL-DGN's pool: NW = 8, NW = 4 (bs >= 2048, n = 5) and n > 64.
CASES = (
    ("ldgn-n1", "l_dgn", 1, 3, 1.0, 128, 4, "index", STD, None, None),
    ("ldgn-n7", "l_dgn", 7, 3, 1.0, 128, 4, "index", STD, None, None),
    ("ldgn-n40-some", "l_dgn", 40, 4, 0.25, 128, 4, "some", STD, None, 1),
    ("ldgn-n70-all", "l_dgn", 70, 3, 0.3, 128, 4, "all", STD, None, None),
    ("ldgn-n40-6x128-unequal", "l_dgn", 40, 4, 0.25, 128, 6, "some", ((64, 128), (128, 64)), None, None),
    ("ldgn-n40-6x64-onehidden", "l_dgn", 40, 4, 0.25, 64, 6, "index", ((64,), (128,)), None, None),
    ("ldgn-n70-2x128", "l_dgn", 70, 3, 0.3, 128, 2, "some", STD, None, None),
    ("ldgn-n7-2x64-all", "l_dgn", 7, 3, 1.0, 64, 2, "all", STD, None, 0),
    ("dgnr-n40-some", "dgn_r", 40, 4, 0.25, 128, 4, "some", STD, None, 2),
    ("dgnr-n70-2x64", "dgn_r", 70, 3, 0.3, 64, 2, "index", STD, None, None),
    ("dgnr-n7-6x128-all", "dgn_r", 7, 3, 1.0, 128, 6, "all", ((128,), (64,)), None, None),
    ("hldgn-max-n40", "hl_dgn", 40, 4, 0.25, 128, 4, "index", STD, "max", 1),
    ("hldgn-mean-n40", "hl_dgn", 40, 4, 0.25, 128, 4, "index", STD, "mean", 1),
    ("hldgn-add-n40-6x64", "hl_dgn", 40, 4, 0.25, 64, 6, "index", ((64, 128), (128, 64)), "add", 1),
    ("hldgn-max-n70-2x128", "hl_dgn", 70, 3, 0.3, 128, 2, "index", STD, "max", 2),
    ("hldgn-max-n5-bs2048", "hl_dgn", 5, 2048, 0.5, 64, 2, "index", STD, "max", 7),
    ("hldgn-n1", "hl_dgn", 1, 3, 1.0, 128, 4, "index", STD, "add", None),
    # an encoder wider than the GEMMs' fused producer: layer 0 by encoder_layer0_kernel into its own buffer; V = 16 on 64 lanes
    ("ldgn-n7-2x512-wide", "l_dgn", 7, 3, 1.0, 512, 2, "some", STD, None, 1),
    ("hldgn-mean-n7-2x512-wide", "hl_dgn", 7, 3, 1.0, 512, 2, "index", STD, "mean", None),
)
CASE_IDS = [c[0] for c in CASES]
WEIGHT_SEED = 31              # the weights of tests/test_gpu_bf16.py


def case_weights(case):
    """The oracle's random weights of a case; unequal Q / V hidden sizes: V from a second draw."""
    from oracle import net_oracle as no
    _, model, _, _, _, hidden, heads, _, duel, _, _ = case
    if duel is None:
        return no.init_weights(model, hidden=hidden, heads=heads, seed=WEIGHT_SEED, random_conv_bias=True, dueling=False)
    sd = no.init_weights(model, hidden=hidden, heads=heads, seed=WEIGHT_SEED, random_conv_bias=True, dueling_hidden=duel[0])
    if duel[1] != duel[0]:
        other = no.init_weights(model, hidden=hidden, heads=heads, seed=WEIGHT_SEED + 1, random_conv_bias=True, dueling_hidden=duel[1])
        for k in [k for k in sd if k.startswith("V.")]:
            del sd[k]
        sd.update({k: v for k, v in other.items() if k.startswith("V.")})
    return sd


def case_obs(case):
    cid, _, n, bs, spread, _, _, _, _, _, zero_env = case
    return make_obs(n, bs, spread, 200 + n + 7 * CASE_IDS.index(cid), zero_env=zero_env)


# ---- tolerances ------------------------------------------------------------------------------------------------------
# A_STAGE[stage]: the absolute floor of the bf16 rule, F32_TOL[stage]: the bound of an fp32 output = 8 x the largest difference
# between the float32 and the float64 evaluation of that reference stage BEFORE its rounding, over every case above on the
# case's own inputs.  tests/test_bf16_ref.py::test_tolerances_are_eight_times_the_measured_noise measures them and holds each
# constant to 8 times its measurement, a fifth less at the most (the float32 summation order is the BLAS build's) and never
# more than twice as much; the measurements stand beside the constants.  8: the kernels accumulate in fp32 in another order
# than either CPU evaluation and use the fast exp.
A_STAGE = {
    "enc0": 3.3e-5,      # measured 4.06e-6 (layer-0 rows reach 30: the degree feature)
    "h0": 1.5e-5,        # measured 1.83e-6
    "xl1": 1.2e-5,       # measured 1.41e-6 (lin_l / key | value / HL-DGN's lin_l | lin_r)
    "xr1": 1.1e-5,       # measured 1.32e-6
    "h1": 2.0e-5,        # measured 2.40e-6 (conv1 attention + bias + ReLU, times the flag)
    "x2": 1.6e-5,        # measured 1.92e-6
    "xl2": 9.0e-6,       # measured 1.12e-6
    "xr2": 8.6e-6,       # measured 1.07e-6
    "x3": 7.1e-6,        # measured 8.78e-7
    "pool": 8.3e-5,      # measured 1.03e-5 (HL-DGN "add" over 40 nodes)
    "hq0": 1.7e-5,       # measured 2.05e-6 (hidden head layers stored as bf16)
}
F32_TOL = {
    "hq_last": 6.3e-6,   # measured 7.77e-7: the last hidden head layer, stored fp32
    "logits": 2.5e-6,    # measured 3.07e-7: from the device's last hidden rows (general heads) or head input (standard heads)
}
