"""The grid of (hidden, heads) shapes the HIP path accepts, the inputs every shape is run on, the float64 reference the kernels
are held to and the bounds - shared by tests/test_shape_grid_ref.py (CPU: the reference itself, the measurement behind every
bound, the mutants the bounds must catch) and tests/test_gpu_shape_grid.py (the kernels).  No GPU, no project kernel.

The reference is ``oracle/net_oracle.py`` evaluated with ``dtype=torch.float64``.  ``reference64`` below is a third, dense
formulation of the same three forwards that takes the SOURCE SETS as an argument, so that a mistake can be seeded into it
(``MUTANTS``); unmutated it agrees with the oracle's float64 evaluation to 1e-12 (tests/test_shape_grid_ref.py).
"""
import functools
import math

import numpy as np
import torch

from melissa_amd.shapes import head_lanes, hip_shape_supported
from oracle import net_oracle as no

# ---- the shapes ------------------------------------------------------------------------------------------------------
ACCEPTED = ((64, 2), (64, 4), (64, 6), (64, 8), (64, 16), (128, 1), (128, 2), (128, 4), (128, 6), (128, 8),
            (256, 1), (256, 2), (256, 4), (512, 1), (512, 2))
SHAPES = tuple((hidden, heads) for hidden in range(64, 577, 64) for heads in range(1, 65) if hip_shape_supported(hidden, heads)[0])
assert SHAPES == ACCEPTED, f"melissa_amd.shapes.hip_shape_supported now accepts {sorted(set(SHAPES) ^ set(ACCEPTED))} differently"
ALL_AGGREGATORS = ((64, 2), (128, 8), (256, 4), (512, 1))          # HL-DGN mean / add (max: every shape)
POOL4_SHAPES = ((64, 2), (128, 2), (128, 4), (256, 4))             # one pair per V = 2, 4, 8, 16: the NW = 4 pool launch


def models_of(shape):
    """(model, aggregator) cells of a shape."""
    cells = [("l_dgn", "max"), ("dgn_r", "max"), ("hl_dgn", "max")]
    return cells + ([("hl_dgn", "mean"), ("hl_dgn", "add")] if shape in ALL_AGGREGATORS else [])


CELLS = tuple((h, k, m, a) for h, k in SHAPES for m, a in models_of((h, k)))
cell_id = lambda c: f"{c[0]}x{c[1]}-{c[2]}" + (f"-{c[3]}" if c[2] == "hl_dgn" else "")
model_key = lambda model, agg: model if model != "hl_dgn" else f"hl_dgn-{agg}"
WEIGHT_SEED = 17


@functools.lru_cache(maxsize=None)
def weights(model, hidden, heads):
    return no.init_weights(model, hidden=hidden, heads=heads, seed=WEIGHT_SEED, random_conv_bias=True)


# ---- the inputs ------------------------------------------------------------------------------------------------------
# name -> (n, bs, spread of the positions).  n40: rows cut at 33 sources, asymmetric adjacency; n70: two set words, an agent in
# word 1; n7: 48 envs, past the 40 from which the agents forward takes the node-feature table at n = 7 (n7h: HL-DGN's rows are
# every node of every env, so it takes the table from 80 envs on: 96); n5: the NW = 4 pool launch (bs >= 2048); l20, l70: the
# learn path.
# The learn path's cases keep env 1 on the spread of the others: inside the box every target has the same sources, the pooled
# maximum is a near tie between nodes, and a gradient through a tie is not a function a rounding bound can be stated for.
CASES = {"n40": (40, 4, 0.25), "n70": (70, 3, 0.3), "n7": (7, 48, 0.6), "n7h": (7, 96, 0.6), "n5": (5, 2048, 0.5),
         "l20": (20, 5, 0.6), "l70": (70, 3, 0.3)}
FORWARD_CASES = ("n40", "n70")
TABLE_CASE, TABLE_CASE_HL, POOL4_CASE = "n7", "n7h", "n5"
LEARN_CASES = ("l20", "l70")
CAP_ROW = 33                      # sources of a row the radius rule cut (GATv2: 32 neighbours + the self loop, or 33 + it)


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """-> (obs [bs, 8 n + 1] float32 with integer features, agent sets bool [bs, n]).
    env 0: one agent, node 0, alone in a corner with flag 1 (DGN-R: a target without a source; GATv2: the self loop alone);
    env 1: every node an agent, all of them inside a 0.1 box (n >= 34: every row is cut - targets below 33 keep 32 neighbours,
      the others lose their own slot and keep 33), the index column on the LAST node, whose flag is 0 (x_2 is taken before the
      mask); the other envs: positions on [0, spread]^2, 2 - 6 agents, from n = 65 one of them in the second set word;
    flags 0 on about a fifth of the nodes (at least one 0 and one 1 per env from env 1 on)."""
    n, bs, spread = CASES[name]
    rng = np.random.RandomState(1000 + n + (500 if name.startswith("l") else 0))
    obs = np.zeros((bs, 8 * n + 1), dtype=np.float32)
    m = obs[:, :-1].reshape(bs, n, 8)
    m[:, :, 0:2] = rng.uniform(0, spread, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, min(n, 9), size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = rng.uniform(size=(bs, n)) >= 0.2
    m[1:, 0, 7], m[1:, n - 1, 7] = 1, 0
    m[0, :, 0:2] = 0.6 + rng.uniform(0, min(spread, 0.4), size=(n, 2))
    m[0, 0, 0:2], m[0, 0, 7] = 0.0, 1
    if not name.startswith("l"):
        m[1, :, 0:2] = 0.3 + rng.uniform(0, 0.1, size=(n, 2))
    live = np.zeros((bs, n), dtype=bool)
    for b in range(bs):
        live[b, rng.choice(n, size=rng.randint(2, min(n, 6) + 1), replace=False)] = True
        if n > 64:
            live[b, n - 1 - b] = True
    live[0], live[1] = False, True
    live[0, 0] = True
    index = np.array([rng.choice(np.flatnonzero(row)) for row in live])
    index[1] = n - 1
    obs[:, -1] = index
    return obs, live


def agent_words(live):
    """bool [bs, n] -> the int64 bit patterns hip_forward_agents takes: [bs], or [bs, words] beyond 64 nodes."""
    bs, n = live.shape
    words = (n + 63) // 64
    masks = np.zeros((bs, words), dtype=np.uint64)
    for b, a in zip(*np.nonzero(live)):
        masks[b, a // 64] |= np.uint64(1) << np.uint64(a % 64)
    am = masks.view(np.int64)
    return am[:, 0].copy() if words == 1 else am


def case_rows(name):
    """The (env, agent) pairs of a case's logits rows: the index column's first, then the agent sets' by env and agent id - the
    row order of hip_forward followed by hip_forward_agents."""
    obs, live = case_inputs(name)
    n = live.shape[1]
    index = [(b, int(a)) for b, a in enumerate(np.clip(obs[:, -1], 0, n - 1).astype(np.int64))]
    return index + [(int(b), int(a)) for b, a in zip(*np.nonzero(live))]


def plan_counts(adj, live, gat):
    """(sum |U1|, sum |U2|, agent rows) of the agents forward from the oracle's adjacency, as mel_forward_tap kind 2 reports
    them: U1 = the agents' closed neighbourhoods (conv1's targets), U2 = U1's (the encoder's rows)."""
    adj = np.asarray(adj)
    closed = adj | np.eye(adj.shape[1], dtype=bool)[None]
    u1 = np.stack([closed[b, live[b]].any(0) for b in range(len(live))])
    u2 = np.stack([closed[b, u1[b]].any(0) for b in range(len(live))])
    return int(u1.sum()), int(u2.sum()), int(live.sum())


# ---- the float64 oracle ----------------------------------------------------------------------------------------------
def oracle(model, agg, sd, obs, n, heads, dtype=torch.float64, formulation="edges", rows=None):
    """-> (logits, head input, adjacency) of oracle/net_oracle.py as float64 numpy (evaluated in ``dtype``)."""
    torch.set_num_threads(8)
    with torch.no_grad():
        if model == "hl_dgn":
            out, mid = no.hldgn_forward(sd, obs, n, heads=heads, aggregator=agg, formulation=formulation, dtype=dtype,
                                        return_intermediates=True)
            head = mid["pooled"]
        else:
            fwd = no.ldgn_forward if model == "l_dgn" else no.dgnr_forward
            out, mid = fwd(sd, obs, n, heads=heads, formulation=formulation, dtype=dtype, rows=rows, return_intermediates=True)
            head = mid["x_cat"]
    return out.double().numpy(), head.double().numpy(), mid["adj"].numpy()


def learn_batch(bs):
    """Actions and targets of the squared-error loss of tests/test_gpu_grad.py."""
    return np.random.RandomState(5).randint(0, 2, bs), np.random.RandomState(6).uniform(-1, 1, bs).astype(np.float32)


def oracle_grads(model, agg, sd, obs, n, heads, dtype=torch.float64, formulation="edges"):
    """loss = mean((Q(obs)[act] - target)^2) through the oracle in ``dtype`` -> (logits, loss, {name: gradient}) as float64."""
    torch.set_num_threads(8)
    bs = obs.shape[0]
    act, target = learn_batch(bs)
    leaves = {k: v.clone().to(dtype).requires_grad_(True) for k, v in sd.items()}
    kw = dict(aggregator=agg) if model == "hl_dgn" else {}
    fwd = {"l_dgn": no.ldgn_forward, "dgn_r": no.dgnr_forward, "hl_dgn": no.hldgn_forward}[model]
    logits = fwd(leaves, obs, n, heads=heads, formulation=formulation, dtype=dtype, **kw)
    loss = (logits[torch.arange(bs), torch.from_numpy(act)] - torch.from_numpy(target).to(dtype)).pow(2).mean()
    loss.backward()
    grads = {k: (None if v.grad is None else v.grad.double().numpy()) for k, v in leaves.items()}
    return logits.detach().double().numpy(), float(loss.detach()), grads


ZERO_GRAD = 1e-10
# A gradient is a sum of products of activations and back-propagated differences whose sizes follow the network's largest
# gradient entry; where the sum cancels (lin_r / query reach the loss through the softmax alone: a hundredth of lin_l's
# gradient and less) the rounding error follows the terms, not the result.  Such a tensor is scaled by SMALL_GRAD of the
# network's largest gradient entry instead of by its own.
SMALL_GRAD = 1e-2


def grad_errors(got, want):
    """{name: (|got - want| max, scale)} - scale: the tensor's largest float64 entry, at least SMALL_GRAD of the network's - over
    the tensors whose float64 gradient is not zero: None (lin_skip, which TransformerConv never uses) or below ZERO_GRAD of the largest gradient entry of the network (a key bias shifts every
    score of a target alike: its float64 gradient is the rounding of a sum that is exactly 0)."""
    out = {}
    top = max(float(np.abs(w).max()) for w in want.values() if w is not None)
    for k, w in want.items():
        if w is None or np.abs(w).max() <= ZERO_GRAD * top:
            continue
        out[k] = (float(np.abs(np.asarray(got[k], dtype=np.float64) - w).max()), max(float(np.abs(w).max()), SMALL_GRAD * top))
    return out


# ---- a dense float64 formulation with the source sets as an argument: the mutants -------------------------------------
MUTANTS = ("lane_dropped", "heads_exchanged", "x2_after_mask", "no_self_loop", "mean_over_live", "last_source_dropped")


def mutant_applies(mutant, model, agg, heads, n):
    return {"lane_dropped": True, "heads_exchanged": heads > 1, "x2_after_mask": model != "hl_dgn",
            "no_self_loop": model != "dgn_r", "mean_over_live": model == "hl_dgn" and agg == "mean",
            "last_source_dropped": n > CAP_ROW}[mutant]


def mutate_weights(sd, model, hidden, heads, mutant):
    """(a) lane_dropped: the channels of ONE lane of the last head leave its score sum - ``hidden / lanes_per_head`` consecutive
    entries of ``att`` (GATv2) or of the query (its weight rows and bias; DGN-R) set to 0, in every conv; the lane is the head's
    second where a head has more than one.  (b) heads_exchanged: the ``att`` / query blocks of the first and the last head
    swapped."""
    sd = {k: v.clone() for k, v in sd.items()}
    lanes = head_lanes(heads, hidden)[0]
    per = hidden // lanes
    lo = (heads - 1) * hidden + (per if lanes > 1 else 0)
    a, b = slice(0, hidden), slice((heads - 1) * hidden, heads * hidden)
    for conv in ("conv1", "conv2"):
        names = [f"{conv}.lin_query.weight", f"{conv}.lin_query.bias"] if model == "dgn_r" else [f"{conv}.att"]
        for name in names:
            if name not in sd:
                continue
            t = sd[name].view(heads * hidden, -1)                # (a view: writes reach sd[name])
            if mutant == "lane_dropped":
                t[lo:lo + per] = 0
            else:
                first = t[a].clone()
                t[a] = t[b]
                t[b] = first
    return sd


def reference64(model, agg, sd, obs, n, heads, rows=None, mutant=None):
    """The three forwards in float64, dense, on explicit source sets -> (logits, head input) as numpy.  ``mutant``:
    (c) x2_after_mask, (d) no_self_loop (GATv2), (e) mean_over_live (HL-DGN mean divided by the live-flag count),
    (f) last_source_dropped (every row of at least 33 sources loses its last one).  (a) / (b): ``mutate_weights``."""
    with torch.no_grad():
        logits, head, _ = _dense64(model, agg, {k: v.double() for k, v in sd.items()}, obs, n, heads, rows, mutant)
    return logits.numpy(), head.numpy()


def _dense64(model, agg, w, obs, n, heads, rows=None, mutant=None, band=0.0):
    """-> (logits, head input, flipped) as tensors, differentiable in the double weights ``w``.  ``band`` > 0: every ReLU and
    leaky-ReLU argument closer to 0 than ``band`` takes the slope of the OTHER side (``flipped`` counts them)."""
    torch.set_num_threads(8)
    flipped = [0]

    def positive(x):
        on = x.detach() > 0
        if band:
            near = x.detach().abs() < band
            flipped[0] += int(near.sum())
            on = on ^ near
        return on

    relu = lambda x: x * positive(x)
    obs = np.asarray(obs, dtype=np.float32)
    bs = obs.shape[0]
    node = torch.from_numpy(obs[:, :-1]).reshape(bs, n, 8)
    feats, dm = node[:, :, 2:7].double(), node[:, :, 7:8].double()
    adj = no.radius_adjacency(node[:, :, :2])
    gat = model != "dgn_r"
    src = adj | torch.eye(n, dtype=torch.bool)[None] if gat and mutant != "no_self_loop" else adj.clone()
    if mutant == "last_source_dropped":
        full = src.sum(2) >= CAP_ROW
        last = (src * torch.arange(1, n + 1)).argmax(2)
        b, i = torch.nonzero(full, as_tuple=True)
        src[b, i, last[b, i]] = False
    lin = lambda name, x: x @ w[name + ".weight"].t() + w[name + ".bias"]

    def conv(prefix, x):
        if gat:
            xl, xr = lin(prefix + ".lin_l", x).view(bs, n, heads, -1), lin(prefix + ".lin_r", x).view(bs, n, heads, -1)
            e = torch.zeros(bs, n, n, heads, dtype=torch.float64)
            for h in range(heads):                                  # (per head: the [bs, i, j, C] block stays small)
                s = xr[:, :, None, h] + xl[:, None, :, h]
                e[..., h] = torch.where(positive(s), s, 0.2 * s) @ w[prefix + ".att"][0, h]
            v = xl
        else:
            q, k = lin(prefix + ".lin_query", x).view(bs, n, heads, -1), lin(prefix + ".lin_key", x).view(bs, n, heads, -1)
            v = lin(prefix + ".lin_value", x).view(bs, n, heads, -1)
            e = torch.einsum("bihc,bjhc->bijh", q, k) / math.sqrt(q.shape[-1])
        e = e.masked_fill(~src[..., None], -float("inf"))
        top = e.max(dim=2, keepdim=True).values
        top = torch.where(torch.isfinite(top), top, torch.zeros((), dtype=torch.float64))
        p = torch.where(src[..., None], torch.exp(e - top), torch.zeros((), dtype=torch.float64))
        out = torch.einsum("bijh,bjhc->bihc", p / (p.sum(2, keepdim=True) + 1e-16), v).reshape(bs, n, -1)
        return relu(out + w[prefix + ".bias"] if gat else out)

    def heads_of(x):
        mlp = lambda p, y: lin(p + ".model.4", relu(lin(p + ".model.2", relu(lin(p + ".model.0", y)))))
        q = mlp("Q", x)
        return q - q.mean(1, keepdim=True) + mlp("V", x)

    x = relu(lin("encoder.model.2", relu(lin("encoder.model.0", feats))))
    o1 = conv("conv1", x)
    h1 = o1 * dm
    if model == "hl_dgn":
        if agg == "max":
            head = h1.max(1).values
        elif agg == "add":
            head = h1.sum(1)
        else:
            head = h1.sum(1) / (dm.sum(1) if mutant == "mean_over_live" else n)
    else:
        pairs = np.asarray(rows if rows is not None else list(enumerate(np.clip(obs[:, -1], 0, n - 1).astype(np.int64))))
        b, g = torch.from_numpy(pairs[:, 0].astype(np.int64)), torch.from_numpy(pairs[:, 1].astype(np.int64))
        x3 = conv("conv2", h1)
        head = torch.cat([x[b, g], (h1 if mutant == "x2_after_mask" else o1)[b, g], x3[b, g]], dim=1)
    return heads_of(head), head, flipped[0]


# The activations have kinks, and a float32 evaluation puts an argument that is 0 up to its rounding on either side: the value
# is the same, the slope is not, and the gradients move by that element's term - which no rounding bound covers.  So a gradient
# bound gets, per tensor, what flipping EVERY argument within KINK_BAND of 0 moves the float64 gradient by (zero for most cases:
# no such argument).  KINK_BAND: one float32 unit in the last place at 1, the size the terms of such an argument reach - the
# rounding a float32 sum of them carries whatever its order.
KINK_BAND = 2.0 ** -23


def kink_allowance(model, agg, sd, obs, n, heads):
    """-> ({name: largest |gradient with the near-kink slopes flipped - gradient|}, near-kink arguments) of the learn loss."""
    bs = obs.shape[0]
    act, target = learn_batch(bs)
    grads = []
    for band in (0.0, KINK_BAND):
        leaves = {k: v.clone().double().requires_grad_(True) for k, v in sd.items()}
        logits, _, flipped = _dense64(model, agg, leaves, obs, n, heads, band=band)
        (logits[torch.arange(bs), torch.from_numpy(act)] - torch.from_numpy(target).double()).pow(2).mean().backward()
        grads.append({k: (None if v.grad is None else v.grad.numpy()) for k, v in leaves.items()})
    return {k: (0.0 if g is None else float(np.abs(grads[1][k] - g).max())) for k, g in grads[0].items()}, flipped


def run_mutant(model, agg, sd, obs, n, hidden, heads, rows, mutant):
    if mutant in ("lane_dropped", "heads_exchanged"):
        return reference64(model, agg, mutate_weights(sd, model, hidden, heads, mutant), obs, n, heads, rows)
    return reference64(model, agg, sd, obs, n, heads, rows, mutant)


# ---- the bounds ------------------------------------------------------------------------------------------------------
# Every bound is 8 x the largest difference between the oracle at float32 and at float64 on the grid's own inputs: every cell of
# CELLS, both formulations; logits and head input over FORWARD_CASES, TABLE_CASE / TABLE_CASE_HL, LEARN_CASES (and POOL4_CASE on POOL4_SHAPES),
# gradients and loss over LEARN_CASES.  8, the factor of tests/bf16_ref.py: the kernels accumulate in fp32 in another order than
# either CPU evaluation and use the hardware exp2.  tests/test_shape_grid_ref.py::test_bounds_are_eight_times_the_measured_noise
# measures them and holds each constant to 8 times its measurement - a fifth less at the most (the float32 summation order is
# the BLAS build's), never more than twice as much; the measurements stand beside the constants.  None exceeds what the suite
# asserted before: 1e-4 on logits, 2e-4 x scale + 1e-7 on gradients.
OLD_LOGITS_BAR, OLD_GRAD_BAR = 1e-4, 2e-4
LOGITS_TOL = {             # absolute
    "l_dgn": 4.0e-7,         # measured 5.04e-08
    "dgn_r": 5.2e-7,         # measured 6.44e-08
    "hl_dgn-max": 3.9e-7,    # measured 4.88e-08
    "hl_dgn-mean": 2.0e-7,   # measured 2.45e-08
    "hl_dgn-add": 4.7e-6,    # measured 5.85e-07 (logits reach 1.7: sums over 70 nodes)
}
HEAD_INPUT_TOL = {         # absolute: x_cat of L-DGN / DGN-R, the pooled rows of HL-DGN
    "l_dgn": 9.1e-6,         # measured 1.14e-06 (x_1: encoder rows reach 10)
    "dgn_r": 9.1e-6,         # measured 1.14e-06 (the same x_1)
    "hl_dgn-max": 1.0e-5,    # measured 1.28e-06
    "hl_dgn-mean": 2.2e-6,   # measured 2.71e-07
    "hl_dgn-add": 9.1e-5,    # measured 1.14e-05
}
LOSS_TOL = {               # relative to max(1, |loss|)
    "l_dgn": 5.4e-7,         # measured 6.79e-08
    "dgn_r": 6.5e-7,         # measured 8.17e-08
    "hl_dgn-max": 4.5e-7,    # measured 5.62e-08
    "hl_dgn-mean": 2.6e-7,   # measured 3.28e-08
    "hl_dgn-add": 1.7e-6,    # measured 2.19e-07
}
GRAD_TOL = {               # relative to grad_errors' scale of the tensor, beyond its kink_allowance; the largest over a model's tensors
    "l_dgn": 9.9e-6,         # measured 1.24e-06
    "dgn_r": 5.6e-6,         # measured 7.06e-07
    "hl_dgn-max": 2.8e-5,    # measured 3.50e-06
    "hl_dgn-mean": 1.2e-5,   # measured 1.51e-06
    "hl_dgn-add": 1.2e-5,    # measured 1.52e-06
}
ZERO_GRAD_TOL = 1e-7       # absolute, the suite's present bar: a gradient the float64 oracle gives as zero (grad_errors)


def grad_bound(key, scale, own, kinks=0.0):
    """The bound of a gradient tensor: GRAD_TOL x its scale - never above the suite's former 2e-4 x max|grad| + 1e-7 - plus its
    kink_allowance (the term the arithmetic gives, not a measured one: the former bar had no place for it either, and the one
    case of the grid with a slope that flips on the device - 64 x 8 L-DGN, l20, a leaky-ReLU argument of 7.7e-9 - misses the
    former bar on conv1.lin_r by it)."""
    return min(GRAD_TOL[key] * scale, OLD_GRAD_BAR * own + 1e-7) + kinks
BF16_TOL = 2e-2            # the project's bf16 bar (tests/test_gpu_bf16.py); the stage-by-stage test owns that path
