"""Plain-torch CPU references of the learn-path kernels of csrc/grad.hip (``mel_gat_forward`` / ``mel_gat_backward``,
``mel_pool_forward`` / ``mel_pool_backward``), the graphs their device tests run on and the list of those cases.  No project
kernel and none of the project's dense formulations is used here: tests/test_learn_ref.py compares this module WITH
``networks/common.py`` and ``oracle/net_oracle.py``, tests/test_gpu_learn_kernels.py compares the kernels with this module.

Every graph is ``bool [bs, n, n]`` with entry ``[b, i, j]`` = node j is a source of target i (row b*n + i of the kernels).
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from melissa_amd.env import episodes
from melissa_amd.networks import common

GATV2, TRANSFORMER = 0, 1                     # MEL_CONV_GATV2, MEL_CONV_TRANSFORMER (include/melissa_hip.h)
AGG_MAX, AGG_MEAN, AGG_ADD = 0, 1, 2          # MEL_AGG_*
TENSORS = ("out", "dxl", "dxv", "dxr", "datt", "dbias")


# ---- graphs --------------------------------------------------------------------------------------------------------
def radius(n, bs, spread, seed=None):
    """The project's radius rule (strict <, first 33 hits) over positions uniform on [0, spread]^2: with ``spread`` near the
    radius almost every pair is within reach, so the cap cuts rows and the graph stops being symmetric."""
    g = torch.Generator().manual_seed(n + bs if seed is None else seed)
    pos = torch.rand(bs, n, 2, generator=g) * spread
    return common.radius_adjacency(pos)


def later_ids(n, bs):
    """Sources of i = every j > i: no edge has its reverse; node n-1 has no source, node 0 has n-1."""
    return torch.triu(torch.ones(n, n, dtype=torch.bool), diagonal=1)[None].repeat(bs, 1, 1)


def ring(n, bs, hop):
    """The single source of i is (i + hop) % n."""
    adj = torch.zeros(n, n, dtype=torch.bool)
    i = torch.arange(n)
    adj[i, (i + hop) % n] = True
    return adj[None].repeat(bs, 1, 1)


def pack(adj):
    """bool [bs, n, n] -> int64 bit patterns of the uint64 source sets, [bs*n] up to 64 nodes and [bs*n, W] beyond
    (MEL_SET_WORDS layout: bit j % 64 of word j // 64 of row b*n + i)."""
    words = np.stack([episodes.adjacency_to_masks(a) for a in adj.numpy()])
    return torch.from_numpy(words.reshape((-1,) + words.shape[2:]).view(np.int64).copy())


def unpack(words, bs, n):
    """The inverse of :func:`pack`."""
    return torch.from_numpy(episodes.sets_to_bool(words.numpy(), n)).reshape(bs, n, n)


GRAPHS = {"radius": radius, "later_ids": later_ids, "ring": ring}


@functools.lru_cache(maxsize=None)
def graph(spec):
    """``spec`` = (builder name, arguments...) -> the graph, built once."""
    return GRAPHS[spec[0]](*spec[1:])


# (graph, (heads, channels) pairs) of the device test; tests/test_learn_ref.py checks what each graph is there for
GPU_CASES = (
    (("radius", 1, 3, 1.0), ((4, 128),)),                                   # n = 1: self-loop only / no source at all
    (("radius", 7, 3, 1.0), ((2, 64), (4, 128))),                           # isolated targets
    (("radius", 40, 2, 0.25), ((2, 64), (1, 256), (4, 128), (6, 64), (8, 128))),   # capped, asymmetric, one word
    (("radius", 70, 2, 0.3), ((2, 64), (4, 128), (6, 128))),                # capped, two words
    (("later_ids", 128, 1), ((2, 64), (64, 2))),                            # word 1 full, totally asymmetric, 127 sources
    (("ring", 128, 2, 65), ((2, 64),)),                                     # 126 of a graph's 128 edges cross the word boundary
    (("radius", 20, 60, 1.0), ((2, 64),)),                                  # 1 200 rows: grid-stride loop, 256 partial rows
)
CASES = tuple((spec, h, c, kind) for spec, shapes in GPU_CASES for h, c in shapes for kind in (GATV2, TRANSFORMER))


def case_id(case):
    spec, h, c, kind = case
    return f"{'gatv2' if kind == GATV2 else 'transformer'}-{spec[0]}{'x'.join(str(a) for a in spec[1:])}-{h}x{c}"


@functools.lru_cache(maxsize=None)
def inputs(spec, heads, channels):
    """The case's fp32 operands, drawn once and modified by nobody: xl, xv, xr and a DENSE grad_out [bs*n, HC], att * 0.3 and
    bias * 0.1 [HC]."""
    adj = graph(spec)
    rows, hc = adj.shape[0] * adj.shape[1], heads * channels
    g = torch.Generator().manual_seed(1000 * rows + hc + heads)
    r = lambda *shape: torch.randn(*shape, generator=g)
    return {"xl": r(rows, hc), "xv": r(rows, hc), "xr": r(rows, hc), "att": r(hc) * 0.3, "bias": r(hc) * 0.1, "gout": r(rows, hc)}


# ---- attention -----------------------------------------------------------------------------------------------------
def attention_ref(kind, xl, xv, xr, att, bias, adj_bool, gout, heads, dtype, relu_mask=None):
    """relu(conv + bias) of csrc/grad.hip as dense masked attention per graph, evaluated in ``dtype`` with torch autograd.
    GATv2: closed neighbourhood (self-loop added), e_ij = att . leaky_relu(x_r[i] + x_l[j], 0.2), aggregates x_l; Transformer:
    open neighbourhood, e_ij = q[i] . k[j] / sqrt(C) with xl = keys, xv = values, xr = queries.  Softmax over the sources with
    1e-16 added to the denominator; a target without a source aggregates 0.  ``att`` / ``xv`` are unused (None) for the other
    kind, ``bias`` may be None.

    Returns a dict: ``pre`` (before the ReLU), ``out``, and the gradients of ``gout`` ``dxl``, ``dxv``, ``dxr``, ``datt``,
    ``dbias`` (None where the kind has no such operand).  With ``relu_mask`` (bool / 0-1, the shape of out) the backward starts
    from ``gout * relu_mask`` at ``pre`` instead of going through this evaluation's own ReLU."""
    bs, n, _ = adj_bool.shape
    hc = xl.shape[1]
    c = hc // heads
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    lxl, lxr, lbias = leaf(xl), leaf(xr), leaf(bias)
    lxv = leaf(xv) if kind == TRANSFORMER else None
    latt = leaf(att) if kind == GATV2 else None
    zero = torch.zeros((), dtype=dtype)
    eye = torch.eye(n, dtype=torch.bool)
    rows = []
    for b in range(bs):                                   # a graph at a time: the pairwise GATv2 tensor is n^2 HC elements
        sl = slice(b * n, (b + 1) * n)
        src, tgt = lxl[sl].view(n, heads, c), lxr[sl].view(n, heads, c)
        if kind == GATV2:
            mask = (adj_bool[b] | eye)[..., None]
            e = (F.leaky_relu(tgt[:, None] + src[None, :], 0.2) * latt.view(heads, c)).sum(-1)          # [i, j, H]
            val = src
        else:
            mask = adj_bool[b][..., None]
            e = torch.einsum("ihc,jhc->ijh", tgt, src) / math.sqrt(c)
            val = lxv[sl].view(n, heads, c)
        e = e.masked_fill(~mask, -float("inf"))
        top = e.max(dim=1, keepdim=True).values
        top = torch.where(torch.isfinite(top), top, zero)                    # a target without a source
        p = torch.where(mask, torch.exp(e - top), zero)
        alpha = p / (p.sum(dim=1, keepdim=True) + 1e-16)
        rows.append(torch.einsum("ijh,jhc->ihc", alpha, val).reshape(n, hc))
    pre = torch.cat(rows)
    if lbias is not None:
        pre = pre + lbias
    out = torch.relu(pre)
    if relu_mask is None:
        out.backward(gout.to(dtype))
    else:
        pre.backward(gout.to(dtype) * relu_mask.to(dtype))
    grad = lambda t: None if t is None else t.grad
    return {"pre": pre.detach(), "out": out.detach(), "dxl": grad(lxl), "dxv": grad(lxv), "dxr": grad(lxr), "datt": grad(latt),
            "dbias": grad(lbias)}


def case_ref(case, dtype, relu_mask=None):
    """:func:`attention_ref` of a case of ``CASES`` on its own inputs."""
    spec, heads, channels, kind = case
    t = inputs(spec, heads, channels)
    return attention_ref(kind, t["xl"], t["xv"], t["xr"], t["att"], t["bias"], graph(spec), t["gout"], heads, dtype, relu_mask)


def bar(want, err32):
    """The project's bar for fp32-accurate kernels (tests/test_gpu_gemm_tiles.py), or twice what the plain fp32 evaluation of the
    same formula loses where that is more (twice: the summation orders differ)."""
    return max(4e-6 * max(1.0, float(want.abs().max())), 2.0 * err32)


# ---- pool ----------------------------------------------------------------------------------------------------------
def pool_ref(x, dm, n, agg, dtype):
    """x [bs*n, hc], dm [bs*n] -> (pooled [bs, hc], arg [bs, hc] int64): max / mean / add over the graph's nodes of x * dm; mean
    divides by n; arg = node of the FIRST maximum (numpy's argmax), max only (else None)."""
    hc = x.shape[1]
    v = (x.to(dtype) * dm.to(dtype)[:, None]).view(-1, n, hc)
    if agg == AGG_MAX:
        arg = torch.from_numpy(np.argmax(v.numpy(), axis=1))
        return v.gather(1, arg[:, None, :])[:, 0], arg
    total = v.sum(dim=1)
    return (total / n if agg == AGG_MEAN else total), None


def pool_ref_backward(grad_pooled, dm, arg, n, agg, dtype):
    """grad_pooled [bs, hc] -> dx [bs*n, hc]: to the first maximum alone (max), divided by n (mean), to every node (add), each
    times the node's dm."""
    bs, hc = grad_pooled.shape
    g = grad_pooled.to(dtype)
    if agg == AGG_MAX:
        dx = torch.zeros(bs, n, hc, dtype=dtype).scatter_(1, arg[:, None, :], g[:, None, :])
    else:
        dx = (g / n if agg == AGG_MEAN else g)[:, None, :].expand(bs, n, hc)
    return (dx * dm.to(dtype).view(bs, n, 1)).reshape(bs * n, hc)


POOL_SHAPES = ((3, 1, 128), (3, 20, 384), (2, 128, 100), (1, 7, 64))         # (bs, n, hc)


@functools.lru_cache(maxsize=None)
def pool_inputs(bs, n, hc):
    """x randn, dm 0/1 with about a fifth zeros, a dense grad_pooled."""
    g = torch.Generator().manual_seed(bs + n + hc)
    x = torch.randn(bs * n, hc, generator=g)
    dm = (torch.rand(bs * n, generator=g) >= 0.2).float()
    return x, dm, torch.randn(bs, hc, generator=g)
