"""References and bars for the direct GEMM tests (tests/test_gemm_ref.py without a GPU, tests/test_gpu_gemm_edges.py on one).

Operands whose rows span 25 (A) and 13 (W, bias) binary orders of magnitude, so that every row tile holds rows of every scale
and an error confined to the small rows cannot hide behind the large ones; the float64 product with the sum of the terms'
magnitudes S beside it; the statistic max |got - want| / S; and the yardstick the bars are computed from: the same statistic
of a plain fp32 evaluation that adds one term at a time in k order (``seq32_stat``).  Nothing here comes from the library.

    exact-fp32 kernels      stat <= 2 x seq32_stat                      (only the summation order differs)
    split-bf16 kernels      stat <= 2 x seq32_stat + (2 + 2^-8) x 2^-24 (the three dropped partial products, below)
    bf16 kernel, fp32 out   as the exact-fp32 kernels (products of bf16 values are exact in fp32)
    bf16 kernel, bf16 out   |err| <= bar x S + 2^-8 x |want|             (one rounding to nearest: bf16 keeps 8 significant bits,
                                                                         half a unit in the last place is 2^-8)

The split kernels' added term: with x = x_hi + x_mid + x_lo, |x_mid| <= 2^-8 |x|, |x_lo| <= 2^-16 |x| (round to nearest, 8
significant bits each), the dropped products a_mid w_lo + a_lo w_mid + a_lo w_lo are at most (2^-24 + 2^-24 + 2^-32) |a w|.

A bar is never allowed above the worst-case bound of any summation order, (K + 2) x 2^-24: it can admit no more than rounding
explains (``bar`` asserts it).
"""
import functools
import types

import numpy as np
import torch

U = 2.0 ** -24
SPLIT_TERM = (2 + 2.0 ** -8) * U
BF16_ROUND = 2.0 ** -8              # unit roundoff of bf16: 8 significant bits, round to nearest
F32_SENTINEL = 0x7FC0BEEF           # a quiet NaN with a payload no arithmetic produces
BF16_SENTINEL = 0x7FD7              # likewise, as bf16


def operands(m, n, k, seed, bf16=False):
    """a [m, k], w [n, k], b [n] fp32 on the CPU: randn (w / sqrt(k)), then row i of a times 2^((i % 25) - 12), row j of w and
    b[j] times 2^((j % 13) - 6): exact scalings.  ``bf16``: a and w are rounded to bf16 values first (and stay bf16 values)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    if bf16:
        a, w = a.bfloat16().float(), w.bfloat16().float()
    sa = torch.ldexp(torch.ones(m), (torch.arange(m) % 25) - 12)
    sw = torch.ldexp(torch.ones(n), (torch.arange(n) % 13) - 6)
    return a * sa[:, None], w * sw[:, None], b * sw


def reference(a, w, b, relu=False):
    """want = a w^T + b and S = |a| |w|^T + |b| in float64 (b may be None); ReLU on want only."""
    a, w = a.double(), w.double()
    want, S = a @ w.t(), a.abs() @ w.abs().t()
    if b is not None:
        want, S = want + b.double(), S + b.double().abs()
    return (torch.relu(want) if relu else want), S


def stat(got, want, S):
    """max_ij |got_ij - want_ij| / S_ij (NaN if any element of got is)."""
    r = (got.double() - want).abs() / S
    return float("nan") if bool(torch.isnan(r).any()) else float(r.max())


def sample_rows(m, seed=0):
    """Every row up to 1 024 of them, else the first 64, the last 65 and 512 seeded random ones."""
    if m <= 1024:
        return np.arange(m)
    rnd = np.random.RandomState(seed).choice(m, 512, replace=False)
    return np.unique(np.concatenate([np.arange(64), np.arange(m - 65, m), rnd]))


def seq32(a, w, b):
    """a w^T + b in plain fp32, one term at a time in k order (each product rounded, then added), the bias last."""
    at, wt = np.ascontiguousarray(a.numpy().T), np.ascontiguousarray(w.numpy().T)
    acc = np.zeros((at.shape[1], wt.shape[1]), np.float32)
    tmp = np.empty_like(acc)
    for kk in range(at.shape[0]):
        np.multiply(at[kk][:, None], wt[kk][None, :], out=tmp)
        acc += tmp
    if b is not None:
        acc += b.numpy()
    return torch.from_numpy(acc)


def seq32_stat(a, w, b, rows=None):
    """``stat`` of ``seq32`` over ``rows`` of a (``sample_rows`` if None)."""
    rows = torch.from_numpy(np.asarray(sample_rows(a.shape[0]) if rows is None else rows))
    sub = a[rows]
    want, S = reference(sub, w, b)
    return stat(seq32(sub, w, b), want, S)


def bar(seq, k, split=False):
    """The bar of a kernel from the yardstick ``seq`` = seq32_stat of its operands."""
    out = 2 * seq + (SPLIT_TERM if split else 0.0)
    assert 0 < out <= (k + 2) * U, f"bar {out / U:.1f} x 2^-24 exceeds what rounding explains at K = {k}: {k + 2} x 2^-24"
    return out


def product(a, w, b):
    """Float64 reference, S and the yardstick of one product a w^T (+ b), with its operands."""
    want, S = reference(a, w, b)
    return types.SimpleNamespace(m=a.shape[0], n=w.shape[0], k=a.shape[1], a=a, w=w, b=b, want=want, S=S, seq=seq32_stat(a, w, b))


@functools.lru_cache(maxsize=None)
def case(m, n, k, bf16=False, bias=True):
    """``product`` of ``operands(m, n, k)``, computed once and shared (nothing modifies it)."""
    a, w, b = operands(m, n, k, seed=m + n + k, bf16=bf16)
    return product(a, w, b if bias else None)


@functools.lru_cache(maxsize=None)
def linear_case(rows, out_f, in_f):
    """A linear layer y = x w^T + b with the gradient dy of its output: x, w, b from ``operands``; dy [rows, out_f] is the
    transpose of another draw's a, so that its COLUMNS span the 25 magnitudes (the rows of dW = dy^T x then do, and the terms
    of dX = dy w).  The three products with their references: y (rows x out x in), dx (rows x in x out), dw (out x in x rows)."""
    y = case(rows, out_f, in_f)
    dy_t = operands(out_f, 1, rows, seed=rows + out_f + in_f + 1)[0]
    dy = dy_t.t().contiguous()
    return types.SimpleNamespace(x=y.a, w=y.w, b=y.b, dy=dy, y=y, dx=product(dy, y.w.t().contiguous(), None),
                                 dw=product(dy_t, y.a.t().contiguous(), None), db=dy.double().sum(0))


def guarded(m, n, ld, dtype=torch.float32, sentinel=None, fill=None, device="cpu"):
    """One allocation [m + 4, ld]: two guard rows, the [m, ld] block, two guard rows, every element the sentinel bit pattern.
    Returns the buffer, the pointer of its [m, n] view buf[2 : m + 2, :n], and ``check()``, which asserts that everything
    outside that view still holds the sentinel bit for bit.  ``fill`` [m, n]: an input - the view holds it, the padding columns
    and guard rows around it the sentinel (a NaN)."""
    assert ld >= n and dtype in (torch.float32, torch.bfloat16)
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    if sentinel is None:
        sentinel = F32_SENTINEL if dtype == torch.float32 else BF16_SENTINEL
    bits = 32 if dtype == torch.float32 else 16
    word = sentinel - (1 << bits) if sentinel >> (bits - 1) else sentinel           # the pattern as a signed integer
    buf = torch.full((m + 4, ld), word, dtype=ints, device=device).view(dtype)
    assert bool(torch.isnan(buf).all())
    if fill is not None:
        buf[2:m + 2, :n] = fill.to(device=device, dtype=dtype)
    outside = torch.ones(m + 4, ld, dtype=torch.bool, device=device)
    outside[2:m + 2, :n] = False

    def check(what=""):
        bad = (buf.view(ints) != word) & outside
        if bool(bad.any()):
            r, c = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{what}: {int(bad.sum())} elements outside [:{m}, :{n}] were written, the first at row {r - 2} "
                                 f"column {c} of the [{m}, {ld}] block")

    return buf, buf[2:m + 2, :n].data_ptr(), check


def interior(buf, m, n):
    """The [m, n] view of a ``guarded`` buffer."""
    return buf[2:m + 2, :n]


# ---- the shapes of tests/test_gpu_gemm_edges.py (m, n, k), shared with tests/test_gemm_ref.py ----------------------------------
STREAM_SHAPES = [(577, 384, 96), (577, 384, 160), (577, 384, 288), (577, 384, 1152),
                 (11009, 384, 96), (11009, 384, 160), (11009, 384, 1152)]
# (m, n, k, ksplit, bias)
SPLITK_CASES = [(1, 64, 192, 2, True), (577, 128, 480, 3, True), (577, 128, 1024, 16, False), (128, 1152, 3584, 16, False),
                (128, 1152, 2560, 16, False)]
EDGE_ROWS = [63, 64, 65, 128]                                    # x 128 x 96
SPLIT_SHAPES = [(333, 384, 256), (129, 256, 128)]
BF16_SHAPES = [(77, 64, 64), (129, 256, 128)]
# mel_gemm_f32_t as (rows, out, in): dX is the product (rows, in, out), dW (out, in, rows)
T_CASES = [(96, 64, 64), (33, 128, 64)]
# hip_linear as (rows, out, in)
LINEAR_CASES = [(2049, 128, 1152), (3200, 128, 1152), (2080, 128, 128),
                # the weight gradient pads the rows above with zeros to a multiple of 32 * 16: their last planes hold nothing but
                # padding.  3 584 rows need none: sixteen live planes of 7 steps
                (3584, 128, 128)]


def products():
    """Every product a GPU case takes a bar from, as (name, thunk of its ``product``): tests/test_gemm_ref.py checks the bar on each."""
    out = {}
    for m, n, k in STREAM_SHAPES + [(m, 128, 96) for m in EDGE_ROWS] + SPLIT_SHAPES:
        out[f"{m}x{n}x{k}"] = functools.partial(case, m, n, k)
    for m, n, k, _, bias in SPLITK_CASES:
        out[f"{m}x{n}x{k}" + ("" if bias else "-nobias")] = functools.partial(case, m, n, k, False, bias)
    for m, n, k in BF16_SHAPES:
        out[f"{m}x{n}x{k}-bf16"] = functools.partial(case, m, n, k, True)
    for rows, out_f, in_f in T_CASES:
        out[f"{rows}x{in_f}x{out_f}-nobias"] = functools.partial(case, rows, in_f, out_f, False, False)
        if rows % 32 == 0:
            out[f"{out_f}x{in_f}x{rows}-nobias"] = functools.partial(case, out_f, in_f, rows, False, False)
    for c in LINEAR_CASES:
        for which in ("y", "dx", "dw"):
            out["linear-%dx%dx%d-%s" % (*c, which)] = lambda c=c, which=which: getattr(linear_case(*c), which)
    return sorted(out.items())
