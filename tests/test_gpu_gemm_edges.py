"""GPU tests of the GEMM kernels where tests/test_gpu_gemm_tiles.py and the split / bf16 / learn-path tests do not reach:

  A  K streams that end on an odd stage: mel_gemm_f32 on the ring and the persistent kernel (the per-tile kernel as a control) at
     3, 5, 9 and 36 K steps per tile, one tile per workgroup and more than two;
  B  mel_gemm_f32_splitk at chunks of 3, 5, 7 and 2 steps, up to sixteen planes, more work items than ring workgroups;
  C  hip_linear forward and backward at batch sizes whose weight gradient runs such chunks;
  D  padded strides: lda > K with NaN in A's padding columns and in the rows around A, ldy > N with every element outside
     Y[:M, :N] compared bit for bit against a sentinel - for every entry point and tile code.

Operands, references and bars come from tests/gemm_ref.py: rows of 25 magnitudes in every tile, the statistic
max |got - want| / S with S = |a| |w|^T + |b|, held to twice the statistic of a plain fp32 evaluation in k order (the split
kernels get the three dropped partial products on top, bf16 output one rounding).  Beside it every case keeps the project's
global bar of its kernel.  The bf16 tests' ``atol + rtol |want|`` was written for outputs of unit scale: here its atol is
taken relative to max(1, max |want|), as the fp32 kernels' global bar is.  Every output and parts buffer is a ``guarded`` one.
Run with -s for the figures: one line per case, the kernel's statistic beside its bar, in units of 2^-24.
"""
import functools

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

TILE_AUTO, TILE_64, TILE_128, TILE_WIDE, TILE_64_PERSISTENT, TILE_64_RING = 0, 1, 2, 3, 11, 31     # include/melissa_hip.h
F32, BF16 = torch.float32, torch.bfloat16


def library():
    from melissa_amd import _lib
    return _lib, _lib.load(), _lib.current_stream_ptr()


@functools.lru_cache(maxsize=None)
def on_device(m, n, k, bf16=False, bias=True):
    """A case of gemm_ref with contiguous device copies of its operands (bf16 cases: a and w as bf16), shared and never modified."""
    p = gr.case(m, n, k, bf16, bias)
    dt = BF16 if bf16 else F32
    return p, p.a.to("cuda", dt), p.w.to("cuda", dt), None if p.b is None else p.b.cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def padded_input(x, pad, dtype=F32):
    """x [m, k] inside a guarded buffer with ld = k + pad: NaN in the padding columns and in two rows before and after."""
    m, k = x.shape
    buf, p, _ = gr.guarded(m, k, k + pad, dtype, fill=x, device="cuda")
    return buf, p, k + pad


def verify(name, got, p, relu=0, split=False, global_bar=None, bf16_out=False):
    """got [m, n] (any device) against product p: no NaN, the statistic under its bar, the global bar as well."""
    want = torch.relu(p.want) if relu else p.want
    got = got.detach().float().cpu()
    missing = int(torch.isnan(got).sum())
    assert missing == 0, f"{name}: {missing} elements are NaN (never written, or computed from padding)"
    bar = gr.bar(p.seq, p.k, split)
    err = (got.double() - want).abs()
    top = max(1.0, float(want.abs().max()))
    if bf16_out:        # one rounding to nearest on top: the statistic of what is left of the error
        s = float(((err - gr.BF16_ROUND * want.abs()).clamp(min=0) / p.S).max())
    else:
        s = gr.stat(got, want, p.S)
    print(f"GEMM-EDGE {name} | {p.m}x{p.n}x{p.k} relu {relu} | stat {s / gr.U:.2f} | bar {bar / gr.U:.2f} | seq32 {p.seq / gr.U:.2f} | "
          f"max error {float(err.max()):.1e} of {top:.1e}")
    assert s <= bar, f"{name}: statistic {s / gr.U:.2f} x 2^-24 over its bar {bar / gr.U:.2f} x 2^-24"
    if global_bar is None:
        global_bar = 4e-6 * top
    assert bool((err <= global_bar).all()), f"{name}: max error {float(err.max()):.2e} over the project's bar"


def torch_bar(p, a, w, b, relu=0):
    """The bar of tests/test_gpu_gemm_tiles.py: the larger of 4e-6 x max(1, max |want|) and twice torch's own fp32 addmm error."""
    want = torch.relu(p.want) if relu else p.want
    native = a @ w.t() if b is None else torch.addmm(b, a, w.t())
    native = (torch.relu(native) if relu else native).cpu().double()
    return max(4e-6 * max(1.0, float(want.abs().max())), 2 * float((native - want).abs().max()))


# ---- A: stream phase --------------------------------------------------------------------------------------------------------------
# K / 32 = 3, 5, 9, 36 steps per tile.  (577, 384): 60 items, one tile per workgroup, one live row in the last row tile.
# (11009, 384): 173 x 6 = 1 038 items for the ring kernel's 512 workgroups and the persistent kernel's 1 024 - every ring
# workgroup walks at least two tiles and, with an odd step count, enters the second at a ring position that is no multiple of four.
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("m,n,k", gr.STREAM_SHAPES)
@pytest.mark.parametrize("tile", [TILE_64_RING, TILE_64_PERSISTENT, TILE_64])
def test_gemm_f32_stream_phase(tile, m, n, k, relu):
    _lib, lib, stream = library()
    p, a, w, b = on_device(m, n, k)
    ybuf, y, check = gr.guarded(m, n, n, device="cuda")
    _lib.check(lib.mel_gemm_f32(a.data_ptr(), k, w.data_ptr(), b.data_ptr(), y, n, m, n, k, relu, tile, stream), "mel_gemm_f32")
    check(f"tile {tile}")
    verify(f"A f32 tile {tile}", gr.interior(ybuf, m, n), p, relu, global_bar=torch_bar(p, a, w, b, relu))


# ---- B: split-K -------------------------------------------------------------------------------------------------------------------
def run_splitk(name, p, a_ptr, lda, w, b, m, n, k, ksplit, relu, ldy, global_bar):
    """mel_gemm_f32_splitk into guarded Y and parts; Y must be the planes summed in chunk order (+ bias, ReLU), bit for bit."""
    _lib, lib, stream = library()
    ybuf, y, check_y = gr.guarded(m, n, ldy, device="cuda")
    pbuf, parts, check_parts = gr.guarded(ksplit * m, n, n, device="cuda")           # exactly ksplit * m * n floats
    _lib.check(lib.mel_gemm_f32_splitk(a_ptr, lda, w.data_ptr(), ptr(b), y, ldy, m, n, k, relu, ksplit, parts, ksplit * m * n,
                                       stream), "mel_gemm_f32_splitk")
    check_y(name), check_parts(name + " parts")
    planes = gr.interior(pbuf, ksplit * m, n).reshape(ksplit, m, n)
    assert not bool(torch.isnan(planes).any()), f"{name}: {int(torch.isnan(planes).sum())} plane elements were never written"
    total = planes[0].clone()
    for s in range(1, ksplit):
        total += planes[s]
    if b is not None:
        total += b
    got = gr.interior(ybuf, m, n)
    assert torch.equal(got, torch.relu(total) if relu else total), f"{name}: Y is not the planes summed in chunk order"
    verify(name, got, p, relu, global_bar=global_bar)


@pytest.mark.parametrize("m,n,k,ksplit,bias,relu", [c + (r,) for c in gr.SPLITK_CASES for r in ((0, 1) if c[4] else (0,))])
def test_gemm_f32_splitk_chunks(m, n, k, ksplit, bias, relu):
    p, a, w, b = on_device(m, n, k, False, bias)
    run_splitk(f"B split-K {ksplit} x {k // 32 // ksplit} steps", p, a.data_ptr(), k, w, b, m, n, k, ksplit, relu, n,
               torch_bar(p, a, w, b, relu))


# ---- C: the learn path ------------------------------------------------------------------------------------------------------------
# 128 x 1152 weight at 2 049 / 3 200 rows: dW through _weight_grad with ksplit 16 over rows zero-padded to 2 560 / 3 584 - chunks of
# 5 / 7 steps, 576 work items; 128 x 128 at 2 080 rows: chunks of 5 steps; at 3 584 rows: no padding, all sixteen planes live
@pytest.mark.parametrize("rows,out_f,in_f", gr.LINEAR_CASES)
def test_hip_linear_against_float64(rows, out_f, in_f):
    from melissa_amd.networks.autograd_ops import hip_linear
    c = gr.linear_case(rows, out_f, in_f)
    x, w, b = (t.cuda().requires_grad_(True) for t in (c.x, c.w, c.b))
    y = hip_linear(x, w, b)
    y.backward(c.dy.cuda())
    verify(f"C linear {rows} rows y", y, c.y, global_bar=2e-5 * max(1.0, float(c.y.want.abs().max())))
    for name, got, q in (("dX", x.grad, c.dx), ("dW", w.grad, c.dw)):
        verify(f"C linear {rows} rows {name}", got, q, global_bar=1e-5 * float(q.want.abs().max()) + 1e-7)
    db_err = float((b.grad.cpu().double() - c.db).abs().max())
    print(f"GEMM-EDGE C linear {rows} rows db | max error {db_err:.1e} of {float(c.db.abs().max()):.1e}")
    assert db_err <= 1e-5 * float(c.db.abs().max()) + 1e-7


# ---- D: strides and guards (relu 0 throughout: a NaN taken from the padding must reach the output) --------------------------------
@pytest.mark.parametrize("tile,ypad", [(t, 4) for t in (TILE_AUTO, TILE_64, TILE_128, TILE_64_PERSISTENT, TILE_64_RING)] +
                         [(t, 1) for t in (TILE_AUTO, TILE_64, TILE_128, TILE_64_PERSISTENT)])     # these store element by element
def test_gemm_f32_padded_strides(tile, ypad):
    _lib, lib, stream = library()
    m, n, k = 577, 384, 96
    p, a, w, b = on_device(m, n, k)
    abuf, a_ptr, lda = padded_input(a, 12)
    ybuf, y, check = gr.guarded(m, n, n + ypad, device="cuda")
    _lib.check(lib.mel_gemm_f32(a_ptr, lda, w.data_ptr(), b.data_ptr(), y, n + ypad, m, n, k, 0, tile, stream), "mel_gemm_f32")
    check(f"tile {tile} ldy N + {ypad}")
    verify(f"D f32 tile {tile} lda K+12 ldy N+{ypad}", gr.interior(ybuf, m, n), p, global_bar=torch_bar(p, a, w, b))


@pytest.mark.parametrize("m", gr.EDGE_ROWS)
@pytest.mark.parametrize("tile", [TILE_64, TILE_128])
def test_gemm_f32_last_row_against_the_guard_rows(tile, m):
    _lib, lib, stream = library()
    n, k = 128, 96
    p, a, w, b = on_device(m, n, k)
    abuf, a_ptr, lda = padded_input(a, 12)
    ybuf, y, check = gr.guarded(m, n, n + 4, device="cuda")
    _lib.check(lib.mel_gemm_f32(a_ptr, lda, w.data_ptr(), b.data_ptr(), y, n + 4, m, n, k, 0, tile, stream), "mel_gemm_f32")
    check(f"tile {tile} M {m}")
    verify(f"D f32 tile {tile} M edge", gr.interior(ybuf, m, n), p, global_bar=torch_bar(p, a, w, b))


def test_gemm_f32_splitk_padded_strides():
    m, n, k, ksplit = 577, 128, 480, 3
    p, a, w, b = on_device(m, n, k)
    abuf, a_ptr, lda = padded_input(a, 12)
    run_splitk("D split-K 3 lda K+12 ldy N+4", p, a_ptr, lda, w, b, m, n, k, ksplit, 0, n + 4, torch_bar(p, a, w, b))


@pytest.mark.parametrize("rows,out_f,in_f", gr.T_CASES)
def test_gemm_f32_t_padded_strides(rows, out_f, in_f):
    """Both forms of mel_gemm_f32_t with lda, ldw and ldy padded by 4, against float64 and bit-equal to the 64 x 64 kernel on
    transposed copies.  dW = dY^T X contracts over the rows: the entry point takes it for rows % 32 == 0 only and must refuse
    the other case without a launch."""
    _lib, lib, stream = library()
    # dX [rows, in] = dY [rows, out] . W [out, in]: the product (rows, in, out) with W' = W^T
    p, dy, wt, _ = on_device(rows, in_f, out_f, False, False)
    w = wt.t().contiguous()                                                         # [out, in]
    dybuf, dy_ptr, ldd = padded_input(dy, 4)
    wbuf, w_ptr, ldw = padded_input(w, 4)
    ybuf, y, check = gr.guarded(rows, in_f, in_f + 4, device="cuda")
    _lib.check(lib.mel_gemm_f32_t(dy_ptr, ldd, 0, w_ptr, ldw, 1, y, in_f + 4, rows, in_f, out_f, stream), "mel_gemm_f32_t")
    check("dX")
    same = torch.full((rows, in_f), float("nan"), device="cuda")
    _lib.check(lib.mel_gemm_f32(dy.data_ptr(), out_f, wt.data_ptr(), None, same.data_ptr(), in_f, rows, in_f, out_f, 0, TILE_64,
                                stream), "mel_gemm_f32")
    assert torch.equal(gr.interior(ybuf, rows, in_f), same)
    verify("D f32_t dX strides + 4", gr.interior(ybuf, rows, in_f), p)
    # dW [out, in] = dY^T . X [rows, in]: the product (out, in, rows) with A' = dY^T, W' = X^T
    xbuf, x_ptr, ldx = padded_input(torch.zeros(rows, in_f, device="cuda"), 4)
    ybuf, y, check = gr.guarded(out_f, in_f, in_f + 4, device="cuda")
    if rows % 32:
        st = lib.mel_gemm_f32_t(dy_ptr, ldd, 1, x_ptr, ldx, 1, y, in_f + 4, out_f, in_f, rows, stream)
        assert st == _lib.ERR_UNSUPPORTED
        assert bool(torch.isnan(ybuf).all())
        check("dW refused")
        return
    p, dyt, xt, _ = on_device(out_f, in_f, rows, False, False)
    dybuf, dy_ptr, ldd = padded_input(dyt.t().contiguous(), 4)                      # dY [rows, out]
    xbuf, x_ptr, ldx = padded_input(xt.t().contiguous(), 4)                         # X [rows, in]
    _lib.check(lib.mel_gemm_f32_t(dy_ptr, ldd, 1, x_ptr, ldx, 1, y, in_f + 4, out_f, in_f, rows, stream), "mel_gemm_f32_t")
    check("dW")
    same = torch.full((out_f, in_f), float("nan"), device="cuda")
    _lib.check(lib.mel_gemm_f32(dyt.data_ptr(), rows, xt.data_ptr(), None, same.data_ptr(), in_f, out_f, in_f, rows, 0, TILE_64,
                                stream), "mel_gemm_f32")
    assert torch.equal(gr.interior(ybuf, out_f, in_f), same)
    verify("D f32_t dW strides + 4", gr.interior(ybuf, out_f, in_f), p)


def split_scratch(m, n, k, tile, ksplit):
    """Scratch of exactly the bytes mel_gemm_f32_split asks for, between two 256-byte guards."""
    need = ((6 * n * k + 255) & ~255) + (4 * ksplit * m * n if ksplit > 1 else 0) + (6 * k * m if tile == TILE_WIDE else 0)
    buf = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device="cuda")

    def check(what):
        assert bool((buf[:256] == 0xA5).all()) and bool((buf[256 + need:] == 0xA5).all()), f"{what}: scratch guard bytes were written"

    return buf, buf.data_ptr() + 256, need, check


def run_split(name, m, n, k, tile, ksplit, apad, ypad):
    _lib, lib, stream = library()
    p, a, w, b = on_device(m, n, k)
    abuf, a_ptr, lda = padded_input(a, apad) if apad else (a, a.data_ptr(), k)
    ybuf, y, check = gr.guarded(m, n, n + ypad, device="cuda")
    sbuf, scratch, need, check_scratch = split_scratch(m, n, k, tile, ksplit)
    _lib.check(lib.mel_gemm_f32_split(a_ptr, lda, w.data_ptr(), b.data_ptr(), y, n + ypad, m, n, k, 0, tile, ksplit, scratch, need,
                                      stream), "mel_gemm_f32_split")
    check(name), check_scratch(name)
    verify(name, gr.interior(ybuf, m, n), p, split=True)
    return gr.interior(ybuf, m, n)


@pytest.mark.parametrize("tile,ksplit", [(TILE_64, 0), (TILE_128, 0), (TILE_128, 2)])
def test_gemm_f32_split_padded_strides(tile, ksplit):
    run_split(f"D split tile {tile} ksplit {ksplit} lda K+12 ldy N+4", 333, 384, 256, tile, ksplit, 12, 4)


def test_gemm_f32_split_planes_padded_ldy():
    """The 128 x 256 planes kernel requires lda == K: only ldy is padded.  It adds the products of the 128 x 128 kernel in the
    same order: bit-identical."""
    wide = run_split("D split tile 3 ldy N+4", 129, 256, 128, TILE_WIDE, 0, 0, 4)
    big = run_split("D split tile 2 ldy N+4", 129, 256, 128, TILE_128, 0, 0, 4)
    assert torch.equal(wide, big)


@pytest.mark.parametrize("y_f32", [0, 1])
@pytest.mark.parametrize("tile,m,n,k", [(TILE_AUTO,) + gr.BF16_SHAPES[0], (TILE_128,) + gr.BF16_SHAPES[1], (TILE_WIDE,) + gr.BF16_SHAPES[1]])
def test_gemm_bf16_padded_strides(tile, m, n, k, y_f32):
    _lib, lib, stream = library()
    p, a, w, b = on_device(m, n, k, True)
    abuf, a_ptr, lda = padded_input(a, 8, BF16)
    ybuf, y, check = gr.guarded(m, n, n + 8, F32 if y_f32 else BF16, device="cuda")
    _lib.check(lib.mel_gemm_bf16(a_ptr, lda, w.data_ptr(), b.data_ptr(), y, n + 8, m, n, k, 0, y_f32, tile, stream), "mel_gemm_bf16")
    check(f"bf16 tile {tile}")
    top = max(1.0, float(p.want.abs().max()))       # tests/test_gpu_bf16.py's atol + rtol |want|, the atol relative to the output's scale
    old = (1e-4 * top + 1e-4 * p.want.abs()) if y_f32 else (1e-3 * top + 2.0 ** -7 * p.want.abs())
    verify(f"D bf16 tile {tile} y_f32 {y_f32} lda K+8 ldy N+8", gr.interior(ybuf, m, n), p, global_bar=old, bf16_out=not y_f32)
    if not y_f32:       # "one rounding": the bf16 result is the fp32 result of the same launch shape, rounded to nearest even
        fbuf, f, _ = gr.guarded(m, n, n + 8, F32, device="cuda")
        _lib.check(lib.mel_gemm_bf16(a_ptr, lda, w.data_ptr(), b.data_ptr(), f, n + 8, m, n, k, 0, 1, tile, stream), "mel_gemm_bf16")
        assert torch.equal(gr.interior(ybuf, m, n), gr.interior(fbuf, m, n).bfloat16())


# ---- the lda contract: 16-byte loads of A from A + row * lda + 4 c -----------------------------------------------------------------
def test_lda_must_be_a_multiple_of_four():
    """Every exact-fp32 and split kernel fetches A in 16-byte pieces (the ring kernel by LDS-DMA): an lda that is no multiple of 4
    is refused with MEL_ERR_UNSUPPORTED before anything is launched (Y keeps its sentinel), as mel_gemm_f32_t does."""
    _lib, lib, stream = library()
    m, n, k = 64, 128, 128
    a = torch.zeros(m + 1, k + 4, device="cuda")
    w = torch.zeros(n, k, device="cuda")
    scratch = torch.empty(((6 * n * k + 255) & ~255) + 4 * 2 * m * n, dtype=torch.uint8, device="cuda")
    parts = torch.empty(2 * m * n, device="cuda")
    ybuf, y, check = gr.guarded(m, n, n, device="cuda")
    calls = []
    for lda in (k + 1, k + 2, k + 3):
        for tile in (TILE_AUTO, TILE_64, TILE_128, TILE_64_PERSISTENT, TILE_64_RING):
            calls.append(lib.mel_gemm_f32(a.data_ptr(), lda, w.data_ptr(), None, y, n, m, n, k, 0, tile, stream))
        calls.append(lib.mel_gemm_f32_splitk(a.data_ptr(), lda, w.data_ptr(), None, y, n, m, n, k, 0, 2, parts.data_ptr(), parts.numel(),
                                             stream))
        for tile, ksplit in ((TILE_AUTO, 0), (TILE_64, 0), (TILE_128, 0), (TILE_128, 2)):
            calls.append(lib.mel_gemm_f32_split(a.data_ptr(), lda, w.data_ptr(), None, y, n, m, n, k, 0, tile, ksplit, scratch.data_ptr(),
                                                scratch.numel(), stream))
        calls.append(lib.mel_gemm_f32_t(a.data_ptr(), lda, 0, w.data_ptr(), k, 1, y, n, m, k, n, stream))
    assert calls and all(st == _lib.ERR_UNSUPPORTED for st in calls), calls
    torch.cuda.synchronize()
    assert bool(torch.isnan(ybuf).all())
    check("refused calls")
