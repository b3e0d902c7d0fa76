"""GPU tests of the learn-path kernels of csrc/grad.hip on their own, row by row: ``mel_gat_forward`` / ``mel_gat_backward`` (both
conv kinds), ``mel_pool_forward`` / ``mel_pool_backward`` and ``mel_transpose_f32``, called through ``_lib`` on caller buffers
prefilled with NaN (a sentinel for the transpose) and compared element by element with the float64 references of
tests/learn_ref.py.

The attention cases (learn_ref.GPU_CASES) feed a DENSE grad_out to graphs the end-to-end gradient tests never draw: rows cut by
the 33-hit cap (an asymmetric adjacency: the sources kernel's transposed lookup decides the answer), sources in the second
adjacency word, isolated targets, n = 1, more rows than the targets kernel's grid has waves - at 2, 4, 8 and 16 channels per
lane, 48 live lanes, and heads of 64, 32, 16, 8 and 1 lanes.  tests/test_learn_ref.py checks without a GPU that the graphs have
these properties and that the reference is the project's formulation.

The bar is tests/test_gpu_gemm_tiles.py's: the larger of 4e-6 x max(1, max |want|) and twice the error of the reference's own
fp32 evaluation.  Each case prints the kernel's error beside that fp32 error for every tensor (run with -s).
"""
import pytest
import torch

from tests import learn_ref as lr

pytestmark = pytest.mark.gpu

PARTIAL_GROUPS = 256                          # MEL_GAT_PARTIAL_GROUPS (include/melissa_hip.h)
NAN = float("nan")


def _ptr(t):
    return None if t is None else t.data_ptr()


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_attention_kernels_match_float64(case):
    from melissa_amd import _lib
    lib = _lib.load()
    spec, heads, channels, kind = case
    adj_bool = lr.graph(spec)
    bs, n, _ = adj_bool.shape
    rows, hc = bs * n, heads * channels
    t = {k: v.cuda() for k, v in lr.inputs(spec, heads, channels).items()}
    gat = kind == lr.GATV2
    xv, att = (None, t["att"]) if gat else (t["xv"], None)
    adj = lr.pack(adj_bool).cuda()
    stream = _lib.current_stream_ptr()

    out = _nan(rows, hc)
    _lib.check(lib.mel_gat_forward(t["xl"].data_ptr(), _ptr(xv), t["xr"].data_ptr(), _ptr(att), t["bias"].data_ptr(),
                                   adj.data_ptr(), bs, n, heads, channels, kind, out.data_ptr(), stream), "mel_gat_forward")

    def backward():
        got = {"dxl": _nan(rows, hc), "dxv": None if gat else _nan(rows, hc), "dxr": _nan(rows, hc),
               "datt": _nan(hc) if gat else None, "dbias": _nan(hc)}
        stats = _nan(rows * heads * 4 + PARTIAL_GROUPS * 2 * hc)
        _lib.check(lib.mel_gat_backward(t["xl"].data_ptr(), _ptr(xv), t["xr"].data_ptr(), _ptr(att), adj.data_ptr(),
                                        out.data_ptr(), t["gout"].data_ptr(), bs, n, heads, channels, kind, got["dxl"].data_ptr(),
                                        _ptr(got["dxv"]), got["dxr"].data_ptr(), _ptr(got["datt"]), got["dbias"].data_ptr(),
                                        stats.data_ptr(), stream), "mel_gat_backward")
        return {k: None if v is None else v.cpu() for k, v in got.items()}

    got = backward()
    again = backward()
    got["out"] = out.cpu()
    name_of = lr.case_id(case)
    for name in lr.TENSORS:                                # every element is written
        if got[name] is not None:
            assert not torch.isnan(got[name]).any(), f"{name_of} {name}: {int(torch.isnan(got[name]).sum())} elements were never written"

    # the ReLU mask: where the kernel's differs from float64's, the pre-activation is within the forward's bar of zero (a rounding
    # flip, not a wrong row); the float64 backward then starts from the KERNEL's mask, so nothing is excluded below
    mask = got["out"] > 0
    want = lr.case_ref(case, torch.float64, relu_mask=mask)
    plain = lr.case_ref(case, torch.float32, relu_mask=mask)
    err32 = {k: float((plain[k].double() - want[k]).abs().max()) for k in lr.TENSORS if want[k] is not None}
    flips = mask != (want["pre"] > 0)
    print(f"{name_of}: {int(flips.sum())} ReLU flips of {mask.numel()}")
    assert float(want["pre"][flips].abs().max() if flips.any() else 0.0) <= lr.bar(want["out"], err32["out"])

    for name in lr.TENSORS:
        if want[name] is None:
            assert got[name] is None
            continue
        err = float((got[name].double() - want[name]).abs().max())
        limit = lr.bar(want[name], err32[name])
        print(f"{name_of} {name}: max error {err:.1e} (reference in fp32: {err32[name]:.1e}, bar {limit:.1e}, "
              f"max |want| {float(want[name].abs().max()):.1e})")
        assert err <= limit, name

    for name, second in again.items():                     # fixed-order sums: the same bits again
        assert second is None or torch.equal(second, got[name]), f"{name_of} {name}: a second backward gave other bits"


@pytest.mark.parametrize("agg", [lr.AGG_MAX, lr.AGG_MEAN, lr.AGG_ADD], ids=["max", "mean", "add"])
@pytest.mark.parametrize("shape", lr.POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_kernels_match_float64(shape, agg):
    from melissa_amd import _lib
    lib = _lib.load()
    bs, n, hc = shape
    x, dm, g = lr.pool_inputs(bs, n, hc)
    want, want_arg = lr.pool_ref(x, dm, n, agg, torch.float64)
    plain, _ = lr.pool_ref(x, dm, n, agg, torch.float32)
    xd, dmd, gd = x.cuda(), dm.cuda(), g.cuda()
    pooled = _nan(bs, hc)
    arg = torch.full((bs, hc), -77, dtype=torch.int32, device="cuda") if agg == lr.AGG_MAX else None
    stream = _lib.current_stream_ptr()
    _lib.check(lib.mel_pool_forward(xd.data_ptr(), dmd.data_ptr(), bs, n, hc, agg, pooled.data_ptr(), _ptr(arg), stream),
               "mel_pool_forward")
    got = pooled.cpu()
    assert not torch.isnan(got).any()
    if agg == lr.AGG_MAX:                                  # x * (0 or 1) is exact and so is a maximum: the same bits
        assert torch.equal(got, plain)
        assert torch.equal(arg.cpu().long(), want_arg)     # the FIRST maximum
    else:
        err, err32 = float((got.double() - want).abs().max()), float((plain.double() - want).abs().max())
        print(f"pool {shape} agg {agg}: max error {err:.1e} (reference in fp32: {err32:.1e})")
        assert err <= lr.bar(want, err32)

    dx = _nan(bs * n, hc)
    _lib.check(lib.mel_pool_backward(gd.data_ptr(), dmd.data_ptr(), _ptr(arg), bs, n, hc, agg, dx.data_ptr(), stream),
               "mel_pool_backward")
    got = dx.cpu()
    assert not torch.isnan(got).any()
    want = lr.pool_ref_backward(g, dm, want_arg, n, agg, torch.float64)
    plain = lr.pool_ref_backward(g, dm, want_arg, n, agg, torch.float32)
    err, err32 = float((got.double() - want).abs().max()), float((plain.double() - want).abs().max())
    print(f"pool backward {shape} agg {agg}: max error {err:.1e} (reference in fp32: {err32:.1e})")
    assert err <= lr.bar(want, err32)
    assert not got[dm == 0].any()                          # exactly 0 on the rows dm switches off
    if agg == lr.AGG_MAX:                                  # and off the maximum's node
        off = torch.ones(bs, n, hc, dtype=torch.bool).scatter_(1, want_arg[:, None, :], False)
        assert not got.view(bs, n, hc)[off].any()


SENTINEL = -77.0


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(1, 64, 64, 32), (31, 33, 40, 32), (33, 65, 65, 64), (1000, 128, 128, 1024),
                                                     (64, 32, 32, 64)])
def test_transpose_writes_the_block_and_nothing_else(rows, cols, ld_src, ld_dst):
    from melissa_amd import _lib
    lib = _lib.load()
    src = torch.randn(rows, ld_src, generator=torch.Generator().manual_seed(rows + cols)).cuda()
    dst = torch.full((cols, ld_dst), SENTINEL, device="cuda")
    _lib.check(lib.mel_transpose_f32(src.data_ptr(), ld_src, rows, cols, dst.data_ptr(), ld_dst, _lib.current_stream_ptr()),
               "mel_transpose_f32")
    got = dst.cpu()
    assert torch.equal(got[:, :rows], src.cpu()[:, :cols].t())
    assert (got[:, rows:] == SENTINEL).all()               # the padding columns are left as they were


def test_transpose_of_no_rows_writes_nothing():
    from melissa_amd import _lib
    lib = _lib.load()
    src = torch.randn(1, 64).cuda()
    dst = torch.full((64, 32), SENTINEL, device="cuda")
    assert lib.mel_transpose_f32(src.data_ptr(), 64, 0, 64, dst.data_ptr(), 32, _lib.current_stream_ptr()) == _lib.OK
    assert (dst.cpu() == SENTINEL).all()
