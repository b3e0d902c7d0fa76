"""GPU tests of the exact-fp32 GEMM entry points on their own: mel_gemm_f32 with every tile code (the 64 x 64 and 128 x 128
per-tile kernels, the persistent kernel, the specialised-wavefront ring kernel) and mel_gemm_f32_splitk (the ring kernel's
split-K).  The shapes exercise the work-item walk the kernels share (gemm_walk.hpp): a single item followed by padding ids,
item counts that are no multiple of 8 (both branches of the XCD remap) with one live row in the last row tile, and more items
than a persistent grid has workgroups.

Every case prefills Y with NaN and compares all of it against the float64 product.  The bar is the larger of the project's bar
for fp32-accurate GEMMs (4e-6 x max(1, max |want|), as test_split_gemm_matches_float64) and twice the error of torch's own fp32
addmm on the same operands (twice: the summation orders differ).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

TILE_AUTO, TILE_64, TILE_128, TILE_64_PERSISTENT, TILE_64_RING = 0, 1, 2, 11, 31     # include/melissa_hip.h


@functools.lru_cache(maxsize=None)
def problem(m, n, k):
    """Operands on the device, the float64 product a w^T + b on the CPU and torch's own fp32 addmm of the same operands:
    computed once per shape and shared by every case that uses it (nothing modifies them)."""
    g = torch.Generator().manual_seed(m + n + k)
    a = torch.randn(m, k, generator=g)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    b = torch.randn(n, generator=g)
    want = torch.addmm(b.double(), a.double(), w.double().t())
    a, w, b = a.cuda(), w.cuda(), b.cuda()
    native = torch.addmm(b, a, w.t()).cpu()
    return a, w, b, want, native


def check(name, y, m, n, k, relu):
    a, w, b, want, native = problem(m, n, k)
    if relu:
        want, native = torch.relu(want), torch.relu(native)
    got = y.cpu().double()
    assert not torch.isnan(got).any(), f"{name}: {int(torch.isnan(got).sum())} elements were never written"
    err = float((got - want).abs().max())
    torch_err = float((native.double() - want).abs().max())
    print(f"{name} {m}x{n}x{k} relu {relu}: max error {err:.1e} (torch fp32 addmm: {torch_err:.1e})")
    assert err <= max(4e-6 * max(1.0, float(want.abs().max())), 2 * torch_err)


# K = 64 and N a multiple of 128, so that every tile code is honoured.  (1, 128): one item and seven padding ids; (577, 384):
# 10 x 6 = 60 items of 64 x 64 and 5 x 3 = 15 of 128 x 128, the last row tile with one live row; (38400, 128): 1 200 items of
# 64 x 64 for the persistent kernel's 1 024 workgroups and the ring kernel's 512
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("m,n", [(1, 128), (577, 384), (38400, 128)])
@pytest.mark.parametrize("tile", [TILE_AUTO, TILE_64, TILE_128, TILE_64_PERSISTENT, TILE_64_RING])
def test_gemm_f32_tiles_match_float64(tile, m, n, relu):
    from melissa_amd import _lib
    lib = _lib.load()
    k = 64
    a, w, b, _, _ = problem(m, n, k)
    y = torch.full((m, n), float("nan"), device="cuda")
    _lib.check(lib.mel_gemm_f32(a.data_ptr(), k, w.data_ptr(), b.data_ptr(), y.data_ptr(), n, m, n, k, relu, tile,
                                _lib.current_stream_ptr()), "mel_gemm_f32")
    check(f"gemm f32 tile {tile}", y, m, n, k, relu)


# K = 256 is 8 steps of 32: ksplit 4 gives chunks of 2 steps, the fewest the entry point takes
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("m,ksplit", [(577, 2), (577, 4), (1, 2)])
def test_gemm_f32_splitk_matches_float64(m, ksplit, relu):
    from melissa_amd import _lib
    lib = _lib.load()
    n, k = 128, 256
    a, w, b, _, _ = problem(m, n, k)
    y = torch.full((m, n), float("nan"), device="cuda")
    parts = torch.full((ksplit * m * n,), float("nan"), device="cuda")
    _lib.check(lib.mel_gemm_f32_splitk(a.data_ptr(), k, w.data_ptr(), b.data_ptr(), y.data_ptr(), n, m, n, k, relu, ksplit,
                                       parts.data_ptr(), parts.numel(), _lib.current_stream_ptr()), "mel_gemm_f32_splitk")
    check(f"gemm f32 split-K {ksplit}", y, m, n, k, relu)
