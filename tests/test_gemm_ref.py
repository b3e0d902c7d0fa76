"""tests/gemm_ref.py checked without a GPU: the bars it computes admit a correct fp32 GEMM (torch's own on the CPU) and stay
under the worst-case rounding bound, they reject two wrong GEMMs - one that loses the low byte of every a, one that drops the
last 32 terms of a single row - on every shape the GPU cases use, and ``guarded`` notices one changed element wherever it is."""
import pytest
import torch

from tests import gemm_ref as gr

PRODUCTS = dict(gr.products())


@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_bar_admits_torch_addmm_and_rejects_wrong_products(name):
    p = PRODUCTS[name]()
    bar = gr.bar(p.seq, p.k)                                            # asserts 0 < bar <= (K + 2) x 2^-24
    assert gr.bar(p.seq, p.k, split=True) <= (p.k + 2) * gr.U
    native = p.a @ p.w.t() if p.b is None else torch.addmm(p.b, p.a, p.w.t())
    got = gr.stat(native, p.want, p.S)
    # a GEMM that clears the low byte of every a (a dropped low plane), otherwise exact; bf16 values have no low byte: there
    # the model clears the last bit of their 8-bit significand
    low = (p.a.view(torch.int32) & ~(0x10000 if "bf16" in name else 0xFF)).view(torch.float32)
    low_stat = gr.stat(gr.reference(low, p.w, p.b)[0], p.want, p.S)
    # a GEMM that leaves the last 32 terms of one row out, otherwise exact
    row = p.m // 2
    short = p.want.clone()
    short[row] = gr.reference(p.a[row:row + 1, :p.k - 32], p.w[:, :p.k - 32], p.b)[0][0]
    short_stat = gr.stat(short, p.want, p.S)
    print(f"{name}: seq32 {p.seq / gr.U:.2f}, bar {bar / gr.U:.2f}, torch addmm {got / gr.U:.2f}, low byte cleared "
          f"{low_stat / gr.U:.1f}, 32 terms dropped {short_stat / gr.U:.3g} (x 2^-24; bound {p.k + 2})")
    assert got <= bar
    assert low_stat > gr.bar(p.seq, p.k, split=True)
    assert short_stat > gr.bar(p.seq, p.k, split=True)
    if "bf16" in name:      # with bf16 output: the same wrong products are outside bar x S + 2^-8 |want| as well
        for wrong in (gr.reference(low, p.w, p.b)[0], short):
            assert bool(((wrong - p.want).abs() > bar * p.S + gr.BF16_ROUND * p.want.abs()).any())


def test_relu_goes_on_want_only():
    a, w, b = gr.operands(5, 64, 32, seed=1)
    want, S = gr.reference(a, w, b)
    want_r, S_r = gr.reference(a, w, b, relu=True)
    assert torch.equal(want_r, torch.relu(want)) and torch.equal(S_r, S) and bool((want < 0).any())
    assert gr.stat(want_r.float(), want_r, S) <= gr.U                   # one rounding to fp32: half a unit in the last place


def test_sampled_rows():
    assert list(gr.sample_rows(1024)) == list(range(1024))
    rows = gr.sample_rows(11009)
    assert set(range(64)) <= set(rows) and set(range(11009 - 65, 11009)) <= set(rows) and 512 <= len(rows) <= 641
    assert list(rows) == list(gr.sample_rows(11009))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("ld", [132, 129])
def test_guarded_reports_one_changed_element(dtype, ld):
    m, n = 7, 128
    places = {"padding column": (2 + 3, n), "guard row before": (1, 5), "guard row after": (m + 2, 0), "first outside": (0, 0),
              "last outside": (m + 3, ld - 1), "last padding column of the last row": (m + 1, ld - 1)}
    for what, (r, c) in places.items():
        buf, ptr, check = gr.guarded(m, n, ld, dtype)
        assert ptr == buf.data_ptr() + 2 * ld * buf.element_size()
        gr.interior(buf, m, n).fill_(1.0)
        check(what)                                                     # writing the view itself is no finding
        buf[r, c] = 0.0
        with pytest.raises(AssertionError, match="1 elements outside"):
            check(what)
    # another NaN is not the sentinel: compared bit for bit
    buf, _, check = gr.guarded(m, n, ld, dtype)
    buf[0, 1] = float("nan")
    with pytest.raises(AssertionError, match="1 elements outside"):
        check()


def test_guarded_input_holds_nan_around_the_operand():
    a = gr.operands(5, 1, 32, seed=2)[0]
    buf, ptr, check = gr.guarded(5, 32, 44, fill=a)
    assert torch.equal(gr.interior(buf, 5, 32), a) and int(torch.isnan(buf).sum()) == 9 * 44 - 5 * 32
    check()


@pytest.mark.parametrize("name", sorted(PRODUCTS))
def test_scaled_operands_stay_normal(name):
    p = PRODUCTS[name]()
    tiny, huge = torch.finfo(torch.float32).tiny, torch.finfo(torch.float32).max
    for x in (p.a, p.w) + (() if p.b is None else (p.b,)):
        mag = x.abs()
        assert bool(torch.isfinite(x).all()) and float(mag.max()) < huge
        assert float(mag[mag > 0].min()) >= tiny
    # every product and partial sum of the plain fp32 evaluation stays normal too: |a_ik w_jk| >= tiny where nonzero, S finite
    lo = float(p.a.abs()[p.a != 0].min()) * float(p.w.abs()[p.w != 0].min())
    assert lo >= tiny and float(p.S.max()) < huge
    if "bf16" in name:
        assert torch.equal(p.a.bfloat16().float(), p.a) and torch.equal(p.w.bfloat16().float(), p.w)


def test_scalings_are_exact_and_every_tile_holds_all_of_them():
    a, w, b = gr.operands(64, 64, 32, seed=3)
    g = torch.Generator().manual_seed(3)
    a0, w0, b0 = torch.randn(64, 32, generator=g), torch.randn(64, 32, generator=g) / 32 ** 0.5, torch.randn(64, generator=g)
    ea, ew = (torch.arange(64) % 25) - 12, (torch.arange(64) % 13) - 6
    assert torch.equal(a, torch.ldexp(a0, ea[:, None].expand(64, 32)))
    assert torch.equal(w, torch.ldexp(w0, ew[:, None].expand(64, 32))) and torch.equal(b, torch.ldexp(b0, ew))
    assert sorted(set(ea[:32].tolist())) == list(range(-12, 13)) and sorted(set(ew[:32].tolist())) == list(range(-6, 7))


def test_bf16_rounding_term_is_the_unit_roundoff_of_the_format():
    """One rounding to nearest of v to bf16 moves it by at most 2^-8 |v| - and by 2^-8 / (1 + 2^-8) |v| at a tie, so no smaller
    power of two would do."""
    v = torch.tensor([1 + 2.0 ** -8, 1.0, 3.1415926, 1 + 3 * 2.0 ** -8, 255.5, 2.0 ** -20 * (1 + 2.0 ** -8)], dtype=torch.float32)
    rel = ((v.bfloat16().double() - v.double()).abs() / v.double().abs())
    assert float(rel.max()) <= gr.BF16_ROUND and float(rel.max()) > gr.BF16_ROUND / 2
    x = torch.randn(1 << 16, generator=torch.Generator().manual_seed(0))
    assert float(((x.bfloat16().double() - x.double()).abs() / x.double().abs()).max()) <= gr.BF16_ROUND
