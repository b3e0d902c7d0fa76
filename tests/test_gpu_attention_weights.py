"""GPU tests of the exported attention coefficients: ``mel_gat_attention_weights`` on the cases of tests/learn_ref.py (n = 1,
isolated targets, rows cut by the 33-hit cap, two adjacency words, 127 sources, edges across the word boundary, 2 to 16 channels
per lane, the 48-lane six-head forms, 1 200 rows) against the float64 reference of tests/test_attention_weights.py, against
``mel_gat_forward`` - relu(alpha . values + bias) rebuilt in float64 from the kernel's coefficients is the forward's output - and
on guarded caller buffers; ``GraphQNetwork.attention_weights`` on the hip backend against the torch backend; ``watch
--attention-out``.

The bar is tests/learn_ref.py:bar - 4e-6 x max(1, max |want|), or twice what the plain fp32 evaluation of the same formula loses.
Each case prints its errors beside it (run with -s)."""
import functools

import numpy as np
import pytest
import torch

from tests import learn_ref as lr
from tests.test_attention_weights import MODELS, alpha_ref, check_structure, conv_operands, make_net, random_obs, scatter_back, sources

pytestmark = pytest.mark.gpu

GUARD = 64          # floats of sentinel / poison before and behind every buffer
SENTINEL = -12345.5
NAN = float("nan")


class Guarded:
    """A device buffer of ``count`` floats with GUARD floats in front of and behind it (tests/test_gpu_head_shapes.py)."""

    def __init__(self, count, fill):
        self.whole = torch.full((count + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.t = self.whole[GUARD:GUARD + count]
        if torch.is_tensor(fill):
            self.t.copy_(fill.reshape(-1))
        else:
            self.t.fill_(fill)

    def ptr(self):
        return self.t.data_ptr()

    def guards(self, value):
        self.whole[:GUARD] = value
        self.whole[-GUARD:] = value

    def intact(self):
        return bool((torch.cat([self.whole[:GUARD], self.whole[-GUARD:]]) == SENTINEL).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


@functools.lru_cache(maxsize=None)
def run_case(case):
    """One case through the kernel, twice - zeros, then NaN in the 64 floats beside every input buffer - into a NaN-filled
    ``alpha`` between sentinels, and once through ``mel_gat_forward``; everything on the host, computed once."""
    from melissa_amd import _lib
    lib = _lib.load()
    spec, heads, channels, kind = case
    adj_bool = lr.graph(spec)
    bs, n, _ = adj_bool.shape
    rows, hc = bs * n, heads * channels
    t = lr.inputs(spec, heads, channels)
    gat = kind == lr.GATV2
    xl, xr = Guarded(rows * hc, t["xl"]), Guarded(rows * hc, t["xr"])
    att = Guarded(hc, t["att"]) if gat else None
    adj = lr.pack(adj_bool).cuda()
    stream = _lib.current_stream_ptr()
    got = {}
    for name, poison in (("clean", 0.0), ("poisoned", NAN)):
        for b in (xl, xr, att):
            if b is not None:
                b.guards(poison)
        alpha = Guarded(rows * n * heads, NAN)
        _lib.check(lib.mel_gat_attention_weights(xl.ptr(), xr.ptr(), att.ptr() if gat else None, adj.data_ptr(), bs, n, heads,
                                                 channels, kind, alpha.ptr(), stream), "mel_gat_attention_weights")
        torch.cuda.synchronize()
        got[name] = alpha.t.cpu().view(bs, n, n, heads)
        got[name + "_intact"] = alpha.intact()
    xv = None if gat else t["xv"].cuda()
    bias = t["bias"].cuda()
    out = torch.full((rows, hc), NAN, device="cuda")
    _lib.check(lib.mel_gat_forward(xl.ptr(), _ptr(xv), xr.ptr(), att.ptr() if gat else None, bias.data_ptr(), adj.data_ptr(), bs, n,
                                   heads, channels, kind, out.data_ptr(), stream), "mel_gat_forward")
    got["out"] = out.cpu()
    return got


@functools.lru_cache(maxsize=None)
def reference(case):
    """(alpha in float64, what the same formula loses in fp32) on the case's inputs."""
    spec, heads, channels, kind = case
    t = lr.inputs(spec, heads, channels)
    want = alpha_ref(kind, t["xl"], t["xr"], t["att"], lr.graph(spec), heads, torch.float64)
    plain = alpha_ref(kind, t["xl"], t["xr"], t["att"], lr.graph(spec), heads, torch.float32)
    return want, float((plain.double() - want).abs().max())


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_kernel_matches_float64(case):
    spec, heads, channels, kind = case
    got = run_case(case)["clean"]
    want, err32 = reference(case)
    assert not torch.isnan(got).any(), f"{int(torch.isnan(got).sum())} elements were never written"
    err = float((got.double() - want).abs().max())
    limit = lr.bar(want, err32)
    print(f"{lr.case_id(case)} alpha: max error {err:.1e} (reference in fp32: {err32:.1e}, bar {limit:.1e})")
    assert err <= limit
    check_structure(got, kind, lr.graph(spec), lr.case_id(case))


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_coefficients_rebuild_the_forward(case):
    """relu(einsum(alpha, values) + bias) in float64 from the KERNEL's coefficients is mel_gat_forward's out: the export
    explains the forward it was taken from."""
    spec, heads, channels, kind = case
    r = run_case(case)
    t = lr.inputs(spec, heads, channels)
    bs, n = lr.graph(spec).shape[:2]
    values = (t["xl"] if kind == lr.GATV2 else t["xv"]).double().view(bs, n, heads, channels)
    want = torch.relu(torch.einsum("bijh,bjhc->bihc", r["clean"].double(), values).reshape(bs * n, -1) + t["bias"].double())
    ref64, ref32 = lr.case_ref(case, torch.float64), lr.case_ref(case, torch.float32)
    err32 = float((ref32["out"].double() - ref64["out"]).abs().max())
    err = float((r["out"].double() - want).abs().max())
    limit = lr.bar(want, err32)
    print(f"{lr.case_id(case)} out from alpha: max error {err:.1e} (reference in fp32: {err32:.1e}, bar {limit:.1e})")
    assert err <= limit


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_kernel_stays_inside_its_rows(case):
    """alpha starts as NaN between sentinels: no NaN is left, what is not a source is the bit pattern of +0.0, the sentinels hold
    their value, and NaN beside every input buffer changes no bit."""
    spec, heads, channels, kind = case
    r = run_case(case)
    assert r["clean_intact"] and r["poisoned_intact"]
    assert not torch.isnan(r["clean"]).any() and not torch.isnan(r["poisoned"]).any()
    assert torch.equal(r["clean"].view(torch.int32), r["poisoned"].view(torch.int32))
    src = sources(kind, lr.graph(spec))
    assert not r["clean"].view(torch.int32)[~src].any()                       # +0.0, not -0.0
    if src.any():
        assert float(r["clean"].max()) > 0


def test_size_guard_names_the_product():
    from melissa_amd import _lib
    lib = _lib.load()
    x = torch.zeros(128 * 512, device="cuda")
    adj = torch.zeros(256, dtype=torch.int64, device="cuda")
    bs, n, heads, channels = 1 << 16, 128, 4, 128                             # bs * n = 2^23 rows pass check_gat; 2^32 elements
    for kind, att in ((lr.GATV2, x.data_ptr()), (lr.TRANSFORMER, None)):
        st = lib.mel_gat_attention_weights(x.data_ptr(), x.data_ptr(), att, adj.data_ptr(), bs, n, heads, channels, kind,
                                           x.data_ptr(), _lib.current_stream_ptr())
        assert st == _lib.ERR_INVALID_ARG
        msg = _lib.last_error()
        assert "bs * n * n * heads" in msg and str(bs * n * n * heads) in msg, msg
    st = lib.mel_gat_attention_weights(x.data_ptr(), x.data_ptr(), x.data_ptr(), adj.data_ptr(), 1, 2, 4, 128, lr.GATV2, None,
                                       _lib.current_stream_ptr())
    assert st == _lib.ERR_INVALID_ARG and "alpha" in _lib.last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("n", [20, 70])
@pytest.mark.parametrize("hidden,heads", [(64, 6), (128, 4)])
@pytest.mark.parametrize("model", list(MODELS))
def test_network_on_the_hip_backend_matches_the_torch_backend(model, hidden, heads, n):
    bs = 3
    net = make_net(model, n, hidden, heads, device="cuda", backend="hip")
    obs = torch.from_numpy(random_obs(n, bs, n + heads)).cuda()
    hip = net.attention_weights(obs)
    edges = net.attention_weights(obs, layout="edges")
    net.learn_kernels = "dense"
    dense = net.attention_weights(obs)
    ops, adj = conv_operands(net, obs)
    assert len(hip) == len(dense) == len(edges) == (1 if model == "hl_dgn" else 2)
    for k, (got, want, (kind, xl, xr, att), (edge_index, a)) in enumerate(zip(hip, dense, ops, edges)):
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (bs, n, n, heads) and not got.requires_grad
        f64 = alpha_ref(kind, xl, xr, att, adj, heads, torch.float64)
        err32 = float((alpha_ref(kind, xl, xr, att, adj, heads, torch.float32).double() - f64).abs().max())
        err = float((got - want).abs().max())
        limit = lr.bar(want, err32)
        print(f"{model} {hidden}x{heads} n {n} conv{k + 1}: hip - torch {err:.1e} (formula in fp32: {err32:.1e}, bar {limit:.1e})")
        assert err <= limit
        check_structure(got, kind, adj, f"{model} conv{k + 1}")
        # layout="edges" of the hip backend: the dense form, exactly, in upstream's order
        assert torch.equal(scatter_back(edge_index, a, bs, n), got.cpu())
        assert edge_index.shape[1] == int(adj.sum()) + (bs * n if kind == lr.GATV2 else 0)
        body = edge_index[:, :int(adj.sum())]
        key = body[1] * (bs * n) + body[0]
        assert bool((key[1:] > key[:-1]).all())
        if kind == lr.GATV2:
            assert torch.equal(edge_index[:, int(adj.sum()):], torch.arange(bs * n).repeat(2, 1))


TIMING_KEYS = ("collect_time", "collect_speed")      # wall-clock readings: no two runs share them


@pytest.mark.parametrize("model", ["l_dgn", "hl_dgn"])
def test_watch_attention_out(model, tmp_path, capsys):
    """The flagged run goes through the command line (``watch.main``), the plain one through ``watch.watch``; the result dicts
    are compared key by key but for TIMING_KEYS."""
    import json

    from melissa_amd import watch
    from melissa_amd.train import build_network
    n, envs, rounds, seed = 20, 2, 3, 9                                       # seed: watch's default
    path = str(tmp_path / "alpha.npz")
    plain = json.loads(json.dumps(watch.watch(model=model, n_nodes=n, envs=envs, episodes=2)))
    capsys.readouterr()
    watch.main(["--model", model, "--nodes", str(n), "--envs", str(envs), "--episodes", "2", "--attention-out", path,
                "--attention-rounds", str(rounds)])
    flagged = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert list(plain) == list(flagged)                                       # the evaluation is unaffected
    for k in plain:
        if k not in TIMING_KEYS:
            np.testing.assert_equal(flagged[k], plain[k], err_msg=k)
    rec = np.load(path)
    convs = 1 if model == "hl_dgn" else 2
    assert sorted(rec.files) == sorted(["obs", "acted", "action"] + [f"alpha_conv{k + 1}" for k in range(convs)])
    assert rec["obs"].shape == (rounds, envs, 8 * n) and rec["obs"].dtype == np.float32
    assert rec["acted"].shape == rec["action"].shape == (rounds, envs, n)
    assert rec["acted"].any() and (rec["action"][~rec["acted"]] == -1).all()
    # the network watch() built: same seed, same constructor
    torch.manual_seed(seed)
    net = build_network(model, n, "cuda:0").eval()
    net.set_feature_dtype("f32")
    obs = torch.from_numpy(rec["obs"]).cuda().view(rounds * envs, 8 * n)
    with torch.no_grad():
        alphas = net.attention_weights(torch.cat([obs, obs.new_zeros(len(obs), 1)], dim=1))
        assert len(alphas) == convs
        for k, a in enumerate(alphas):
            stored = rec[f"alpha_conv{k + 1}"]
            assert stored.shape == (rounds, envs, n, n, 4)
            assert np.array_equal(stored.reshape(-1, n, n, 4), a.cpu().numpy())
        r, b, i = np.nonzero(rec["acted"])
        rows = torch.cat([obs[torch.from_numpy(r * envs + b).cuda()], torch.from_numpy(i).cuda().float()[:, None]], dim=1)
        logits = net.hip_forward(rows)
    assert np.array_equal(rec["action"][r, b, i], logits.argmax(dim=1).cpu().numpy())
