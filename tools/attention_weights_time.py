"""Time of ``mel_gat_attention_weights`` next to ``mel_gat_forward`` on the same inputs (the coefficient export walks a row's
sources twice, the forward once).

    python tools/attention_weights_time.py [--bs 32] [--nodes 50] [--heads 4] [--channels 128] [--steps 200] [--warmup 50]

Random projections and a radius graph at the env's density; HIP events around ``--steps`` back-to-back launches after
``--warmup`` launches, both conv kinds.  Prints one JSON line per (kind, entry point): us per launch.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from melissa_amd import _lib
from melissa_amd.networks.autograd_ops import radius_graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=32)
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--heads", type=int, default=4)
    ap.add_argument("--channels", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    a = ap.parse_args()
    lib = _lib.load()
    bs, n, heads, channels = a.bs, a.nodes, a.heads, a.channels
    rows, hc = bs * n, heads * channels
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    obs = torch.zeros(bs, 8 * n + 1, device="cuda")
    obs[:, :-1].view(bs, n, 8)[:, :, :2] = torch.rand(bs, n, 2, device="cuda", generator=g)
    adj = radius_graph(obs, n, 5)
    xl, xv, xr, att, bias = rnd(rows, hc), rnd(rows, hc), rnd(rows, hc), rnd(hc) * 0.3, rnd(hc) * 0.1
    out = torch.empty(rows, hc, device="cuda")
    alpha = torch.empty(rows, n, heads, device="cuda")
    stream = _lib.current_stream_ptr()
    sources = float(torch.tensor([bin(int(w) & (2 ** 64 - 1)).count("1") for w in adj.reshape(-1).tolist()]).sum()) / rows
    for kind, name in ((_lib.CONV_GATV2, "gatv2"), (_lib.CONV_TRANSFORMER, "transformer")):
        gat = kind == _lib.CONV_GATV2
        p_att, p_bias, p_xv = (att.data_ptr(), bias.data_ptr(), None) if gat else (None, None, xv.data_ptr())
        calls = {
            "mel_gat_forward": lambda: lib.mel_gat_forward(xl.data_ptr(), p_xv, xr.data_ptr(), p_att, p_bias, adj.data_ptr(), bs, n,
                                                           heads, channels, kind, out.data_ptr(), stream),
            "mel_gat_attention_weights": lambda: lib.mel_gat_attention_weights(xl.data_ptr(), xr.data_ptr(), p_att, adj.data_ptr(),
                                                                               bs, n, heads, channels, kind, alpha.data_ptr(),
                                                                               stream),
        }
        for entry, call in calls.items():
            for _ in range(a.warmup):
                _lib.check(call(), entry)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                call()
            t1.record()
            torch.cuda.synchronize()
            print(json.dumps(dict(kind=name, entry=entry, bs=bs, nodes=n, heads=heads, channels=channels, rows=rows,
                                  mean_neighbours=round(sources, 2), steps=a.steps, warmup=a.warmup,
                                  us_per_launch=round(t0.elapsed_time(t1) * 1e3 / a.steps, 3))))


if __name__ == "__main__":
    main()
