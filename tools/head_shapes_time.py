"""Forward time of a 6-head L-DGN on its own kernels against the workaround a user had before them: the same weights
zero-padded to 8 heads (a full wavefront at hc = 1024, a third more projection FLOPs).

    python tools/head_shapes_time.py [--variant native|padded|both] [--nodes 50] [--envs 1024] [--hidden 128] [--steps 200]

The step is ``hip_forward_agents`` on env-like observations (integer features: the forward takes the node-feature table, as the
round loop's does) with about 0.1 N controlling agents per env.  Prints one JSON line per variant (us per forward, from HIP
events around ``--steps`` forwards) after checking that both variants give the same logits.  Under ``rocprofv3 --kernel-trace
--stats`` run one variant per process: the per-launch times of that variant are then the whole trace.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from melissa_amd.networks import LDGNNetwork

DUEL = lambda: ({"hidden_sizes": [128, 128]}, {"hidden_sizes": [128, 128]})


def pad_heads(sd, hidden, heads, to):
    """The state_dict of a ``heads``-head L-DGN as a ``to``-head one that computes the same logits: the extra heads have zero
    projections, zero attention vectors and zero biases (their output channels are relu(0) = 0), and nothing reads them."""
    hc, pc = heads * hidden, to * hidden
    out = {}
    for k, v in sd.items():
        if k.startswith(("conv1.", "conv2.")):
            conv, name = k.split(".", 1)
            if name == "att":
                p = v.new_zeros(1, to, hidden)
                p[:, :heads] = v
            elif name.endswith("weight"):
                cols = v.shape[1] if conv == "conv1" else pc
                p = v.new_zeros(pc, cols)
                p[:hc, :v.shape[1]] = v
            else:
                p = v.new_zeros(pc)
                p[:hc] = v
            out[k] = p
        elif k in ("Q.model.0.weight", "V.model.0.weight"):          # head input: x_1 | x_2 | x_3
            p = v.new_zeros(v.shape[0], hidden + 2 * pc)
            p[:, :hidden] = v[:, :hidden]
            p[:, hidden:hidden + hc] = v[:, hidden:hidden + hc]
            p[:, hidden + pc:hidden + pc + hc] = v[:, hidden + hc:]
            out[k] = p
        else:
            out[k] = v
    return out


def inputs(n, bs, seed=3):
    rng = np.random.RandomState(seed)
    m = np.zeros((bs, n, 8), dtype=np.float32)
    m[:, :, 0:2] = rng.uniform(0, 1, size=(bs, n, 2))
    m[:, :, 2] = rng.randint(0, n, size=(bs, n))
    m[:, :, 3] = rng.randint(0, 5, size=(bs, n))
    m[:, :, 4:7] = rng.randint(0, 2, size=(bs, n, 3))
    m[:, :, 7] = (rng.uniform(size=(bs, n)) > 0.1)
    masks = np.zeros((bs, (n + 63) // 64), dtype=np.uint64)
    for b in range(bs):
        for a in rng.choice(n, size=max(1, n // 10), replace=False):
            masks[b, int(a) // 64] |= np.uint64(1) << np.uint64(int(a) % 64)
    am = masks.view(np.int64)
    return torch.from_numpy(m.reshape(bs, n * 8)).cuda(), torch.from_numpy(am[:, 0].copy() if am.shape[1] == 1 else am).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", default="both", choices=["native", "padded", "both"])
    ap.add_argument("--nodes", type=int, default=50)
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--heads", type=int, default=6)
    ap.add_argument("--pad-to", type=int, default=8)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--dtype", default="f32a")
    a = ap.parse_args()
    n, bs = a.nodes, a.envs
    torch.manual_seed(5)
    native = LDGNNetwork(5, a.hidden, 2, a.heads, n, dueling_param=DUEL(), device="cuda", backend="hip")
    with torch.no_grad():
        for conv in (native.conv1, native.conv2):
            conv.bias.uniform_(-0.1, 0.1)
    padded = LDGNNetwork(5, a.hidden, 2, a.pad_to, n, dueling_param=DUEL(), device="cuda", backend="hip")
    padded.load_state_dict(pad_heads(native.state_dict(), a.hidden, a.heads, a.pad_to))
    obs, masks = inputs(n, bs)
    cap = bs * n
    nets = {"native": native, "padded": padded}
    logits = {}
    for name, net in nets.items():
        net.set_feature_dtype(a.dtype)
        if a.variant in (name, "both"):
            with torch.no_grad():
                out, off = net.hip_forward_agents(obs, masks, cap, integer_features=True)
            logits[name] = out[:int(off[-1])].clone()
    if len(logits) == 2:
        diff = float((logits["native"] - logits["padded"]).abs().max())
        assert diff <= 1e-5, diff
    for name, out in logits.items():
        net = nets[name]
        with torch.no_grad():
            for _ in range(20):
                net.hip_forward_agents(obs, masks, cap, integer_features=True)
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.steps):
                net.hip_forward_agents(obs, masks, cap, integer_features=True)
            t1.record()
            torch.cuda.synchronize()
        heads = a.heads if name == "native" else a.pad_to
        print(json.dumps(dict(variant=name, model="l_dgn", nodes=n, envs=bs, hidden=a.hidden, heads=heads, hc=heads * a.hidden,
                              dtype=a.dtype, rows=int(out.shape[0]), steps=a.steps, us_per_forward=t0.elapsed_time(t1) * 1e3 / a.steps,
                              max_abs_diff_native_vs_padded=(diff if len(logits) == 2 else None))))


if __name__ == "__main__":
    main()
