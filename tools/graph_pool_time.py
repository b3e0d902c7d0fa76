"""Wall time of the training-graph pool: ``device_graph_pool`` (csrc/graph_pool.hpp) against the host loop ``packed_graph_pool``
on the same machine (python tools/graph_pool_time.py).

    pair    (20, 64, 0) and (50, 4096, 0): both generators on the same inputs; the arrays must be equal
    device  (20, 50000, 0) and (50, 50000, 0): the device alone; the host figure beside it is EXTRAPOLATED from the host's
            measured time per candidate in the pair run of the same N

A device time is a host clock around ``device_graph_pool``: launches, the count read after every chunk and the copy of the three
arrays back to the host; the library load and one small untimed call come first.  Median of three (pair) or one run (device).
Every measurement is a child process under its own ``timeout``; the tool stops at the first one that does not exit with 0 and,
for a device run that ran out of time, says so next to the rate the pair run of that N reached."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (kind, n, count, time limit in seconds)
RUNS = (("pair", 20, 64, 240), ("pair", 50, 4096, 120), ("device", 20, 50000, 300), ("device", 50, 50000, 120))


def one(kind, n, count):
    import numpy as np
    import torch
    from melissa_amd import _lib
    from melissa_amd.env import device_graph_pool, packed_graph_pool
    _lib.load()
    device_graph_pool(12, 2, radius=0.4)                       # untimed: runtime start-up, first launches
    times, got = [], None
    for _ in range(3 if kind == "pair" else 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = device_graph_pool(n, count)
        times.append(time.perf_counter() - t0)
    out = dict(kind=kind, n=n, count=count, candidates=int(got[2][-1]) + 1, device_s=sorted(times)[len(times) // 2],
               device_runs=times)
    if kind == "pair":
        t0 = time.perf_counter()
        want = packed_graph_pool(n, count)
        out["host_s"] = time.perf_counter() - t0
        out["equal"] = all(np.array_equal(g, w) for g, w in zip(got, want))
    print(json.dumps(out), flush=True)
    return 0 if out.get("equal", True) else 1


def main():
    if "--one" in sys.argv:
        kind, n, count = sys.argv[sys.argv.index("--one") + 1:][:3]
        raise SystemExit(one(kind, int(n), int(count)))
    host_per_candidate, device_rate = {}, {}
    for kind, n, count, limit in RUNS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--one", kind, str(n), str(count)]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if res.returncode != 0:
            print(f"{kind} ({n}, {count}, 0): exit status {res.returncode}" +
                  (f" - not finished within {limit} s; the pair run at N = {n} reached {device_rate[n]:.3g} candidates/s"
                   if res.returncode in (124, 137) and n in device_rate else ""), flush=True)
            sys.stderr.write(res.stderr[-2000:])
            raise SystemExit(res.returncode)
        r = json.loads(res.stdout.strip().splitlines()[-1])
        rate = r["candidates"] / r["device_s"]
        line = (f"({n}, {count}, 0): {r['candidates']} candidates, device {r['device_s']:.4f} s "
                f"({rate:.4g} candidates/s, {r['device_s'] / count * 1e6:.2f} us per accepted graph)")
        if kind == "pair":
            host_per_candidate[n], device_rate[n] = r["host_s"] / r["candidates"], rate
            line += (f", host {r['host_s']:.3f} s ({host_per_candidate[n] * 1e6:.0f} us per candidate): device "
                     f"{r['host_s'] / r['device_s']:.0f}x faster, arrays equal")
        else:
            host = host_per_candidate[n] * r["candidates"]
            line += f", host EXTRAPOLATED {host:.0f} s ({host / 3600:.2f} h) from its time per candidate above"
        print(line, flush=True)


if __name__ == "__main__":
    main()
