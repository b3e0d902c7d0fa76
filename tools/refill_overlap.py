"""What the episode refill on the side stream does to the main stream's kernels: python tools/refill_overlap.py <kernel_trace.csv>
(rocprofv3 --kernel-trace --output-format csv -- python bench.py --steps 200 --warmup 30; per-launch rows, not --stats).

Over the last STEPS (default 190) graph-replayed steps it splits the launches of conv2's GEMM (gemm_planes_kernel), of
gemm_split_big_kernel<3> and of the two attention launches into those whose span intersects the span of any episode_* kernel and
those that do not, and prints count, mean, median, max and standard deviation of both groups.  Then the refills themselves: mean
duration of every refill kernel, the span from the gate's end (wait_counter_kernel) to the end of episode_publish_kernel, and
the window the refill has - from the gate's end to the start of the next gemm_planes_kernel launch.  One JSON line at the end."""
import csv
import json
import statistics
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 190
span = lambda r: (int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
short = lambda r: r["Kernel_Name"].split("(")[0].replace("void ", "").replace("mel::", "")
first = [i for i, r in enumerate(rows) if "plan_enc_kernel" in r["Kernel_Name"]][-(steps + 1):]
t0, t1 = int(rows[first[0]]["Start_Timestamp"]), int(rows[first[-1]]["Start_Timestamp"])
timed = [r for r in rows if t0 <= int(r["Start_Timestamp"]) < t1]
side = [span(r) for r in timed if "episode_" in r["Kernel_Name"]]


def stats(us):
    if not us:
        return dict(count=0)
    return dict(count=len(us), mean=round(statistics.mean(us), 2), median=round(statistics.median(us), 2),
                max=round(max(us), 2), sd=round(statistics.pstdev(us), 2))


out = {"steps": len(first) - 1, "us_per_step": round((t1 - t0) / 1e3 / (len(first) - 1), 2), "kernels": {}}
groups = {}
for r in timed:
    name = short(r)
    if any(k in name for k in ("gemm_planes_kernel", "gemm_split_big_kernel<3", "gat_attend_rows_kernel")):
        s, e = span(r)
        hit = any(s < b and a < e for a, b in side)
        groups.setdefault(name[:70], {True: [], False: []})[hit].append((e - s) / 1e3)
for name, g in groups.items():
    out["kernels"][name] = {"overlapped": stats(g[True]), "free": stats(g[False])}
    print(f"{name}\n    beside a refill kernel {stats(g[True])}\n    alone                  {stats(g[False])}")

# ---- the refills: gate -> draw ... publish
gates = [r for r in timed if "wait_counter_kernel" in r["Kernel_Name"]]
planes = [int(r["Start_Timestamp"]) for r in timed if "gemm_planes_kernel" in r["Kernel_Name"]]
per_kernel, spans, windows = {}, [], []
for g in gates:
    g_end = int(g["End_Timestamp"])
    pub = next((r for r in timed if "episode_publish_kernel" in r["Kernel_Name"] and int(r["Start_Timestamp"]) >= g_end), None)
    if pub is None:
        continue
    p_end = int(pub["End_Timestamp"])
    for r in timed:
        if "episode_" in r["Kernel_Name"] and g_end <= int(r["Start_Timestamp"]) <= p_end:
            per_kernel.setdefault(short(r)[:40], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    spans.append((p_end - g_end) / 1e3)
    nxt = [p for p in planes if p >= g_end]
    if nxt:
        windows.append((nxt[0] - g_end) / 1e3)
out["refill_kernels"] = {k: stats(v) for k, v in per_kernel.items()}
out["gate_to_publish_us"], out["gate_to_next_planes_us"] = stats(spans), stats(windows)
for k, v in out["refill_kernels"].items():
    print(f"{k:<42s} {v}")
print("gate end -> publish end        ", out["gate_to_publish_us"])
print("gate end -> next planes launch ", out["gate_to_next_planes_us"])
print(json.dumps(out))
