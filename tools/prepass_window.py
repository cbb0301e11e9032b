"""The pre-pass window of the headline's chain count from a rocprofv3
--kernel-trace CSV of `bench.py --steps K --warmup 1 --settle-ms 0 --no-cpu-baseline --no-sgd`
(tools/prof_chain.sh's trace line): for every K-step launch of k_count_chain_classes (largest
grid, at least half the longest duration) the kernels that run directly before it on the stream
inside the same native call — k_zero_fill, k_chain_planes, k_chain_zclasses, or the one
k_chain_prepass — with their durations, and the WINDOW from the first one's start to the count
kernel's start, which holds the launch gaps between them too.  In time order the second launch
is the bench's timed call.
    python3 tools/prepass_window.py TRACE.csv OUT.json"""
import csv
import json
import sys

path, out = sys.argv[1], sys.argv[2]
PRE = ("k_zero_fill", "k_chain_planes<", "k_chain_zclasses", "k_chain_prepass<")
rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
t0 = lambda r: int(r["Start_Timestamp"])
t1 = lambda r: int(r["End_Timestamp"])
grid = lambda r: int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
short = lambda r: next((p.rstrip("<") for p in PRE if p in r["Kernel_Name"]), r["Kernel_Name"])
counts = [i for i, r in enumerate(rows) if "k_count_chain_classes<" in r["Kernel_Name"]]
g = max(grid(rows[i]) for i in counts)
big = [i for i in counts if grid(rows[i]) == g]
longest = max(t1(rows[i]) - t0(rows[i]) for i in big)
big = [i for i in big if t1(rows[i]) - t0(rows[i]) >= 0.5 * longest]
launches = []
for i in big:
    j = i
    while j > 0 and any(p in rows[j - 1]["Kernel_Name"] for p in PRE):
        j -= 1
    pre = rows[j:i]
    first = t0(pre[0]) if pre else t0(rows[i])
    launches.append({
        "prepass_kernels_us": [[short(r), (t1(r) - t0(r)) / 1e3] for r in pre],
        "prepass_kernels_sum_us": sum(t1(r) - t0(r) for r in pre) / 1e3,
        "window_us": (t0(rows[i]) - first) / 1e3,
        "count_kernel_us": (t1(rows[i]) - t0(rows[i])) / 1e3,
        "call_span_us": (t1(rows[i]) - first) / 1e3,
    })
timed = launches[min(1, len(launches) - 1)]
res = {"source": path, "count_kernel": rows[big[0]]["Kernel_Name"].split("(")[0], "grid": g,
       "timed_call": dict(timed, window_over_span=timed["window_us"] / timed["call_span_us"]),
       "launches_in_order": launches}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res["timed_call"], indent=1))
