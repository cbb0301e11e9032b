"""Device time of the one-sample pairwise U-statistics (tuplewise.onesample, csrc/selfpairs.hip)
beside the host's way to the same numbers (GPU box).

Shapes: Un of every kernel on one block of n = 1e5; the blocks of UnN at n = 1e6, N = 64 (64
blocks of 15625 points); the blocks of UnNB at n = 1e6, N = 64, B = 1e6 (64 x 1e6 index pairs).
Every device time is the median of 5 windows after one warm call, each window `reps`
back-to-back launches (both kernels of an entry point) between two device events, per launch in
ms; the operands are resident, so uploads and the host's draws are outside the windows.  The
whole drop-in calls (host shuffle and draws, upload, launch, read-back) are host-clock medians
of 3.  Host comparisons, one core: scipy.stats.kendalltau (an O(n log n) merge sort, tau-b),
np.var(ddof=1), and a chunked NumPy all-pairs sum for Gini.

Kendall's rate is set against the VALU peak 3.93e13 lane-op/s divided by the inner loop's own
lane-ops per pair (--kendall-lane-ops, counted in the ISA: DESIGN.md §4.9).

--sorted: the sorted path (tw_self_sorted, csrc/selfsorted.hip) beside all pairs, same method:
Kendall and Gini Un at n = 1e4, 1e5, 1e6 with both algorithms and at 1e7 sorted only (the
all-pairs figure there is extrapolated from its pairs/s at 1e6 and marked so), the UnN shape
n = 1e6, N = 64 with both, and the chunk sweep at 1e6; writes profiles/time_onesample_sorted.json.
The split of the sorted Kendall time over its launches comes from a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- \\
        python tools/time_onesample.py --trace-sorted 1000000
    python tools/time_onesample.py --trace-sorted 1000000 --split-from OUT/.../run_kernel_stats.csv

Usage: time_onesample.py [--out profiles/time_onesample.json] [--quick] [--sorted]"""
import argparse
import json
import os
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tuplewise.onesample as os1  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

PEAK_LANE_OPS = 3.93e13
CODES = {"gini": L.TW_SELF_GINI, "var": L.TW_SELF_VAR, "kendall": L.TW_SELF_KENDALL}


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return statistics.median(times)


def host_ms(fn, runs=3):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def make(n, kernel, seed):
    rng = np.random.RandomState(seed)
    if kernel == "kendall":
        a = rng.normal(size=n)
        return np.ascontiguousarray(np.stack([a, 0.6 * a + rng.normal(size=n)], axis=1))
    return rng.normal(1.0, 2.0, n)


def complete_launch(S, blocks, k, kernel):
    """A closure launching tw_self_pairs on `blocks` resident blocks of k items of S."""
    ken = kernel == "kendall"
    sd = L.to_device(S.reshape(-1))
    od = L.to_device(np.arange(blocks + 1, dtype=np.int64) * k)
    work = L.empty((L.lib().tw_self_pairs_work_bytes(blocks, k) // 8,), torch.int64)
    out = L.empty((blocks, 5 if ken else 1), torch.int64 if ken else torch.float64)

    def go():
        L.call("tw_self_pairs", sd, od, blocks, k, L.TW_F64, CODES[kernel], work, out,
               L.stream_handle())
    return go, out


def indexed_launch(S, blocks, k, B, kernel, seed):
    ken = kernel == "kendall"
    rng = np.random.RandomState(seed)
    base = (np.arange(blocks, dtype=np.int64) * k)[:, None]
    ii = rng.randint(0, k, size=(blocks, B))
    jj = rng.randint(0, k - 1, size=(blocks, B))
    jj += jj >= ii
    sd = L.to_device(S.reshape(-1))
    idev = L.to_device((ii + base).reshape(-1).astype(np.int32))
    jdev = L.to_device((jj + base).reshape(-1).astype(np.int32))
    pd = L.to_device(np.arange(blocks + 1, dtype=np.int64) * B)
    work = L.empty((L.lib().tw_self_pairs_idx_work_bytes(blocks, B) // 8,), torch.int64)
    out = L.empty((blocks, 5 if ken else 1), torch.int64 if ken else torch.float64)

    def go():
        L.call("tw_self_pairs_idx32", sd, idev, jdev, pd, blocks, B, L.TW_F64, CODES[kernel],
               work, out, L.stream_handle())
    return go, out


def gini_host(S, chunk=256):
    """Chunked NumPy all-pairs: sum |s_i - s_j| over i < j, chunk rows against the rest."""
    n, tot = len(S), 0.0
    for a in range(0, n, chunk):
        row = S[a:a + chunk, None]
        d = row - S[None, a:a + chunk]
        tot += np.abs(d, out=d).sum() / 2
        if a + chunk < n:
            d = row - S[None, a + chunk:]
            tot += np.abs(d, out=d).sum()
    return tot / (n * (n - 1) / 2)


def host_reference(S, kernel):
    if kernel == "kendall":
        from scipy.stats import kendalltau
        return "scipy.stats.kendalltau", lambda: kendalltau(S[:, 0], S[:, 1]).statistic
    if kernel == "var":
        return "np.var(ddof=1)", lambda: np.var(S, ddof=1)
    return "chunked NumPy all-pairs", lambda: gini_host(S)


def sorted_launch(S, blocks, k, kernel, chunk=0):
    """A closure launching tw_self_sorted on `blocks` resident blocks of k items of S."""
    ken = kernel == "kendall"
    sd = L.to_device(S.reshape(-1))
    od = L.to_device(np.arange(blocks + 1, dtype=np.int64) * k)
    need = L.lib().tw_self_sorted_work_bytes(blocks, blocks * k, k, CODES[kernel], chunk)
    work = L.empty((need // 8,), torch.int64)
    out = L.empty((blocks, 5 if ken else 1), torch.int64 if ken else torch.float64)

    def go():
        L.call("tw_self_sorted", sd, od, blocks, blocks * k, k, L.TW_F64, CODES[kernel], chunk,
               work, out, L.stream_handle())
    return go, out


def same_result(a, b, kernel):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    if kernel == "kendall":
        return bool(np.array_equal(a, b))
    return bool(np.allclose(a, b, rtol=1e-12, atol=0.0))


def phase_of(kernel_name):
    """The phase of tw_self_sorted's Kendall path a kernel belongs to (csrc/selfsorted.hip)."""
    head = kernel_name.split("(")[0]
    if "k_ss_sort_vals" in head or "k_ss_count" in head or "k_ss_compose" in head:
        return "ranks"
    if "k_ss_order" in head or ("k_ss_sort_keys" in head and "false" in head):
        return "order"
    if "k_ss_cross" in head or "k_ss_sort_keys" in head:
        return "inversions"
    if "k_ss_final_kendall" in head or "tw::k_zero_fill" in head:
        return "rest"
    return None


def split_from(csv_path, calls):
    """Device time of one tw_self_sorted call by phase, from the kernel stats of a rocprofv3
    --kernel-trace --stats run of `--trace-sorted` (`calls` launches of the entry point)."""
    import csv
    phases = {"ranks": 0.0, "order": 0.0, "inversions": 0.0, "rest": 0.0}
    kernels = {}
    with open(csv_path, newline="") as f:
        for row in csv.DictReader(f):
            phase = phase_of(row["Name"])
            if phase:
                ms = float(row["TotalDurationNs"]) * 1e-6 / calls
                phases[phase] += ms
                kernels[row["Name"].split("(")[0].replace("void tw::", "")] = ms
    return {"ms_per_call": phases, "kernels_ms_per_call": kernels, "calls": calls}


def sorted_table(a):
    """The sorted path beside all pairs: Un of Kendall and Gini at n = 1e4 .. 1e7 (all pairs at
    1e7 extrapolated from its pairs/s at 1e6), the UnN shape, and the chunk sweep at 1e6."""
    sizes = (2_000, 20_000) if a.quick else (10_000, 100_000, 1_000_000, 10_000_000)
    n2, N = (100_000, 64) if a.quick else (1_000_000, 64)
    res = {"device": torch.cuda.get_device_name(0),
           "chunk": int(L.lib().tw_self_sorted_chunk()),
           "timing": "device events, median of 5 windows of `reps` launches after a warm call, "
                     "ms per launch, resident operands",
           "rows": [], "chunk_sweep": []}
    for kernel in ("kendall", "gini"):
        rate = None
        for n in sizes:
            S = make(n, kernel, 1)
            pairs = n * (n - 1) // 2
            go_s, out_s = sorted_launch(S, 1, n, kernel)
            row = {"shape": f"Un n={n}", "kernel": kernel, "pairs": pairs,
                   "sorted_ms": device_ms(go_s, 20 if n <= 100_000 else 3 if n <= 1_000_000 else 1)}
            if n <= 1_000_000:
                go_p, out_p = complete_launch(S, 1, n, kernel)
                row["pairs_ms"] = device_ms(go_p, 20 if n <= 100_000 else 1)
                row["same_result"] = same_result(out_s, out_p, kernel)
                rate = pairs / row["pairs_ms"]
            else:
                row["pairs_ms_extrapolated"] = pairs / rate  # at the pairs/s of the size before
            row["speedup"] = row.get("pairs_ms", row.get("pairs_ms_extrapolated")) / row["sorted_ms"]
            print(json.dumps(row), flush=True)
            res["rows"].append(row)
            del go_s, out_s
            torch.cuda.empty_cache()
        S = make(n2, kernel, 2)
        k = n2 // N
        go_s, out_s = sorted_launch(S, N, k, kernel)
        go_p, out_p = complete_launch(S, N, k, kernel)
        row = {"shape": f"UnN n={n2} N={N}", "kernel": kernel, "pairs": N * (k * (k - 1) // 2),
               "sorted_ms": device_ms(go_s, 5), "pairs_ms": device_ms(go_p, 5)}
        row["same_result"] = same_result(out_s, out_p, kernel)
        row["speedup"] = row["pairs_ms"] / row["sorted_ms"]
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    n = sizes[-2]
    S = make(n, "kendall", 1)
    for chunk in (1024, 2048, 4096, 8192, 16384):
        go_s, _ = sorted_launch(S, 1, n, "kendall", chunk)
        row = {"shape": f"Un n={n}", "kernel": "kendall", "chunk": chunk,
               "sorted_ms": device_ms(go_s, 3)}
        print(json.dumps(row), flush=True)
        res["chunk_sweep"].append(row)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="n = 2e4 / 1e5 instead of 1e5 / 1e6")
    ap.add_argument("--kendall-lane-ops", type=float, default=11.75,
                    help="VALU instructions per pair of the Kendall inner loop (from the ISA)")
    ap.add_argument("--sorted", action="store_true",
                    help="the sorted path beside all pairs (profiles/time_onesample_sorted.json)")
    ap.add_argument("--trace-sorted", type=int, default=0, metavar="N",
                    help="only launch the sorted Kendall count of N points --calls times: the "
                         "program of a rocprofv3 --kernel-trace --stats run")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--split-from", default=None, metavar="CSV",
                    help="add the per-phase split from that run's kernel stats to --out")
    a = ap.parse_args()
    sorted_out = a.out or str(ROOT / "profiles" / "time_onesample_sorted.json")
    if a.split_from:
        res = json.loads(pathlib.Path(sorted_out).read_text())
        res["split"] = dict(split_from(a.split_from, a.calls), n=a.trace_sorted)
        pathlib.Path(sorted_out).write_text(json.dumps(res, indent=1) + "\n")
        print(json.dumps(res["split"]))
        return
    torch.cuda.set_device(0)
    if a.trace_sorted:
        go, _ = sorted_launch(make(a.trace_sorted, "kendall", 1), 1, a.trace_sorted, "kendall")
        for _ in range(a.calls):
            go()
        torch.cuda.synchronize()
        return
    if a.sorted:
        res = sorted_table(a)
        out = pathlib.Path(sorted_out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(res, indent=1) + "\n")
        return
    a.out = a.out or str(ROOT / "profiles" / "time_onesample.json")
    if hasattr(os, "sched_setaffinity"):  # the host comparisons on one core
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})
    torch.set_num_threads(1)
    n1, n2, N = (20_000, 100_000, 64) if a.quick else (100_000, 1_000_000, 64)
    B = n2
    k = n2 // N
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_self_pairs_tile()),
           "timing": "device: median of 5 windows of `reps` launches after a warm call, device "
                     "events, ms per launch, resident operands; *_call_ms and host_ms: median of "
                     "3 host-clock runs on one core",
           "peak_lane_ops": PEAK_LANE_OPS, "kendall_lane_ops_per_pair": a.kendall_lane_ops,
           "rows": []}
    for kernel in ("gini", "var", "kendall"):
        # ---- Un, one block of n1
        S = make(n1, kernel, 1)
        go, out = complete_launch(S, 1, n1, kernel)
        pairs = n1 * (n1 - 1) // 2
        ms = device_ms(go, 1 if pairs >= 1 << 31 else 20)
        row = {"shape": f"Un n={n1}", "kernel": kernel, "pairs": pairs, "device_ms": ms,
               "pairs_per_s": pairs / (ms * 1e-3)}
        value = os1.Un(S, kernel)
        row["value"] = float(value)
        row["call_ms"] = host_ms(lambda: os1.Un(S, kernel))
        name, ref = host_reference(S, kernel)
        row["host"], row["host_ms"] = name, host_ms(ref, 1 if kernel == "gini" else 3)
        want = ref()
        row["host_value"] = float(want)
        if kernel == "kendall":  # continuous data: no ties, tau-b = tau-a
            assert abs(value - want) <= 1e-12 * abs(want), (value, want)
            row["frac_of_valu_bound"] = row["pairs_per_s"] / (PEAK_LANE_OPS / a.kendall_lane_ops)
        else:
            assert abs(value - want) <= 1e-10 * abs(want), (value, want)
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        # ---- UnN's blocks: N blocks of k
        S = make(n2, kernel, 2)
        go, out = complete_launch(S, N, k, kernel)
        pairs = N * (k * (k - 1) // 2)
        ms = device_ms(go, 5)
        row = {"shape": f"UnN n={n2} N={N}", "kernel": kernel, "pairs": pairs, "device_ms": ms,
               "pairs_per_s": pairs / (ms * 1e-3)}
        if kernel == "kendall":
            row["frac_of_valu_bound"] = row["pairs_per_s"] / (PEAK_LANE_OPS / a.kendall_lane_ops)
        np.random.seed(0)
        row["call_ms"] = host_ms(lambda: os1.UnN(S, N, kernel))
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        # ---- UnNB's blocks: N x B index pairs
        go, out = indexed_launch(S, N, k, B, kernel, 3)
        ms = device_ms(go, 5)
        row = {"shape": f"UnNB n={n2} N={N} B={B}", "kernel": kernel, "pairs": N * B,
               "device_ms": ms, "pairs_per_s": N * B / (ms * 1e-3)}
        np.random.seed(0)
        row["call_ms"] = host_ms(lambda: os1.UnNB(S, N, B, kernel))
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
