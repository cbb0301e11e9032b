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

Usage: time_onesample.py [--out profiles/time_onesample.json] [--quick]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_onesample.json"))
    ap.add_argument("--quick", action="store_true", help="n = 2e4 / 1e5 instead of 1e5 / 1e6")
    ap.add_argument("--kendall-lane-ops", type=float, default=11.75,
                    help="VALU instructions per pair of the Kendall inner loop (from the ISA)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
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
