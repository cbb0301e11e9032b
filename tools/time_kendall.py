"""Device time of the Kendall tau matrix (tuplewise.kendall, csrc/kendall.hip) beside the parent's
way to the same numbers: one (n, 2) Kendall call per column pair (GPU box).

Shapes: n = 1e4 with p in {2, 16, 64, 256}; 64 blocks of 1562 rows at p = 64; n = 1e5 at p = 16.
tw_col_ranks and tw_kendall_matrix are timed separately on resident operands: the median of 5
windows after one warm call, each window `reps` back-to-back launches between two device events,
ms per launch.  The whole tau_matrix call (upload, both launches, read-back, the host's float
matrix) is a host-clock median of 3.

The baseline, in the same run: tw_self_pairs (Kendall) and tw_self_sorted on resident (n, 2)
column pairs, each the mean over a sample of 32 column pairs (every column pair of the table
when it has fewer), scaled to the p (p - 1) / 2 launches the matrix takes that way (uploads not
counted: the scaling favours the baseline).  The integers of the sampled pairs are checked
against the matrix.

The bound of the pair kernel: pairs x columns generated x VALU instructions per sign /
3.93e13 lane-op/s, and the matrix time at the int8 rate (--int8-ops, multiply-adds per second);
the share of the bound is given against their maximum (the units overlap) and their sum (they
do not).

Usage: time_kendall.py [--out profiles/time_kendall.json] [--quick]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tuplewise.kendall as K  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

PEAK_LANE_OPS = 3.93e13
GROUP = 64  # columns per group of csrc/kendall.hip


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


def make(n, p, seed):
    rng = np.random.RandomState(seed)
    base = rng.normal(size=(n, 1))
    return np.ascontiguousarray(0.5 * base + rng.normal(size=(n, p)))


def matrix_launches(S, blocks, k):
    """Closures launching tw_col_ranks and tw_kendall_matrix on resident blocks of k rows."""
    lib = L.lib()
    p = S.shape[1]
    total = blocks * k
    width = int(lib.tw_kendall_matrix_width(k))
    sd = L.to_device(S[:total].reshape(-1))
    od = L.to_device(np.arange(blocks + 1, dtype=np.int64) * k)
    rwork = L.empty((max(1, lib.tw_col_ranks_work_bytes(blocks, total, k, p) // 8),), torch.int64)
    ranks = L.empty((total * p,), torch.int16 if width == 16 else torch.int32)
    mwork = L.empty((max(1, lib.tw_kendall_matrix_work_bytes(blocks, p, p) // 8),), torch.int64)
    M = L.empty((blocks, p, p), torch.int64)
    Ua, Ub = L.empty((blocks, p), torch.int64), L.empty((blocks, p), torch.int64)

    def go_ranks():
        L.call("tw_col_ranks", sd, od, blocks, total, k, p, L.TW_F64, width, rwork, ranks,
               L.stream_handle())

    def go_matrix():
        L.call("tw_kendall_matrix", ranks, p, ranks, p, od, blocks, k, width, mwork, M, Ua, Ub,
               L.stream_handle())
    return go_ranks, go_matrix, M, Ua, width


def pair_baseline(S, blocks, k, pairs_cols, reps):
    """Mean device ms per (n, 2) launch of tw_self_pairs and tw_self_sorted over the sampled
    column pairs, and their counters for the check."""
    lib = L.lib()
    total = blocks * k
    od = L.to_device(np.arange(blocks + 1, dtype=np.int64) * k)
    wp = L.empty((max(1, lib.tw_self_pairs_work_bytes(blocks, k) // 8),), torch.int64)
    ws = L.empty((max(1, lib.tw_self_sorted_work_bytes(blocks, total, k, L.TW_SELF_KENDALL, 0) // 8),),
                 torch.int64)
    out_p = L.empty((blocks, 5), torch.int64)
    out_s = L.empty((blocks, 5), torch.int64)
    t_pairs, t_sorted, counters = [], [], []
    for a, b in pairs_cols:
        sd = L.to_device(np.ascontiguousarray(S[:total, [a, b]]).reshape(-1))

        def go_p():
            L.call("tw_self_pairs", sd, od, blocks, k, L.TW_F64, L.TW_SELF_KENDALL, wp, out_p,
                   L.stream_handle())

        def go_s():
            L.call("tw_self_sorted", sd, od, blocks, total, k, L.TW_F64, L.TW_SELF_KENDALL, 0, ws,
                   out_s, L.stream_handle())
        t_pairs.append(device_ms(go_p, reps))
        t_sorted.append(device_ms(go_s, reps))
        cp, cs = out_p.cpu().numpy(), out_s.cpu().numpy()
        assert np.array_equal(cp, cs)
        counters.append(cp)
    return statistics.mean(t_pairs), statistics.mean(t_sorted), counters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_kendall.json"))
    ap.add_argument("--quick", action="store_true", help="n = 2000 / 1e4 instead of 1e4 / 1e5")
    ap.add_argument("--sign-ops16", type=float, default=1.75,
                    help="VALU instructions per sign of the 16-bit inner loop (from the ISA)")
    ap.add_argument("--sign-ops32", type=float, default=2.75)
    ap.add_argument("--int8-ops", type=float, default=2.5e15,
                    help="dense int8 multiply-adds per second of the matrix unit")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    n1, n2 = (2000, 10_000) if a.quick else (10_000, 100_000)
    shapes = [(n1, 1, p) for p in (2, 16, 64, 256)]
    shapes += [(64 * (n1 * 10 // 64), 64, 64), (n2, 1, 16)]
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_kendall_matrix_tile()),
           "timing": "device events, median of 5 windows of `reps` launches after a warm call, ms "
                     "per launch, resident operands; call_ms: median of 3 host-clock runs",
           "peak_lane_ops": PEAK_LANE_OPS, "int8_ops": a.int8_ops,
           "sign_ops": {"16": a.sign_ops16, "32": a.sign_ops32}, "rows": []}
    for n, blocks, p in shapes:
        k = n // blocks
        S = make(n, p, 7 + p)
        go_r, go_m, M, Ua, width = matrix_launches(S, blocks, k)
        reps = 3 if n * p > 2_000_000 else 10
        row = {"shape": f"n={n} blocks={blocks} p={p}", "width": width,
               "pairs": blocks * (k * (k - 1) // 2), "ranks_ms": device_ms(go_r, reps),
               "matrix_ms": device_ms(go_m, reps)}
        row["both_ms"] = row["ranks_ms"] + row["matrix_ms"]
        if blocks == 1:
            row["call_ms"] = host_ms(lambda: K.tau_matrix(S))
        # the bound: the diagonal groups generate 64 columns per pair, the others 128
        g = -(-p // GROUP)
        cols = min(p, GROUP) if g == 1 else GROUP * g + 2 * GROUP * (g * (g - 1) // 2)
        ops = a.sign_ops16 if width == 16 else a.sign_ops32
        valu_ms = row["pairs"] * cols * ops / PEAK_LANE_OPS * 1e3
        blocks16 = -(-min(p, GROUP) // 16)
        prods = blocks16 * (blocks16 + 1) // 2 if g == 1 else 10 * g + 16 * (g * (g - 1) // 2)
        mfma_ms = row["pairs"] * prods * 256 / a.int8_ops * 1e3
        row.update(valu_bound_ms=valu_ms, mfma_bound_ms=mfma_ms,
                   share_of_max=max(valu_ms, mfma_ms) / row["matrix_ms"],
                   share_of_sum=(valu_ms + mfma_ms) / row["matrix_ms"])
        # the parent's way: one launch per column pair
        all_pairs = [(i, j) for i in range(p) for j in range(i + 1, p)]
        rng = np.random.RandomState(p)
        pick = all_pairs if len(all_pairs) <= 32 else [all_pairs[i] for i in
                                                       rng.choice(len(all_pairs), 32, False)]
        tp, ts, counters = pair_baseline(S, blocks, k, pick, 3)
        Mh, Uh = M.cpu().numpy(), Ua.cpu().numpy()
        P = k * (k - 1) // 2
        for (i, j), c in zip(pick, counters):
            assert np.array_equal(Mh[:, i, j], c[:, 0] - c[:, 1]), (i, j)
            assert np.array_equal(Uh[:, i], P - c[:, 2]) and np.array_equal(Uh[:, j], P - c[:, 3])
        row.update(column_pairs=len(all_pairs), sampled=len(pick), self_pairs_ms_per_launch=tp,
                   self_sorted_ms_per_launch=ts, self_pairs_scaled_ms=tp * len(all_pairs),
                   self_sorted_scaled_ms=ts * len(all_pairs), same_integers=True)
        row["ratio_to_self_pairs"] = row["self_pairs_scaled_ms"] / row["both_ms"]
        row["ratio_to_self_sorted"] = row["self_sorted_scaled_ms"] / row["both_ms"]
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        del go_r, go_m, M, Ua
        torch.cuda.empty_cache()
    bar = next(r for r in res["rows"] if r["shape"] == f"n={n1} blocks=1 p=64")
    res["bar"] = {"shape": bar["shape"], "required_ratio_to_self_pairs": 30.0,
                  "ratio_to_self_pairs": bar["ratio_to_self_pairs"],
                  "met": bool(bar["ratio_to_self_pairs"] >= 30.0)}
    print(json.dumps(res["bar"]), flush=True)
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
