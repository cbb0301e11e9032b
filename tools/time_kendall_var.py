"""Device time of the Kendall row sums (tuplewise.kendall_var, csrc/kendall_rows.hip) beside the
matrix kernel on the same rank image (GPU box).

Shapes: n = 1e4 with p in {2, 16, 64, 256}; 64 blocks of 1562 rows at p = 64; n = 1e5 at p = 16.
tw_kendall_rows and, in the same run, tw_kendall_matrix are timed on one resident rank image of
tw_col_ranks: the median of 5 windows after one warm call, each window `reps` back-to-back
launches between two device events, ms per launch.  R == 2 M is checked at every shape.

The bar: at n = 1e4, p = 64 the rows launch takes at most 2 x 1.15 of the matrix launch (ordered
against unordered pairs, and the margin of DESIGN.md §4.17 for the per-anchor epilogue).

The bound of the rows kernel: ordered pairs x columns generated x VALU instructions per sign
(--sign-ops16 / --sign-ops32, counted in the loop's ISA) / 3.93e13 lane-op/s, and the matrix time
at the int8 rate (--int8-ops); the share of the bound is given against their maximum (the units
overlap) and their sum (they do not).

--sweep adds the rows launch at the bar's shape under every anchor count and a few plans.
Whole calls (host clock): tau_var at n = 1e4, p = 64 and p = 1024 with the host's integer
arithmetic timed alone, and a one-core NumPy restatement of the row sums at n = 1e4, p = 16 on
1000 anchors, scaled (a child process with one BLAS thread; --numpy-only is that child).

Usage: time_kendall_var.py [--out profiles/time_kendall_var.json] [--quick] [--sweep]"""
import argparse
import json
import os
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402

PEAK_LANE_OPS = 3.93e13
GROUP = 64  # columns per group of csrc/kendall_rows.hip


def make(n, p, seed):
    rng = np.random.RandomState(seed)
    base = rng.normal(size=(n, 1))
    return np.ascontiguousarray(0.5 * base + rng.normal(size=(n, p)))


def numpy_rows(S, anchors):
    """R, Q, F, E of the first `anchors` points against all of S, in float64 NumPy."""
    n, p = S.shape
    R, Q, F, E = (np.zeros((p, p)) for _ in range(4))
    for lo in range(0, anchors, 128):
        A = S[lo:min(anchors, lo + 128)]
        s = np.sign(A[:, None, :] - S[None, :, :])
        c = np.matmul(s.transpose(0, 2, 1), s)
        u = np.einsum("iaa->ia", c)
        R += c.sum(axis=0)
        Q += (c * c).sum(axis=0)
        F += (c * u[:, :, None]).sum(axis=0)
        E += u.T @ u
    return R, Q, F, E


def numpy_only(n, p, anchors):
    S = make(n, p, 7 + p)
    t0 = time.perf_counter()
    numpy_rows(S, anchors)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"shape": f"n={n} p={p}", "anchors": anchors, "ms": ms,
                      "scaled_ms": ms * n / anchors, "threads": 1}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_kendall_var.json"))
    ap.add_argument("--quick", action="store_true", help="n = 2000 / 1e4 instead of 1e4 / 1e5")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--numpy-only", action="store_true")
    ap.add_argument("--sign-ops16", type=float, default=1.83,
                    help="VALU instructions per sign of the 16-bit chunk loop (from the ISA)")
    ap.add_argument("--sign-ops32", type=float, default=2.76)
    ap.add_argument("--int8-ops", type=float, default=2.5e15,
                    help="dense int8 multiply-adds per second of the matrix unit")
    a = ap.parse_args()
    n1, n2 = (2000, 10_000) if a.quick else (10_000, 100_000)
    if a.numpy_only:
        return numpy_only(n1, 16, min(1000, n1))

    import torch
    import tuplewise.kendall_var as V
    from tuplewise import _lib as L
    torch.cuda.set_device(0)
    lib = L.lib()

    def device_ms(fn, reps):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1) / reps)
        return statistics.median(times)

    def launches(S, blocks, k):
        """The resident rank image of S and closures launching both kernels on it."""
        p = S.shape[1]
        total = blocks * k
        width = int(lib.tw_kendall_matrix_width(k))
        sd = L.to_device(S[:total].reshape(-1))
        od = L.to_device(np.arange(blocks + 1, dtype=np.int64) * k)
        rwork = L.empty((max(1, lib.tw_col_ranks_work_bytes(blocks, total, k, p) // 8),), torch.int64)
        ranks = L.empty((total * p,), torch.int16 if width == 16 else torch.int32)
        L.call("tw_col_ranks", sd, od, blocks, total, k, p, L.TW_F64, width, rwork, ranks,
               L.stream_handle())
        mwork = L.empty((max(1, lib.tw_kendall_matrix_work_bytes(blocks, p, p) // 8),), torch.int64)
        M = L.empty((blocks, p, p), torch.int64)
        Ua, Ub = L.empty((blocks, p), torch.int64), L.empty((blocks, p), torch.int64)
        vwork = L.empty((max(1, lib.tw_kendall_rows_work_bytes(blocks, p) // 8),), torch.int64)
        out = [L.empty((blocks, p, p), torch.int64) for _ in range(4)]

        def go_matrix():
            L.call("tw_kendall_matrix", ranks, p, ranks, p, od, blocks, k, width, mwork, M, Ua, Ub,
                   L.stream_handle())

        def go_rows():
            L.call("tw_kendall_rows", ranks, p, od, blocks, k, width, vwork, *out,
                   L.stream_handle())
        return go_matrix, go_rows, M, out[0], width

    shapes = [(n1, 1, p) for p in (2, 16, 64, 256)]
    shapes += [(64 * (n1 * 10 // 64), 64, 64), (n2, 1, 16)]
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "device events, median of 5 windows of `reps` launches after a warm call, ms "
                     "per launch, one resident rank image for both kernels; *_call_ms: host clock",
           "peak_lane_ops": PEAK_LANE_OPS, "int8_ops": a.int8_ops,
           "sign_ops": {"16": a.sign_ops16, "32": a.sign_ops32}, "rows": []}
    for n, blocks, p in shapes:
        k = n // blocks
        S = make(n, p, 7 + p)
        go_m, go_v, M, R, width = launches(S, blocks, k)
        reps = 3 if n * p > 2_000_000 else 10
        row = {"shape": f"n={n} blocks={blocks} p={p}", "width": width,
               "ordered_pairs": blocks * k * (k - 1), "matrix_ms": device_ms(go_m, reps),
               "rows_ms": device_ms(go_v, reps)}
        row["rows_over_matrix"] = row["rows_ms"] / row["matrix_ms"]
        assert torch.equal(R, 2 * M), row["shape"]
        row["R_is_2M"] = True
        # the bound: a diagonal group generates its own columns per ordered pair; a pair of
        # groups runs as two halves of 64 + 32 columns, 8 products and 6 squares each
        g = -(-p // GROUP)
        nb = -(-min(p, GROUP) // 16)
        cols = 16 * nb if g == 1 else GROUP * g + 192 * (g * (g - 1) // 2)
        prods = nb * (nb + 1) // 2 if g == 1 else 10 * g + 28 * (g * (g - 1) // 2)
        ops = a.sign_ops16 if width == 16 else a.sign_ops32
        valu_ms = row["ordered_pairs"] * cols * ops / PEAK_LANE_OPS * 1e3
        mfma_ms = row["ordered_pairs"] * prods * 256 / a.int8_ops * 1e3
        row.update(valu_bound_ms=valu_ms, mfma_bound_ms=mfma_ms,
                   share_of_max=max(valu_ms, mfma_ms) / row["rows_ms"],
                   share_of_sum=(valu_ms + mfma_ms) / row["rows_ms"])
        print(json.dumps(row), flush=True)
        res["rows"].append(row)
        if a.sweep and (n, blocks, p) == (n1, 1, 64):
            sweep = []
            for anchors in (1, 2, 4):
                for plan in (0, 128, 256, 512, 1024):
                    lib.tw_kendall_rows_set_anchors(anchors)
                    lib.tw_kendall_rows_set_plan(plan)
                    try:
                        sweep.append({"anchors": anchors, "plan": plan,
                                      "rows_ms": device_ms(go_v, reps)})
                    finally:
                        lib.tw_kendall_rows_set_anchors(0)
                        lib.tw_kendall_rows_set_plan(0)
                    print(json.dumps(sweep[-1]), flush=True)
            res["sweep"] = {"shape": row["shape"], "points": sweep}
        del go_m, go_v, M, R
        torch.cuda.empty_cache()
    bar = next(r for r in res["rows"] if r["shape"] == f"n={n1} blocks=1 p=64")
    res["bar"] = {"shape": bar["shape"], "allowed_rows_over_matrix": 2 * 1.15,
                  "rows_over_matrix": bar["rows_over_matrix"],
                  "met": bool(bar["rows_over_matrix"] <= 2 * 1.15)}
    print(json.dumps(res["bar"]), flush=True)

    # whole calls: upload, ranks, rows, read-back, and the host's integer arithmetic
    calls = []
    for p in (64, 1024):
        S = make(n1, p, 7 + p)
        V.tau_var(S[:64])  # warm
        runs = 3 if p == 64 else 1
        t_call, t_host = [], []
        for _ in range(runs):
            t0 = time.perf_counter()
            V.tau_var(S)
            t_call.append((time.perf_counter() - t0) * 1e3)
        m = V.row_moments(S)
        for _ in range(runs):
            t0 = time.perf_counter()
            V._var_b_matrix(m.R, m.Q, m.F, m.E, m.n)
            V._tau(m.R, m.n, "b")
            t_host.append((time.perf_counter() - t0) * 1e3)
        calls.append({"shape": f"n={n1} p={p}", "tau_var_call_ms": statistics.median(t_call),
                      "host_arithmetic_ms": statistics.median(t_host), "runs": runs})
        print(json.dumps(calls[-1]), flush=True)
    res["whole_calls"] = calls
    env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
    child = subprocess.run([sys.executable, __file__, "--numpy-only"] + (["--quick"] if a.quick else []),
                           env=env, capture_output=True, text=True, timeout=900)
    if child.returncode == 0:
        res["numpy_one_core"] = json.loads(child.stdout.strip().splitlines()[-1])
        print(json.dumps(res["numpy_one_core"]), flush=True)
    else:
        res["numpy_one_core"] = {"error": child.stderr[-500:]}
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
