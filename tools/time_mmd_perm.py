"""Device and call time of the MMD / energy permutation test (tuplewise.mmd.permutation_test,
csrc/mmd_perm.hip) beside the only way the package had before it: one host permutation and one
mm.Un call per permutation (GPU box).

Shapes: n = m = 1e4 at d in {2, 8, 64} with P in {100, 1000} permutations, both kernels, and one
small shape (n = m = 500, d = 8, P = 1000).  Per shape:
  device_ms        tw_mmd_perm_sums on resident operands (P + 1 columns: the observed split and the
                   permutations), the median of 5 windows of back-to-back calls between two device
                   events after one warm call
  bound_ms         pairs * columns multiply-adds at the measured rate of v_mfma_f64_16x16x4_f64
                   (profiles/mb_mfma_f64.log: 64 cycles an instruction, 16 multiply-adds a cycle
                   and SIMD, 1024 SIMDs at 2.4 GHz) plus ONE evaluation of g per pair at the
                   float64 VALU rate (tools/time_mmd.py's lane-ops per pair) — the vector unit
                   does not run beside the matrix unit (the same log), so the two add
  share_of_bound   bound_ms / device_ms
  call_ms          the whole permutation_test call (draws, packing, upload, launch, read-back),
                   host clock, median of 3; draws_ms the P np.random.permutation calls and the
                   label rows alone
  baseline_*       per permutation: np.random.permutation, the two gathers and mm.Un (upload,
                   launch, read-back), `baseline_iters` iterations timed on the host clock and
                   scaled to P (baseline_call_ms); baseline_device_ms is tw_mmd_sums on resident
                   operands times P
  ratio_call, ratio_device   baseline over this module

Usage: time_mmd_perm.py [--out profiles/time_mmd_perm.json] [--quick] [--lib path/to/variant.so]"""
import argparse
import json
import math
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tuplewise import _lib as L  # noqa: E402

F64_VALU_LANE_OPS = 3.93e13  # lane-ops/s (tools/time_mmd.py)
MFMA_F64_MACS = 16 * 1024 * 2.4e9  # multiply-adds/s: 1024 per 64-cycle instruction and SIMD
FOLD = {"gaussian": (673 / 32, 98 / 32), "energy": (481 / 32, 129 / 32)}  # tools/time_mmd.py


def lane_ops(d, kernel):
    f64, other = FOLD[kernel]
    return (3.0 + 0.5 * 16 / 256) * d + f64 + 0.5 * other


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


def reps_for(ms_guess):
    return max(1, min(200, int(200 / max(ms_guess, 1e-3))))


def shape(mm, n, m, d, P, kernel, baseline_iters):
    rng = np.random.RandomState(d + P)
    X, Z = rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(m, d))
    sigma = math.sqrt(d) if kernel == "gaussian" else None
    kid, c = mm._coef(kernel, sigma)
    N, cols = n + m, P + 1
    labels = np.zeros((cols, N), dtype=bool)
    labels[0, :n] = True
    for p in range(1, cols):
        labels[p, rng.permutation(N)[:n]] = True
    packed = np.packbits(labels.T, axis=1, bitorder="little")
    words = np.zeros((N, 4 * ((cols + 31) // 32)), dtype=np.uint8)
    words[:, :packed.shape[1]] = packed
    wd = L.to_device(np.concatenate([X, Z]).reshape(-1))
    ld = L.to_device(words.view("<i4").reshape(-1))
    work = L.empty((int(L.lib().tw_mmd_perm_work_bytes(N, cols)) // 8,), torch.float64)
    out = L.empty((cols, 3), torch.float64)

    def go():
        L.call("tw_mmd_perm_sums", wd, N, d, ld, cols, kid, c, work, out, L.stream_handle())

    t = device_ms(go, reps_for(device_ms(go, 1)))
    pairs = N * (N - 1) // 2
    mfma_ms = pairs * cols / MFMA_F64_MACS * 1e3
    g_ms = pairs * lane_ops(d, kernel) / F64_VALU_LANE_OPS * 1e3
    rec = {"n": n, "m": m, "d": d, "P": P, "kernel": kernel, "pairs": pairs, "device_ms": t,
           "mfma_bound_ms": mfma_ms, "g_once_ms": g_ms, "bound_ms": mfma_ms + g_ms,
           "share_of_bound": (mfma_ms + g_ms) / t,
           "pair_columns_per_s": pairs * cols / (t * 1e-3)}

    # the whole call, and its host draws alone
    def call():
        np.random.seed(1)
        return mm.permutation_test(X, Z, P, kernel, sigma)

    def draws():
        np.random.seed(1)
        lab = np.zeros((P + 1, N), dtype=bool)
        for p in range(1, P + 1):
            lab[p, np.random.permutation(N)[:n]] = True
        return lab

    res = call()
    rec["call_ms"] = host_ms(call)
    rec["draws_ms"] = host_ms(draws)
    rec["pvalue"] = res.pvalue

    # the baseline: one host permutation and one mm.Un per permutation
    pool = np.concatenate([X, Z])

    def one():
        pi = np.random.permutation(N)
        return mm.Un(pool[pi[:n]], pool[pi[n:]], kernel, sigma)

    one()
    t0 = time.perf_counter()
    for _ in range(baseline_iters):
        one()
    per = (time.perf_counter() - t0) * 1e3 / baseline_iters
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    bx, bz = (L.to_device(np.array([0, k], dtype=np.int64)) for k in (n, m))
    w2 = L.empty((int(L.lib().tw_mmd_work_bytes(1, n, m)) // 8,), torch.float64)
    o2 = L.empty((1, 3), torch.float64)

    def un():
        L.call("tw_mmd_sums", xd, zd, d, bx, bz, 1, n, m, kid, c, w2, o2, L.stream_handle())

    un_ms = device_ms(un, reps_for(device_ms(un, 1)))
    rec.update({"baseline_iters": baseline_iters, "baseline_per_permutation_ms": per,
                "baseline_call_ms": per * P, "baseline_un_device_ms": un_ms,
                "baseline_device_ms": un_ms * P, "ratio_call": per * P / rec["call_ms"],
                "ratio_device": un_ms * P / t})
    # the observed column against the existing kernel's sums of the same split
    a, b = out.cpu().numpy()[0], o2.cpu().numpy()[0]
    rec["observed_matches_un"] = bool(np.all(np.abs(a - b) <= 1e-12 * a.sum()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_mmd_perm.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    ap.add_argument("--lib", default=None, help="a variant build of libtuplewise.so to time")
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = pathlib.Path(args.lib).resolve()
    import tuplewise.mmd as mm
    assert torch.cuda.is_available(), "time_mmd_perm.py needs a HIP device"
    big = 1000 if args.quick else 10_000
    res = {"device": torch.cuda.get_device_name(0), "lib": str(L.LIB_PATH.name),
           "cols_per_pass": int(L.lib().tw_mmd_perm_cols()), "tile": int(L.lib().tw_mmd_tile()),
           "mfma_f64_macs_per_s": MFMA_F64_MACS, "f64_valu_lane_ops_per_s": F64_VALU_LANE_OPS,
           "shapes": []}
    for d in (2, 8, 64):
        for P in (100, 1000):
            for kernel in ("gaussian", "energy"):
                res["shapes"].append(shape(mm, big, big, d, P, kernel, 50))
                print(json.dumps(res["shapes"][-1]), flush=True)
    for kernel in ("gaussian", "energy"):
        res["shapes"].append(shape(mm, 500, 500, 8, 1000, kernel, 50))
        print(json.dumps(res["shapes"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
