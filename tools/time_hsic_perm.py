"""Device and call time of the HSIC / distance-covariance permutation test
(tuplewise.hsic_perm.permutation_test, csrc/hsic_perm.hip) beside the only way the package had
before it: one host permutation, one gather of Y and one hsic.Un call per permutation (GPU box).

Shapes: n = 1e4 at (dx, dy) in {(2, 2), (8, 8), (64, 64), (64, 2)} with P in {100, 1000}
permutations, both kernels, and one small shape (n = 500, d = 8, P = 1000).  Per shape:
  device_ms        tw_hsic_perm_sums on resident operands (P + 1 columns: the identity and the
                   permutations; row sums from one tw_hsic_sums call outside the window), the
                   median of 5 windows of back-to-back calls between two device events after one
                   warm call
  bound_ms         pairs * [(P + 1) * ops_moved + ceil((P + 1) / C) * ops_held] lane-ops at the
                   float64 VALU rate (3.93e13 lane-ops/s), ops counted from the kernel's gfx950
                   assembly (a float64 instruction one, any other VALU half)
  share_of_bound   bound_ms / device_ms
  call_ms          the whole permutation_test call (draws, upload, both launches, read-back), host
                   clock, median of 3; draws_ms the P np.random.permutation calls alone
  baseline_*       per permutation: np.random.permutation, Y[pi] and hsic.Un (upload, launch,
                   read-back), `baseline_iters` iterations timed on the host clock and scaled to P
                   (baseline_call_ms); baseline_device_ms is tw_hsic_sums on resident operands
                   times P + 1
  ratio_call, ratio_device   baseline over this module

Usage: time_hsic_perm.py [--out profiles/time_hsic_perm.json] [--quick] [--lib variant.so]"""
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
PER_COORD = 3.0 + 0.5 * 17 / 128  # a chunk: 384 float64 + 17 other VALU per 8 coordinates x 16 pairs
# lane-ops per pair of one side's g and fold: (moved, held)
FOLD = {"gaussian": (22.5, 26.5), "distance": (18.0, 16.5)}


def ops(d, kernel, held):
    return PER_COORD * d + FOLD[kernel][1 if held else 0]


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


def shape(hs, hp, n, dx, dy, P, kernel, baseline_iters):
    rng = np.random.RandomState(dx + dy + P)
    X = rng.normal(size=(n, dx))
    Y = X @ rng.normal(size=(dx, dy)) / math.sqrt(dx) + 0.5 * rng.normal(size=(n, dy))
    sigma = (math.sqrt(dx), math.sqrt(dy)) if kernel == "gaussian" else None
    kid, cx, cy = hs._coef(kernel, sigma)
    cols, C = P + 1, int(L.lib().tw_hsic_perm_cols())
    perms = np.stack([np.arange(n)] + [rng.permutation(n) for _ in range(P)]).astype(np.int32)
    # the unpermuted sample's sums and row sums: the baseline's kernel, also timed below
    xd, yd = L.to_device(X.reshape(-1)), L.to_device(Y.reshape(-1))
    od = L.to_device(np.array([0, n], dtype=np.int64))
    w1 = L.empty((int(L.lib().tw_hsic_work_bytes(1, n, 0)) // 8,), torch.float64)
    o1, rows = L.empty((1, 8), torch.float64), L.empty((n, 2), torch.float64)

    def un():
        L.call("tw_hsic_sums", xd, dx, yd, dy, od, 1, n, kid, cx, cy, 0, w1, rows, o1,
               L.stream_handle())

    un()
    rt = rows.t().contiguous()
    move_y = dy <= dx  # the host's rule (tuplewise.hsic_perm._perm_sums)
    if move_y:
        idx, args = perms, (xd, dx, yd, dy, n)
        tail = (rt[0], rt[1], kid, cx, cy)
    else:
        idx = np.empty_like(perms)
        idx[np.arange(cols)[:, None], perms] = np.arange(n, dtype=np.int32)
        args, tail = (yd, dy, xd, dx, n), (rt[1], rt[0], kid, cy, cx)
    idd = L.to_device(idx.reshape(-1))
    work = L.empty((int(L.lib().tw_hsic_perm_work_bytes(n, cols, 0)) // 8,), torch.float64)
    out = L.empty((cols, 2), torch.float64)

    def go():
        L.call("tw_hsic_perm_sums", *args, idd, cols, *tail, 0, work, out, L.stream_handle())

    t = device_ms(go, reps_for(device_ms(go, 1)))
    pairs = n * (n - 1) // 2
    d_m, d_h = (dy, dx) if move_y else (dx, dy)
    lane_ops = pairs * (cols * ops(d_m, kernel, False) + -(-cols // C) * ops(d_h, kernel, True))
    bound = lane_ops / F64_VALU_LANE_OPS * 1e3
    rec = {"n": n, "dx": dx, "dy": dy, "P": P, "kernel": kernel, "pairs": pairs,
           "moved": "y" if move_y else "x", "device_ms": t, "bound_ms": bound,
           "ops_moved": ops(d_m, kernel, False), "ops_held": ops(d_h, kernel, True),
           "share_of_bound": bound / t, "pair_columns_per_s": pairs * cols / (t * 1e-3)}

    # the whole call, and its host draws alone
    def call():
        np.random.seed(1)
        return hp.permutation_test(X, Y, P, kernel, sigma)

    def draws():
        np.random.seed(1)
        pm = np.empty((P + 1, n), dtype=np.int32)
        for p in range(1, P + 1):
            pm[p] = np.random.permutation(n)
        return pm

    res = call()
    rec["call_ms"] = host_ms(call)
    rec["draws_ms"] = host_ms(draws)
    rec["pvalue"] = res.pvalue

    # the baseline: one host permutation, one gather and one hs.Un per permutation
    def one():
        return hs.Un(X, Y[np.random.permutation(n)], kernel, sigma)

    one()
    t0 = time.perf_counter()
    for _ in range(baseline_iters):
        one()
    per = (time.perf_counter() - t0) * 1e3 / baseline_iters
    un_ms = device_ms(un, reps_for(device_ms(un, 1)))
    rec.update({"baseline_iters": baseline_iters, "baseline_per_permutation_ms": per,
                "baseline_call_ms": per * P, "baseline_un_device_ms": un_ms,
                "baseline_device_ms": un_ms * cols, "ratio_call": per * P / rec["call_ms"],
                "ratio_device": un_ms * cols / t})
    # the identity column against the existing kernel's sums
    a, b = out.cpu().numpy()[0], o1.cpu().numpy()[0]
    rec["observed_matches_un"] = bool(abs(a[0] - b[0]) <= 1e-12 * b[0]
                                      and abs(a[1] - b[5]) <= 1e-12 * b[5])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_hsic_perm.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    ap.add_argument("--lib", default=None, help="a variant build of libtuplewise.so to time")
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = pathlib.Path(args.lib).resolve()
    import tuplewise.hsic as hs
    import tuplewise.hsic_perm as hp
    assert torch.cuda.is_available(), "time_hsic_perm.py needs a HIP device"
    big = 1000 if args.quick else 10_000
    res = {"device": torch.cuda.get_device_name(0), "lib": str(L.LIB_PATH.name),
           "cols_per_chunk": int(L.lib().tw_hsic_perm_cols()), "tile": int(L.lib().tw_hsic_tile()),
           "f64_valu_lane_ops_per_s": F64_VALU_LANE_OPS, "per_coordinate_lane_ops": PER_COORD,
           "fold_lane_ops_moved_held": FOLD, "shapes": []}
    for dx, dy in ((2, 2), (8, 8), (64, 64), (64, 2)):
        for P in (100, 1000):
            for kernel in ("gaussian", "distance"):
                res["shapes"].append(shape(hs, hp, big, dx, dy, P, kernel, 50))
                print(json.dumps(res["shapes"][-1]), flush=True)
    for kernel in ("gaussian", "distance"):
        res["shapes"].append(shape(hs, hp, 500, 8, 8, 1000, kernel, 50))
        print(json.dumps(res["shapes"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
