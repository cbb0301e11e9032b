"""Device time of the kernel independence U-statistics (tuplewise.hsic, csrc/hsic.hip) beside
tw_mmd_sums (the bar of DESIGN.md §4.14) and a chunked NumPy restatement on one core (GPU box).

Shapes: Un at n = 1e4 for dx = dy in {2, 8, 64} and (dx, dy) = (64, 2), both kernels; the 64
blocks of one UnN on n = 1e5 at d = 8 (blocks of 1562 rows); the 64 blocks of one UnNB on the
same partition with B = 1e6 4-tuples per block.  In the same run tw_mmd_sums is timed at
n = m = 1e4 for d = 8 and d = 64: it evaluates about 2 n^2 pair functions where tw_hsic_sums
evaluates n^2, so the bar is t_hsic(n, d, d) <= 0.5 * t_mmd(d) * 1.25 (`bar`, per kernel and d).

Every device time is the median of 5 windows after one warm call, each window `reps` back-to-back
calls of the entry point between two device events, per call in ms; the operands are resident, so
uploads, the host's shuffle and draws and the read-back are outside the windows.  A pair is one
unordered (i, j): BOTH K_ij and L_ij, n (n - 1) / 2 per block; a 4-tuple of the incomplete
statistic is four pair functions.  `share_of_f64_valu` is pairs/s times the lane-ops of one pair
over the float64 VALU rate 3.93e13 lane-ops/s (256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).  The
lane-ops per pair are read from the gfx950 assembly of the unmasked inner loops (DESIGN.md
§4.14), a float64 instruction one lane-op and any other VALU instruction half of one: per side
and coordinate three float64 instructions (and 17 others per chunk of 128 pair-coordinates), then
per 16 pairs of a lane the two folds and the two reduce-scatter sums of the anchors' row sums.

The NumPy restatement computes the same eight sums in row chunks (distances coordinate by
coordinate, np.exp / np.sqrt, np.sum per chunk; the row sums accumulated per chunk).  Where its
full run would take long it is timed on `numpy_pairs` pairs and scaled to all of them
(`numpy_note` says so); where it runs in full its sums are compared with the device's at rtol
1e-12 (`matches_numpy`).

Usage: time_hsic.py [--out profiles/time_hsic.json] [--quick]"""
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

import tuplewise.hsic as hs  # noqa: E402
import tuplewise.mmd as mm  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

F64_VALU_LANE_OPS = 3.93e13  # lane-ops/s
# per 16 pairs of a lane, unmasked (gfx950 assembly of k_hsic_sums): (float64 VALU, other VALU) of
# K's fold + L's fold, and of the two reduce-scatter sums
FOLD = {"gaussian": (361 + 394, 53 + 52), "distance": (280 + 312, 67 + 67)}
ANCHOR = {"gaussian": (9 + 13, 68 + 53), "distance": (9 + 13, 62 + 53)}
CHUNK = (384, 17)  # per chunk of 8 coordinates x 8 anchors x 2 points = 128 pair-coordinates
# tw_mmd_sums' own counts (tools/time_mmd.py): per pair function
MMD_FOLD = {"gaussian": (673 / 32, 98 / 32), "energy": (481 / 32, 129 / 32)}
NUMPY_PAIR_COORDS = 4.0e8  # the restatement stops after this many pair-coordinates


def lane_ops(dx, dy, kernel):
    per_coord = (CHUNK[0] + 0.5 * CHUNK[1]) / 128
    return (per_coord * (dx + dy) + (FOLD[kernel][0] + 0.5 * FOLD[kernel][1]) / 16
            + (ANCHOR[kernel][0] + 0.5 * ANCHOR[kernel][1]) / 16)


def mmd_lane_ops(d, kernel):
    f64, other = MMD_FOLD[kernel]
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
    """Windows of about 0.2 s."""
    return max(1, min(200, int(200 / max(ms_guess, 1e-3))))


def make(n, dx, dy, seed):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, dx))
    Y = X @ rng.normal(size=(dx, dy)) / math.sqrt(dx) + 0.5 * rng.normal(size=(n, dy))
    return X, np.ascontiguousarray(Y)


def sigmas(kernel, dx, dy):
    return (math.sqrt(dx), math.sqrt(dy)) if kernel == "gaussian" else None


# ------------------------------------------------------------------------ NumPy restatement
def np_dist(A, B):
    acc = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        t = A[:, None, c] - B[None, :, c]
        acc = acc + t * t
    return acc


def np_g(D, kernel, c):
    return np.exp(D * c) if kernel == "gaussian" else np.sqrt(D)


def np_components(X, Y, kernel, cx, cy, budget_pairs, chunk=32):
    """The eight sums, the pairs done and the seconds taken: row chunks against the rows at or
    after them (each unordered pair once), stopping once budget_pairs are done (not None)."""
    n = X.shape[0]
    s = np.zeros(3)
    k, l = np.zeros(n), np.zeros(n)  # noqa: E741
    done = 0
    t0 = time.perf_counter()
    for a in range(0, n, chunk):
        K = np.triu(np_g(np_dist(X[a:a + chunk], X[a:]), kernel, cx), 1)
        Lm = np.triu(np_g(np_dist(Y[a:a + chunk], Y[a:]), kernel, cy), 1)
        s += (np.sum(K * Lm), np.sum(K * K), np.sum(Lm * Lm))
        k[a:a + chunk] += K.sum(axis=1)
        l[a:a + chunk] += Lm.sum(axis=1)
        k[a:] += K.sum(axis=0)
        l[a:] += Lm.sum(axis=0)
        rows = K.shape[0]
        done += K.size - rows * (rows + 1) // 2
        if budget_pairs is not None and done >= budget_pairs:
            break
    sums = list(s) + [k.sum(), l.sum(), (k * l).sum(), (k * k).sum(), (l * l).sum()]
    return sums, done, time.perf_counter() - t0


def np_tuples(X, Y, i, j, q, r, kernel, cx, cy):
    def dist(A, B):
        acc = np.zeros(A.shape[0])
        for col in range(A.shape[1]):
            t = A[:, col] - B[:, col]
            acc = acc + t * t
        return acc
    kij = np_g(dist(X[i], X[j]), kernel, cx)
    return [float(np.sum(kij * np_g(dist(Y[a], Y[b]), kernel, cy)))
            for a, b in ((i, j), (q, r), (i, q))]


def close(got, want):
    return bool(np.allclose(got, want, rtol=1e-12, atol=0.0))


# ----------------------------------------------------------------------------------- shapes
def complete(X, Y, N, kernel):
    """One complete statistic on N equal blocks (N = 1: Un on the whole sample)."""
    dx, dy = X.shape[1], Y.shape[1]
    sg = sigmas(kernel, dx, dy)
    kid, cx, cy = hs._coef(kernel, sg)
    k = X.shape[0] // N
    Xu, Yu = X[:N * k], Y[:N * k]
    xd, yd = L.to_device(Xu.reshape(-1)), L.to_device(Yu.reshape(-1))
    od = L.to_device(np.arange(N + 1, dtype=np.int64) * k)
    nbytes = int(L.lib().tw_hsic_work_bytes(N, k, 0))
    group = next(g for g in range(1, 9) if int(L.lib().tw_hsic_work_bytes(N, k, g)) == nbytes)
    work = L.empty((nbytes // 8,), torch.float64)
    out = L.empty((N, 8), torch.float64)
    rows = L.empty((N * k, 2), torch.float64)

    def go():
        L.call("tw_hsic_sums", xd, dx, yd, dy, od, N, k, kid, cx, cy, 0, work, rows, out,
               L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    pairs = N * (k * (k - 1) // 2)
    rate = pairs / (t * 1e-3)
    ops = lane_ops(dx, dy, kernel)
    rec = {"n": X.shape[0], "dx": dx, "dy": dy, "N": N, "block": k, "kernel": kernel,
           "group": group, "work_bytes": nbytes, "pairs": pairs, "reps": reps, "device_ms": t,
           "pairs_per_s": rate, "lane_ops_per_pair": ops,
           "share_of_f64_valu": rate * ops / F64_VALU_LANE_OPS}
    if N == 1:
        rec["call_ms"] = host_ms(lambda: hs.Un(X, Y, kernel, sg))
    else:
        rec["call_ms"] = host_ms(lambda: hs._Complete(kernel, sg).evaluate(Xu, Yu, k, N))
    block_pairs = k * (k - 1) // 2
    budget = int(NUMPY_PAIR_COORDS / (dx + dy))
    sums, done, secs = np_components(Xu[:k], Yu[:k], kernel, cx, cy,
                                     None if budget >= block_pairs else budget)
    rec["numpy_pairs"] = done
    rec["numpy_ms"] = secs * 1e3 * pairs / done
    rec["numpy_note"] = "one core" + ("" if done == pairs else
                                      f"; {done} pairs of one block timed, scaled to {pairs}")
    if done == block_pairs:
        rec["matches_numpy"] = close(out.cpu().numpy()[0], sums)
    rec["speedup_over_numpy"] = rec["numpy_ms"] / t
    return rec


def incomplete(X, Y, N, B, kernel, seed):
    """The N blocks of one UnNB: one tw_hsic_idx32 launch of N x B 4-tuples."""
    dx, dy = X.shape[1], Y.shape[1]
    sg = sigmas(kernel, dx, dy)
    kid, cx, cy = hs._coef(kernel, sg)
    k = X.shape[0] // N
    Xu, Yu = X[:N * k], Y[:N * k]
    rng = np.random.RandomState(seed)
    base = (np.arange(N) * k)[:, None]
    idx = [a.reshape(N, B) + base for a in hs._tuples_from(
        *(rng.randint(0, k - t, size=N * B) for t in range(4)))]
    xd, yd = L.to_device(Xu.reshape(-1)), L.to_device(Yu.reshape(-1))
    dev = [L.to_device(a.reshape(-1).astype(np.int32)) for a in idx]
    od = L.to_device(np.arange(N + 1, dtype=np.int64) * B)
    work = L.empty((int(L.lib().tw_hsic_idx_work_bytes(N, B)) // 8,), torch.float64)
    out = L.empty((N, 3), torch.float64)

    def go():
        L.call("tw_hsic_idx32", xd, dx, yd, dy, *dev, od, N, B, kid, cx, cy, work, out,
               L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    rec = {"n": X.shape[0], "dx": dx, "dy": dy, "N": N, "block": k, "B": B, "kernel": kernel,
           "tuples": N * B, "pair_functions": 4 * N * B, "reps": reps, "device_ms": t,
           "tuples_per_s": N * B / (t * 1e-3),
           # the rows of four pair functions and four int32 indices per 4-tuple
           "gathered_bytes_per_s": N * B * (8 * 2 * (dx + 3 * dy) + 16) / (t * 1e-3),
           "call_ms": host_ms(lambda: hs._sums_indexed(
               Xu, Yu, *(a.reshape(-1) for a in idx), np.arange(N + 1) * B, kid, cx, cy))}
    t0 = time.perf_counter()
    want = np_tuples(Xu, Yu, *(a[0] for a in idx), kernel, cx, cy)
    rec["numpy_ms"] = (time.perf_counter() - t0) * 1e3 * N
    rec["numpy_note"] = f"one core; one block timed, times {N}"
    rec["matches_numpy"] = close(out.cpu().numpy()[0], want)
    rec["speedup_over_numpy"] = rec["numpy_ms"] / t
    return rec


def mmd_sums(n, d, kernel, seed):
    """tw_mmd_sums (unchanged) at n = m: the yardstick of the bar."""
    rng = np.random.RandomState(seed)
    X, Z = rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(n, d))
    kid, c = mm._coef(kernel, math.sqrt(d) if kernel == "gaussian" else None)
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    bo = L.to_device(np.array([0, n], dtype=np.int64))
    work = L.empty((int(L.lib().tw_mmd_work_bytes(1, n, n)) // 8,), torch.float64)
    out = L.empty((1, 3), torch.float64)

    def go():
        L.call("tw_mmd_sums", xd, zd, d, bo, bo, 1, n, n, kid, c, work, out, L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    pairs = n * (n - 1) + n * n
    rate = pairs / (t * 1e-3)
    return {"n": n, "m": n, "d": d, "kernel": kernel, "pair_functions": pairs, "reps": reps,
            "device_ms": t, "lane_ops_per_pair_function": mmd_lane_ops(d, kernel),
            "share_of_f64_valu": rate * mmd_lane_ops(d, kernel) / F64_VALU_LANE_OPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_hsic.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hsic.py needs a HIP device"
    n_un = 1000 if args.quick else 10_000
    rows, N, B = (6400, 8, 1000) if args.quick else (100_000, 64, 1_000_000)
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_hsic_tile()),
           "f64_valu_lane_ops_per_s": F64_VALU_LANE_OPS, "Un": [], "UnN": [], "UnNB": [],
           "mmd_sums": [], "bar": []}
    for dx, dy in ((2, 2), (8, 8), (64, 64), (64, 2)):
        X, Y = make(n_un, dx, dy, dx + dy)
        for kernel in ("gaussian", "distance"):
            res["Un"].append(complete(X, Y, 1, kernel))
            print(json.dumps(res["Un"][-1]), flush=True)
    for d in (8, 64):
        for kernel, theirs in (("gaussian", "gaussian"), ("distance", "energy")):
            m = mmd_sums(n_un, d, theirs, d)
            res["mmd_sums"].append(m)
            print(json.dumps(m), flush=True)
            h = next(r for r in res["Un"] if (r["dx"], r["dy"], r["kernel"]) == (d, d, kernel))
            limit = 0.5 * m["device_ms"] * 1.25
            res["bar"].append({"d": d, "kernel": kernel, "hsic_ms": h["device_ms"],
                               "mmd_ms": m["device_ms"], "ratio": h["device_ms"] / m["device_ms"],
                               "limit_ms": limit, "met": bool(h["device_ms"] <= limit)})
            print(json.dumps(res["bar"][-1]), flush=True)
    X, Y = make(rows, 8, 8, 8)
    for kernel in ("gaussian", "distance"):
        res["UnN"].append(complete(X, Y, N, kernel))
        print(json.dumps(res["UnN"][-1]), flush=True)
        res["UnNB"].append(incomplete(X, Y, N, B, kernel, 8))
        print(json.dumps(res["UnNB"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
