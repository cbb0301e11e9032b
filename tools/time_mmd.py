"""Device time of the kernel two-sample U-statistics (tuplewise.mmd, csrc/mmd.hip) beside a
chunked NumPy restatement on one core (GPU box).

Shapes: Un at n = m = 1e4 for d in {2, 8, 64} and both kernels; the 64 blocks of one UnN on
n = m = 1e5 at d = 8 (blocks of 1562 rows); the 64 blocks of one UnNB on the same partition with
B = 1e6 quadruples per block.  For the comparison DESIGN.md §4.12 makes, tw_triplet_rows (the
row-writing kernel the micro-tile comes from) is timed on the Un shapes at d = 8 and d = 64.

Every device time is the median of 5 windows after one warm call, each window `reps`
back-to-back calls of the entry point between two device events, per call in ms; the operands are
resident, so uploads, the host's shuffles and draws and the read-back are outside the windows.  A
pair is one evaluation of g: n (n - 1) / 2 + m (m - 1) / 2 + n m per block for the complete
statistic, four per quadruple for the incomplete one.  `share_of_f64_valu` is pairs/s times the
lane-ops of one pair over the float64 VALU rate 3.93e13 lane-ops/s (256 CUs x 4 SIMDs x 16 lanes
x 2.4 GHz); the lane-ops per pair are read from the gfx950 assembly of the inner loops (DESIGN.md
§4.12): three float64 instructions per coordinate (and 16 register moves per chunk of 256
pair-coordinates), then g and its add — a float64 instruction is
one lane-op, any other VALU instruction half of one (it issues at twice the rate).  The whole
calls (upload, launches, read-back) are host-clock medians of 3.

The NumPy restatement computes the same sums in row chunks (distances coordinate by coordinate as
the oracle of tests/test_triplets_cpu.py does, np.exp / np.sqrt, np.sum per chunk).  Where its
full run would take minutes it is timed on `numpy_pairs` pairs and scaled to all of them
(`numpy_note` says so); where it runs in full its sums are compared with the device's at rtol
1e-12 (`matches_numpy`).

Usage: time_mmd.py [--out profiles/time_mmd.json] [--quick]"""
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

import tuplewise.mmd as mm  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

F64_VALU_LANE_OPS = 3.93e13  # lane-ops/s
# g and its add per pair in the unmasked fold of k_mmd_sums (gfx950 assembly):
# (float64 VALU instructions, other VALU instructions)
FOLD = {"gaussian": (673 / 32, 98 / 32), "energy": (481 / 32, 129 / 32)}
CHUNK_MOVES = 16 / 256  # register moves of the prefetched chunk per pair-coordinate (768 + 16 per chunk)
NUMPY_FULL_PAIR_COORDS = 2.0e9  # the restatement runs in full below this many pair-coordinates


def lane_ops(d, kernel):
    f64, other = FOLD[kernel]
    return (3.0 + 0.5 * CHUNK_MOVES) * d + f64 + 0.5 * other


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


def make(n, m, d, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(m, d))


def pairs_of(n, m):
    return n * (n - 1) // 2 + m * (m - 1) // 2 + n * m


# ------------------------------------------------------------------------ NumPy restatement
def np_dist(A, B):
    acc = np.zeros((A.shape[0], B.shape[0]))
    for c in range(A.shape[1]):
        t = A[:, None, c] - B[None, :, c]
        acc = acc + t * t
    return acc


def np_g(D, kernel, c):
    return np.exp(D * c) if kernel == "gaussian" else np.sqrt(D)


def np_components(X, Z, kernel, c, budget_pairs, chunk=32):
    """(Sxx, Szz, Sxz), the pairs done and the seconds taken; with a budget (not None) a
    component's row chunks stop once a third of budget_pairs is done."""
    sums, done = [], 0
    t0 = time.perf_counter()
    for A, B, tri in ((X, X, True), (Z, Z, True), (X, Z, False)):
        s, part = 0.0, 0
        for a in range(0, A.shape[0], chunk):
            rows = A[a:a + chunk]
            G = np_g(np_dist(rows, B[a:] if tri else B), kernel, c)
            s += float(np.sum(np.triu(G, 1) if tri else G))
            part += G.size - (len(rows) * (len(rows) + 1) // 2 if tri else 0)
            if budget_pairs is not None and part * 3 >= budget_pairs:
                break
        sums.append(s)
        done += part
    return sums, done, time.perf_counter() - t0


def np_quadruples(X, Z, i, j, k, l, kernel, c):  # noqa: E741
    def dist(A, B):
        acc = np.zeros(A.shape[0])
        for col in range(A.shape[1]):
            t = A[:, col] - B[:, col]
            acc = acc + t * t
        return acc
    return [float(np.sum(np_g(dist(A, B), kernel, c)))
            for A, B in ((X[i], X[j]), (Z[k], Z[l]), (X[i], Z[l]), (X[j], Z[k]))]


def close(got, want):
    return bool(np.allclose(got, want, rtol=1e-12, atol=0.0))


# ----------------------------------------------------------------------------------- shapes
def complete(X, Z, N, kernel, full_numpy):
    """One complete statistic on N equal blocks (N = 1: Un on the whole samples)."""
    d = X.shape[1]
    sigma = math.sqrt(d) if kernel == "gaussian" else None
    kid, c = mm._coef(kernel, sigma)
    k, kz = X.shape[0] // N, Z.shape[0] // N
    Xu, Zu = X[:N * k], Z[:N * kz]
    xd, zd = L.to_device(Xu.reshape(-1)), L.to_device(Zu.reshape(-1))
    bx = L.to_device(np.arange(N + 1, dtype=np.int64) * k)
    bz = L.to_device(np.arange(N + 1, dtype=np.int64) * kz)
    work = L.empty((int(L.lib().tw_mmd_work_bytes(N, k, kz)) // 8,), torch.float64)
    out = L.empty((N, 3), torch.float64)

    def go():
        L.call("tw_mmd_sums", xd, zd, d, bx, bz, N, k, kz, kid, c, work, out, L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    pairs = N * pairs_of(k, kz)
    rate = pairs / (t * 1e-3)
    rec = {"n": X.shape[0], "m": Z.shape[0], "d": d, "N": N, "block": [k, kz], "kernel": kernel,
           "pairs": pairs, "reps": reps, "device_ms": t, "pairs_per_s": rate,
           "lane_ops_per_pair": lane_ops(d, kernel),
           "share_of_f64_valu": rate * lane_ops(d, kernel) / F64_VALU_LANE_OPS}
    if N == 1:
        rec["call_ms"] = host_ms(lambda: mm.Un(X, Z, kernel, sigma))
    else:
        rec["call_ms"] = host_ms(lambda: mm._Complete(kernel, sigma).evaluate(Xu, Zu, k, kz, N))
    block_pairs = pairs_of(k, kz)
    budget = None if full_numpy else int(NUMPY_FULL_PAIR_COORDS / 8 / d)
    sums, done, secs = np_components(Xu[:k], Zu[:kz], kernel, c, budget)
    rec["numpy_pairs"] = done
    rec["numpy_ms"] = secs * 1e3 * pairs / done
    rec["numpy_note"] = "one core" + ("" if done == pairs else
                                      f"; {done} pairs of one block timed, scaled to {pairs}")
    if done == block_pairs:
        rec["matches_numpy"] = close(out.cpu().numpy()[0], sums)
    rec["speedup_over_numpy"] = rec["numpy_ms"] / t
    return rec


def incomplete(X, Z, N, B, kernel, seed):
    """The N blocks of one UnNB: one tw_mmd_idx32 launch of N x B quadruples."""
    d = X.shape[1]
    sigma = math.sqrt(d) if kernel == "gaussian" else None
    kid, c = mm._coef(kernel, sigma)
    k, kz = X.shape[0] // N, Z.shape[0] // N
    Xu, Zu = X[:N * k], Z[:N * kz]
    rng = np.random.RandomState(seed)
    ii, kk = rng.randint(0, k, size=(N, B)), rng.randint(0, kz, size=(N, B))
    jj, ll = rng.randint(0, k - 1, size=(N, B)), rng.randint(0, kz - 1, size=(N, B))
    jj += jj >= ii
    ll += ll >= kk
    ii, jj = ii + (np.arange(N) * k)[:, None], jj + (np.arange(N) * k)[:, None]
    kk, ll = kk + (np.arange(N) * kz)[:, None], ll + (np.arange(N) * kz)[:, None]
    xd, zd = L.to_device(Xu.reshape(-1)), L.to_device(Zu.reshape(-1))
    id_, jd, kd, ld = (L.to_device(a.reshape(-1).astype(np.int32)) for a in (ii, jj, kk, ll))
    od = L.to_device(np.arange(N + 1, dtype=np.int64) * B)
    work = L.empty((int(L.lib().tw_mmd_idx_work_bytes(N, B)) // 8,), torch.float64)
    out = L.empty((N, 4), torch.float64)

    def go():
        L.call("tw_mmd_idx32", xd, zd, d, id_, jd, kd, ld, od, N, B, kid, c, work, out,
               L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    pairs = 4 * N * B
    rate = pairs / (t * 1e-3)
    rec = {"n": X.shape[0], "m": Z.shape[0], "d": d, "N": N, "block": [k, kz], "B": B,
           "kernel": kernel, "quadruples": N * B, "pairs": pairs, "reps": reps, "device_ms": t,
           "pairs_per_s": rate, "lane_ops_per_pair": lane_ops(d, kernel),
           "share_of_f64_valu": rate * lane_ops(d, kernel) / F64_VALU_LANE_OPS,
           # two rows of d doubles per pair and four int32 indices per quadruple
           "gathered_bytes_per_s": N * B * (8 * 8 * d + 16) / (t * 1e-3),
           "call_ms": host_ms(lambda: mm._sums_indexed(
               Xu, Zu, ii.reshape(-1), jj.reshape(-1), kk.reshape(-1), ll.reshape(-1),
               np.arange(N + 1) * B, kid, c))}
    t0 = time.perf_counter()
    want = np_quadruples(Xu, Zu, ii[0], jj[0], kk[0], ll[0], kernel, c)
    rec["numpy_ms"] = (time.perf_counter() - t0) * 1e3 * N
    rec["numpy_note"] = f"one core; one block timed, times {N}"
    rec["matches_numpy"] = close(out.cpu().numpy()[0], want)
    rec["speedup_over_numpy"] = rec["numpy_ms"] / t
    return rec


def triplet_rows(X, Z):
    """tw_triplet_rows on one block: every anchor's two rows of distances, written to HBM."""
    n, m, d = X.shape[0], Z.shape[0], X.shape[1]
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    bx, bz = L.to_device(np.array([0, n], dtype=np.int64)), L.to_device(np.array([0, m], dtype=np.int64))
    oo = L.to_device(np.arange(n + 1, dtype=np.int64) * m)
    wo = L.to_device(np.arange(n + 1, dtype=np.int64) * (n - 1))
    other, own = L.empty((n * m,), torch.float64), L.empty((n * (n - 1),), torch.float64)

    def go():
        L.call("tw_triplet_rows", xd, zd, d, bx, bz, 0, 1, 0, n, n, m, oo, wo, other, own,
               L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    pairs = n * (m + n - 1)
    rate = pairs / (t * 1e-3)
    return {"n": n, "m": m, "d": d, "pairs": pairs, "reps": reps, "device_ms": t,
            "pairs_per_s": rate, "lane_ops_per_pair": 3.0 * d,
            "share_of_f64_valu": rate * 3.0 * d / F64_VALU_LANE_OPS,
            "written_bytes_per_s": 8 * pairs / (t * 1e-3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_mmd.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mmd.py needs a HIP device"
    n_un = 1000 if args.quick else 10_000
    rows_per_class, N, B = (6400, 8, 1000) if args.quick else (100_000, 64, 1_000_000)
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_mmd_tile()),
           "f64_valu_lane_ops_per_s": F64_VALU_LANE_OPS, "Un": [], "UnN": [], "UnNB": [],
           "triplet_rows": []}
    for d in (2, 8, 64):
        X, Z = make(n_un, n_un, d, d)
        for kernel in ("gaussian", "energy"):
            full = pairs_of(n_un, n_un) * d <= NUMPY_FULL_PAIR_COORDS
            res["Un"].append(complete(X, Z, 1, kernel, full))
            print(json.dumps(res["Un"][-1]), flush=True)
        if d >= 8:
            res["triplet_rows"].append(triplet_rows(X, Z))
            print(json.dumps(res["triplet_rows"][-1]), flush=True)
    X, Z = make(rows_per_class, rows_per_class, 8, 8)
    for kernel in ("gaussian", "energy"):
        res["UnN"].append(complete(X, Z, N, kernel, True))
        print(json.dumps(res["UnN"][-1]), flush=True)
        res["UnNB"].append(incomplete(X, Z, N, B, kernel, 8))
        print(json.dumps(res["UnNB"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
