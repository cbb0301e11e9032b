"""Device time of the triplet U-statistics (tuplewise.triplets, csrc/triplets.hip) beside the
NumPy oracle of tests/test_triplets_cpu.py on one core (GPU box).

Shapes: Un at n = m in {500, 2000, 8000}, d = 8, with the pair count's "pairs" and "sorted"
algorithms; the blocks of UnN at 1e5 rows per class, N = 64 (blocks of 1562 rows), d in {8, 64};
the blocks of UnNB on the same partition with B = 1e5 triplets per block.

Every device time is the median of 5 windows after one warm call, each window `reps`
back-to-back passes between two device events, per pass in ms; the operands are resident, so
uploads, the host's shuffles and draws and the read-back are outside the windows.  A pass of a
complete statistic is every batch's tw_triplet_rows launch and count launch in the module's own
order; the rows alone and the counts alone (on the last batch's rows) give the split.  The rows
kernel's rate is the bytes it writes (8 per distance) over its time, beside the HBM rate the
microarchitecture guide gives as achievable (6.3e12 B/s of 8e12 peak).  The whole calls (upload,
launches, read-back) are host-clock medians of 3.  The oracle runs once per shape it can finish
(its (n, n) distance matrices are held whole: n <= 2000, and one block of the UnN shapes times
N).

Usage: time_triplets.py [--out profiles/time_triplets.json] [--quick]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tuplewise.triplets as tr  # noqa: E402
from tuplewise import _lib as L  # noqa: E402
from test_triplets_cpu import o_UB_indices, o_Un  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # B/s


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


def make(n, m, d, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(n, d)), rng.normal(0.3, 1.0, size=(m, d))


def reps_for(ms_guess):
    """Windows of about 0.2 s."""
    return max(1, min(200, int(200 / max(ms_guess, 1e-3))))


def complete(X, Z, N, algo, oracle):
    """One complete statistic on N equal blocks (N = 1: Un on the whole samples)."""
    k, kz = X.shape[0] // N, Z.shape[0] // N
    Xu, Zu = X[:N * k], Z[:N * kz]
    bat = tr._Batches(Xu, Zu, np.arange(N + 1) * k, np.arange(N + 1) * kz, "gt", algo)
    nq = len(bat.edges)
    triplets = N * k * (k - 1) * kz

    def rows():
        for q in range(nq):
            bat.rows(q)

    def counts():
        for q in range(nq):
            bat.count(q)

    def both():
        for q in range(nq):
            bat.rows(q)
            bat.count(q)

    probe = device_ms(both, 1)
    reps = reps_for(probe)
    t_both, t_rows, t_counts = device_ms(both, reps), device_ms(rows, reps), device_ms(counts, reps)
    written = 8 * sum(bat.row_elems)
    rec = {"n": X.shape[0], "m": Z.shape[0], "d": X.shape[1], "N": N, "block": [k, kz],
           "algo": bat.algo, "batches": nq, "triplets": triplets, "reps": reps,
           "device_ms": t_both, "triplets_per_s": triplets / (t_both * 1e-3),
           "rows_ms": t_rows, "count_ms": t_counts,
           "rows_share": t_rows / (t_rows + t_counts),
           "rows_bytes_written": written,
           "rows_written_bytes_per_s": written / (t_rows * 1e-3),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "rows_share_of_hbm": written / (t_rows * 1e-3) / HBM_ACHIEVABLE}
    if N == 1:
        rec["call_ms"] = host_ms(lambda: tr.Un(X, Z, algo=algo))
    else:
        rec["call_ms"] = host_ms(lambda: tr._Complete("gt", algo).evaluate(Xu, Zu, k, kz, N))
    if oracle:
        t0 = time.perf_counter()
        want = o_Un(Xu[:k], Zu[:kz])
        one = (time.perf_counter() - t0) * 1e3
        rec["oracle_ms"] = one * N
        rec["oracle_note"] = "one core" + ("" if N == 1 else f"; one block timed, times {N}")
        got = tr.Un(Xu[:k], Zu[:kz], algo=algo)
        rec["equals_oracle"] = bool(got == want)
    return rec


def incomplete(X, Z, N, B, seed):
    """The N blocks of one UnNB: one tw_triplet_idx32 launch of N x B triplets."""
    k, kz = X.shape[0] // N, Z.shape[0] // N
    Xu, Zu = X[:N * k], Z[:N * kz]
    rng = np.random.RandomState(seed)
    ii = rng.randint(0, k, size=(N, B))
    jj = rng.randint(0, k - 1, size=(N, B))
    jj += jj >= ii
    kk = rng.randint(0, kz, size=(N, B))
    ii, jj = ii + (np.arange(N) * k)[:, None], jj + (np.arange(N) * k)[:, None]
    kk = kk + (np.arange(N) * kz)[:, None]
    xd, zd = L.to_device(Xu.reshape(-1)), L.to_device(Zu.reshape(-1))
    id_, jd, kd = (L.to_device(a.reshape(-1).astype(np.int32)) for a in (ii, jj, kk))
    od = L.to_device(np.arange(N + 1, dtype=np.int64) * B)
    work = L.empty((L.lib().tw_triplet_idx_work_bytes(N, B) // 8,), torch.int64)
    out = L.empty((N,), torch.int64)

    def go():
        L.call("tw_triplet_idx32", xd, zd, X.shape[1], id_, jd, kd, od, N, B, L.TW_PRED_GT, work,
               out, L.stream_handle())

    reps = reps_for(device_ms(go, 1))
    t = device_ms(go, reps)
    d = X.shape[1]
    rec = {"n": X.shape[0], "m": Z.shape[0], "d": d, "N": N, "block": [k, kz], "B": B,
           "triplets": N * B, "reps": reps, "device_ms": t,
           "triplets_per_s": N * B / (t * 1e-3),
           # three rows of d doubles and three int32 indices per triplet
           "gathered_bytes_per_s": N * B * (3 * 8 * d + 12) / (t * 1e-3),
           "call_ms": host_ms(lambda: tr._count_indexed(
               Xu, Zu, ii.reshape(-1), jj.reshape(-1), kk.reshape(-1), np.arange(N + 1) * B, "gt"))}
    t0 = time.perf_counter()
    want = [o_UB_indices(Xu, Zu, ii[b], jj[b], kk[b], "gt") for b in range(N)]
    rec["oracle_ms"] = (time.perf_counter() - t0) * 1e3
    rec["oracle_note"] = "one core"
    got = out.cpu().numpy().view(np.uint64)
    rec["equals_oracle"] = bool(all(np.float64(int(g) / B) == w for g, w in zip(got, want)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_triplets.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_triplets.py needs a HIP device"
    sizes = [200, 600] if args.quick else [500, 2000, 8000]
    rows_per_class, N, B = (6400, 8, 1000) if args.quick else (100_000, 64, 100_000)
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_triplet_rows_tile()),
           "rows_bytes_cap": tr.ROWS_BYTES, "sorted_min_pairs": tr.E.SORTED_MIN_PAIRS,
           "Un": [], "UnN": [], "UnNB": []}
    for n in sizes:
        X, Z = make(n, n, 8, n)
        for algo in ("pairs", "sorted"):
            res["Un"].append(complete(X, Z, 1, algo, oracle=n <= 2000))
            print(json.dumps(res["Un"][-1]), flush=True)
    for d in (8, 64):
        X, Z = make(rows_per_class, rows_per_class, d, d)
        for algo in ("pairs", "sorted"):
            res["UnN"].append(complete(X, Z, N, algo, oracle=algo == "pairs"))
            print(json.dumps(res["UnN"][-1]), flush=True)
        res["UnNB"].append(incomplete(X, Z, N, B, d))
        print(json.dumps(res["UnNB"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
