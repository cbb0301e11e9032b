"""Device time of the HSIC row sums for a grid of bandwidth pairs (tuplewise.hsic_var,
csrc/hsic_rows.hip) beside tw_hsic_sums with d_rows on the same inputs in the same session, and a
chunked NumPy restatement on one core (GPU box).

Shapes: n = 1e4 paired Gaussian points (Y = X A + 0.5 noise) at dx = dy = d in {2, 8, 64}:
tw_hsic_sums with d_rows, tw_hsic_rows at S = 1 with weights (both kernels) and without, and at
S = max_sigma in one launch (Gaussian kernel, with weights); 64 blocks of 1562 at d = 8;
select_sigma end to end on a grid of 8 pairs at d = 8.

Every device time is the median of 5 windows after one warm call, each window `reps` back-to-back
calls of the entry point between two device events, per call in ms; the operands are resident.
tw_hsic_sums is timed before and after tw_hsic_rows (A B A) and the ratios use the mean of the
two.  The whole calls (upload, launches, read-back, host arithmetic) are host-clock medians of 3.

The bars, stated before the run:
  1  one weighted tw_hsic_rows launch at S = 1 <= 1.36 x tw_hsic_sums with d_rows (§4.14 measured
     5 % + 7 % for that kernel's two folded row sums; three cost 18 %; x 1.15)
  2  S = max_sigma pairs in one launch faster than max_sigma launches at S = 1, at d = 64; d = 8
     recorded; beside both the lane-op model (3 (dx + dy) + S G) / (S (3 (dx + dy) + G)), G = the
     two sides' g in lane-ops solved from tw_hsic_rows' own S = 1 times at d = 2 and d = 8:
     t(d) ~ 3 (2 d) + G.

The NumPy restatement computes the five row sums of one pair from distance chunks (distances
coordinate by coordinate, np.exp per side, np.sum per chunk; the weighted sums in a second pass
over the same chunks) on `numpy_rows` rows and is scaled to all rows.

Usage: time_hsic_var.py [--out profiles/time_hsic_var.json] [--quick]"""
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
import tuplewise.hsic_var as hv  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

BAR1 = 1.36


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


def timed(go):
    reps = max(1, min(200, int(200 / max(device_ms(go, 1), 1e-3))))  # windows of about 0.2 s
    return device_ms(go, reps), reps


def make(n, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, d))
    Y = X @ rng.normal(size=(d, d)) + 0.5 * rng.normal(size=(n, d))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def pairs_of(d, S):
    base = math.sqrt(d)
    if S == 1:
        return [(base, 1.5 * base)]
    return [(float(a), float(1.5 * a)) for a in base * np.geomspace(0.25, 4.0, S)]


class Resident:
    """One partition of N equal blocks on the device."""

    def __init__(self, X, Y, N):
        self.dx, self.dy, self.N = X.shape[1], Y.shape[1], N
        self.k = X.shape[0] // N
        self.xd = L.to_device(X[:N * self.k].reshape(-1))
        self.yd = L.to_device(Y[:N * self.k].reshape(-1))
        self.off = L.to_device(np.arange(N + 1, dtype=np.int64) * self.k)

    def sums(self, kernel):
        """tw_hsic_sums with d_rows."""
        kid, cx, cy = hs._coef(kernel, pairs_of(self.dx, 1)[0] if kernel == "gaussian" else None)
        work = L.empty((int(L.lib().tw_hsic_work_bytes(self.N, self.k, 0)) // 8,), torch.float64)
        out = L.empty((self.N, 8), torch.float64)
        rows = L.empty((self.N * self.k, 2), torch.float64)

        def go():
            L.call("tw_hsic_sums", self.xd, self.dx, self.yd, self.dy, self.off, self.N, self.k, kid,
                   cx, cy, 0, work, rows, out, L.stream_handle())
        t, reps = timed(go)
        return t, reps, out.cpu().numpy(), rows.cpu().numpy()

    def rows(self, kernel, S, weighted):
        """One tw_hsic_rows launch; weighted: the weights are a first launch's rows."""
        kid = hs._KERNELS[kernel]
        cs = ([hs._coef(kernel, s)[1:] for s in pairs_of(self.dx, S)] if kernel == "gaussian"
              else [(0.0, 0.0)])
        cd = L.to_device(np.asarray(cs, dtype=np.float64).reshape(-1))
        nbytes = int(L.lib().tw_hsic_rows_work_bytes(self.N, self.k, S))
        work = L.empty((nbytes // 8,), torch.float64)
        first = L.empty((S, self.N * self.k, 3), torch.float64)
        out = L.empty((S, self.N * self.k, 3), torch.float64)

        def launch(w, o):
            L.call("tw_hsic_rows", self.xd, self.dx, self.yd, self.dy, self.off, self.N, self.k, kid,
                   cd, S, w, work, o, L.stream_handle())
        launch(None, first)
        t, reps = timed(lambda: launch(first if weighted else None, out))
        return t, reps, nbytes, first.cpu().numpy(), out.cpu().numpy()


def np_rows(X, Y, cx, cy, rows, chunk=32):
    """(p, k, l, u, v) of the first `rows` rows for one pair; seconds per evaluated row.  The
    weighted sums need every k_j and l_j, so the first pass runs over ALL rows in chunks and only
    the second is cut to `rows`: the time of the first is scaled from its own `rows` rows."""
    n = X.shape[0]

    def chunk_KL(i0, m):
        out = []
        for A, c in ((X, cx), (Y, cy)):
            acc = np.zeros((m, n))
            for col in range(A.shape[1]):
                t = A[i0:i0 + m, None, col] - A[None, :, col]
                acc = acc + t * t
            G = np.exp(acc * c)
            G[np.arange(m), np.arange(i0, i0 + m)] = 0.0
            out.append(G)
        return out

    k, l = np.zeros(n), np.zeros(n)  # noqa: E741
    p = np.zeros(rows)
    t_first = 0.0
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        t0 = time.perf_counter()
        K, Lm = chunk_KL(i0, m)
        k[i0:i0 + m], l[i0:i0 + m] = K.sum(axis=1), Lm.sum(axis=1)
        if i0 < rows:
            p[i0:i0 + m] = (K * Lm).sum(axis=1)[:max(0, min(m, rows - i0))]
            t_first += time.perf_counter() - t0
    u, v = np.zeros(rows), np.zeros(rows)
    t0 = time.perf_counter()
    for i0 in range(0, rows, chunk):
        m = min(chunk, rows - i0)
        K, Lm = chunk_KL(i0, m)
        u[i0:i0 + m], v[i0:i0 + m] = K @ l, Lm @ k
    t_second = time.perf_counter() - t0
    return (p, k[:rows], l[:rows], u, v), (t_first + t_second) / rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_hsic_var.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_hsic_var.py needs a HIP device"
    n = 1024 if args.quick else 10_000
    blocks, total = (8, 8 * 200) if args.quick else (64, 100_000)
    S = int(L.lib().tw_hsic_rows_max_sigma())
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_hsic_tile()),
           "max_sigma": S, "bar1": BAR1, "shapes": []}
    rows_ms = {}
    for d in (2, 8, 64):
        X, Y = make(n, d, d)
        R = Resident(X, Y, 1)
        rec = {"n": n, "dx": d, "dy": d}
        for kernel in ("gaussian", "distance"):
            # A B A: tw_hsic_sums before and after tw_hsic_rows, so that a clock that drifts over
            # the session does not favour either; the ratio is taken against the mean of the two
            ta, reps, out, krows = R.sums(kernel)
            tw_, repsw, nbytes, first, second = R.rows(kernel, 1, True)
            tu, repsu, _, _, _ = R.rows(kernel, 1, False)
            tb, _, _, _ = R.sums(kernel)
            t = 0.5 * (ta + tb)
            rec[f"sums_{kernel}_ms"], rec[f"sums_{kernel}_reps"] = t, reps
            rec[f"sums_{kernel}_before_after_ms"] = [ta, tb]
            rec[f"rows_{kernel}_S1_weighted_ms"], rec[f"rows_{kernel}_S1_weighted_reps"] = tw_, repsw
            rec[f"rows_{kernel}_S1_unweighted_ms"] = tu
            rec[f"rows_{kernel}_S1_weighted_over_sums"] = tw_ / t
            rec[f"rows_{kernel}_S1_unweighted_over_sums"] = tu / t
            rec[f"rows_{kernel}_S1_work_bytes"] = nbytes
            rec[f"bar1_{kernel}_met"] = bool(tw_ / t <= BAR1)
            # the rows are the sums' (tw_hsic_sums on the same operands)
            rec[f"rows_{kernel}_match_sums"] = bool(
                np.allclose(first[0, :, 1:], krows, rtol=1e-11, atol=0)
                and np.allclose(first[0, :, 0].sum() / 2.0, out[0, 0], rtol=1e-11, atol=0)
                and np.allclose(second[0, :, 1].sum(), out[0, 5], rtol=1e-11, atol=0))
        rows_ms[d] = rec["rows_gaussian_S1_weighted_ms"]
        tS, repsS, nbytes, first, second = R.rows("gaussian", S, True)
        rec["rows_gaussian_Smax_weighted_ms"], rec["rows_gaussian_Smax_reps"] = tS, repsS
        rec["rows_gaussian_Smax_work_bytes"] = nbytes
        rec["rows_gaussian_Smax_over_Smax_launches"] = tS / (S * rows_ms[d])
        rec["Smax_faster_than_Smax_launches"] = bool(tS < S * rows_ms[d])
        if d == 8:  # one core for scale: 64 rows against everything, scaled
            _, cx, cy = hs._coef("gaussian", pairs_of(d, 1)[0])
            nrows = min(n, 64)
            got, per_row = np_rows(X, Y, cx, cy, nrows)
            R1 = R.rows("gaussian", 1, True)
            want = (R1[3][0, :nrows, 0], R1[3][0, :nrows, 1], R1[3][0, :nrows, 2],
                    R1[4][0, :nrows, 1], R1[4][0, :nrows, 2])
            rec["numpy_rows"] = nrows
            rec["numpy_five_sums_ms"] = per_row * n * 1e3
            rec["numpy_note"] = f"one core; {nrows} rows timed (both passes), scaled to n rows"
            rec["numpy_matches"] = bool(all(np.allclose(g, w, rtol=1e-11, atol=0)
                                            for g, w in zip(got, want)))
            rec["speedup_over_numpy_two_launches"] = rec["numpy_five_sums_ms"] / (
                rec["rows_gaussian_S1_weighted_ms"] + rec["rows_gaussian_S1_unweighted_ms"])
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    # the two sides' g in lane-ops from tw_hsic_rows' own S = 1 times: t(d) ~ 6 d + G at d = 2, 8
    t2, t8 = rows_ms[2], rows_ms[8]
    G = (48.0 * t2 - 12.0 * t8) / (t8 - t2)
    res["G_lane_ops"] = G
    for rec in res["shapes"]:
        d = rec["dx"]
        rec["model_Smax_over_Smax_launches"] = (6.0 * d + S * G) / (S * (6.0 * d + G))
    res["bar2_met"] = bool(res["shapes"][2]["Smax_faster_than_Smax_launches"])
    # 64 blocks of 1562
    X, Y = make(total, 8, 8)
    R = Resident(X, Y, blocks)
    t, reps, _, _ = R.sums("gaussian")
    t1, reps1, nbytes, _, _ = R.rows("gaussian", 1, True)
    _, cx, cy = hs._coef("gaussian", pairs_of(8, 1)[0])
    res["blocks"] = {"N": blocks, "block": R.k, "d": 8, "sums_ms": t, "rows_S1_weighted_ms": t1,
                     "rows_S1_weighted_over_sums": t1 / t, "reps": [reps, reps1],
                     "work_bytes": nbytes,
                     "call_ms": host_ms(lambda: hv._rows_blocks(
                         X[:blocks * R.k], Y[:blocks * R.k], np.arange(blocks + 1) * R.k, 0,
                         [(cx, cy)]))}
    print(json.dumps(res["blocks"]), flush=True)
    # Un_var and select_sigma end to end
    X, Y = make(n, 8, 8)
    grid = pairs_of(8, 8)
    sel = hv.select_sigma(X, Y, grid)
    res["select_sigma"] = {"n": n, "d": 8, "grid": len(grid), "index": sel.index,
                           "sigma": list(sel.sigma),
                           "criterion_max": float(sel.criterion[sel.index]),
                           "call_ms": host_ms(lambda: hv.select_sigma(X, Y, grid)),
                           "Un_var_call_ms": host_ms(lambda: hv.Un_var(X, Y, sigma=grid[4])),
                           "Un_call_ms": host_ms(lambda: hs.Un(X, Y, sigma=grid[4]))}
    print(json.dumps(res["select_sigma"]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
