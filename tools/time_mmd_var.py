"""Device time of the MMD row sums for a grid of bandwidths (tuplewise.mmd_var, csrc/mmd_rows.hip)
beside tw_mmd_sums on the same inputs in the same session, and a chunked NumPy restatement on one
core (GPU box).

Shapes: n = m = 1e4 Gaussian points at d in {2, 8, 64} (tools/time_mmd.py's inputs): tw_mmd_sums,
tw_mmd_rows at S = 1 and S = 8 (Gaussian kernel) and at S = 1 (energy kernel); 64 blocks of
1562 x 1562 at d = 8, S = 1; select_sigma end to end on a grid of 16 at d = 8.

Every device time is the median of 5 windows after one warm call, each window `reps` back-to-back
calls of the entry point between two device events, per call in ms; the operands are resident.
tw_mmd_sums is timed before and after tw_mmd_rows (A B A) and the ratios use the mean of the two.
The whole calls (upload, launches, read-back, host arithmetic) are host-clock medians of 3.

The bars, stated before the run:
  S = 1   tw_mmd_rows <= 1.15 x tw_mmd_sums (5 % the anchors' cross-lane sums, 7 % the row pass:
          §4.14's measured cost of what this kernel adds to k_mmd_sums)
  S = 8   tw_mmd_rows < 8 x tw_mmd_sums at d = 8 and d = 64, and against the lane-op model
          (3 d + 8 G) / (8 (3 d + G)) x 1.15, G = g's lane-ops solved from tw_mmd_sums' own times
          at d = 2 and d = 8 in this session: t(d) ~ 3 d + G.

The NumPy restatement computes the four row sums of S sigmas from one distance chunk (distances
coordinate by coordinate, np.exp per sigma, np.sum per chunk) on `numpy_rows` rows of X and is
scaled to all pairs.

Usage: time_mmd_var.py [--out profiles/time_mmd_var.json] [--quick]"""
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
import tuplewise.mmd_var as mv  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

MARGIN = 1.15


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


def timed(go):
    reps = reps_for(device_ms(go, 1))
    return device_ms(go, reps), reps


def make(n, m, d, seed):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(m, d))


def grid_of(d, S):
    return [math.sqrt(d)] if S == 1 else list(math.sqrt(d) * np.geomspace(0.25, 4.0, S))


class Resident:
    """One partition of N equal blocks on the device."""

    def __init__(self, X, Z, N):
        self.d, self.N = X.shape[1], N
        self.k, self.kz = X.shape[0] // N, Z.shape[0] // N
        self.xd = L.to_device(X[:N * self.k].reshape(-1))
        self.zd = L.to_device(Z[:N * self.kz].reshape(-1))
        self.bx = L.to_device(np.arange(N + 1, dtype=np.int64) * self.k)
        self.bz = L.to_device(np.arange(N + 1, dtype=np.int64) * self.kz)

    def sums(self, kernel):
        kid, c = mm._coef(kernel, math.sqrt(self.d) if kernel == "gaussian" else None)
        work = L.empty((int(L.lib().tw_mmd_work_bytes(self.N, self.k, self.kz)) // 8,), torch.float64)
        out = L.empty((self.N, 3), torch.float64)

        def go():
            L.call("tw_mmd_sums", self.xd, self.zd, self.d, self.bx, self.bz, self.N, self.k,
                   self.kz, kid, c, work, out, L.stream_handle())
        t, reps = timed(go)
        return t, reps, out.cpu().numpy()

    def rows(self, kernel, S):
        kid = mm._KERNELS[kernel]
        cs = [mm._coef(kernel, s)[1] for s in grid_of(self.d, S)] if kernel == "gaussian" else [0.0]
        cd = L.to_device(np.asarray(cs, dtype=np.float64))
        nbytes = int(L.lib().tw_mmd_rows_work_bytes(self.N, self.k, self.kz, S))
        work = L.empty((nbytes // 8,), torch.float64)
        rx = L.empty((S, self.N * self.k, 2), torch.float64)
        rz = L.empty((S, self.N * self.kz, 2), torch.float64)

        def go():
            L.call("tw_mmd_rows", self.xd, self.zd, self.d, self.bx, self.bz, self.N, self.k,
                   self.kz, kid, cd, S, work, rx, rz, L.stream_handle())
        t, reps = timed(go)
        return t, reps, nbytes, rx.cpu().numpy(), rz.cpu().numpy()


def np_rows(X, Z, cs, rows, chunk=32):
    """a and r of the first `rows` rows of X for every c of cs; seconds per evaluated pair."""
    t0 = time.perf_counter()
    a, r = np.zeros((len(cs), rows)), np.zeros((len(cs), rows))
    for i0 in range(0, rows, chunk):
        x = X[i0:i0 + chunk]
        for B, out, own in ((X, a, True), (Z, r, False)):
            acc = np.zeros((x.shape[0], B.shape[0]))
            for col in range(x.shape[1]):
                t = x[:, None, col] - B[None, :, col]
                acc = acc + t * t
            for s, c in enumerate(cs):
                G = np.exp(acc * c)
                if own:
                    G[np.arange(x.shape[0]), np.arange(i0, i0 + x.shape[0])] = 0.0
                out[s, i0:i0 + x.shape[0]] = G.sum(axis=1)
    secs = time.perf_counter() - t0
    return a, r, secs / (rows * (X.shape[0] + Z.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_mmd_var.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_mmd_var.py needs a HIP device"
    n = 1000 if args.quick else 10_000
    blocks, rows_per_class = (8, 6400) if args.quick else (64, 100_000)
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_mmd_tile()),
           "max_sigma": int(L.lib().tw_mmd_rows_max_sigma()), "margin": MARGIN, "shapes": []}
    sums_ms = {}
    for d in (2, 8, 64):
        X, Z = make(n, n, d, d)
        R = Resident(X, Z, 1)
        rec = {"n": n, "m": n, "d": d}
        for kernel in ("gaussian", "energy"):
            # A B A: tw_mmd_sums before and after tw_mmd_rows, so that a clock that drifts over
            # the session does not favour either; the ratio is taken against the mean of the two
            ta, reps, out = R.sums(kernel)
            t1, reps1, nbytes, rx, rz = R.rows(kernel, 1)
            tb, _, _ = R.sums(kernel)
            t = 0.5 * (ta + tb)
            rec[f"sums_{kernel}_ms"], rec[f"sums_{kernel}_reps"] = t, reps
            rec[f"sums_{kernel}_before_after_ms"] = [ta, tb]
            rec[f"rows_{kernel}_S1_ms"], rec[f"rows_{kernel}_S1_reps"] = t1, reps1
            rec[f"rows_{kernel}_S1_over_sums"] = t1 / t
            rec[f"rows_{kernel}_S1_work_bytes"] = nbytes
            # the rows are the sums' (tw_mmd_sums on the same operands)
            got = (rx[0, :, 0].sum() / 2.0, rz[0, :, 1].sum() / 2.0, rx[0, :, 1].sum())
            rec[f"rows_{kernel}_S1_match_sums"] = bool(np.allclose(got, out[0], rtol=1e-11, atol=0))
        sums_ms[d] = rec["sums_gaussian_ms"]
        t8, reps8, nbytes, rx, rz = R.rows("gaussian", 8)
        rec["rows_gaussian_S8_ms"], rec["rows_gaussian_S8_reps"] = t8, reps8
        rec["rows_gaussian_S8_work_bytes"] = nbytes
        rec["rows_gaussian_S8_over_8_sums"] = t8 / (8.0 * sums_ms[d])
        rec["bar_S1"] = MARGIN
        rec["bar_S1_met"] = bool(rec["rows_gaussian_S1_over_sums"] <= MARGIN)
        if d == 8:  # one core for scale: 64 rows of X against everything, scaled
            cs = [mm._coef("gaussian", s)[1] for s in grid_of(d, 8)]
            nrows = min(n, 64)
            a, r, per_pair = np_rows(X, Z, cs, nrows)
            rec["numpy_rows"] = nrows
            rec["numpy_S8_ms"] = per_pair * 2 * n * (2 * n) * 1e3  # all four sums, ordered pairs
            rec["numpy_note"] = f"one core; {nrows} rows of X timed, scaled to the 2n x 2n ordered pairs"
            rec["numpy_matches"] = bool(np.allclose(a, rx[:, :nrows, 0], rtol=1e-11, atol=0)
                                        and np.allclose(r, rx[:, :nrows, 1], rtol=1e-11, atol=0))
            rec["speedup_over_numpy_S8"] = rec["numpy_S8_ms"] / t8
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    # g's lane-ops from tw_mmd_sums' own times: t(d) ~ 3 d + G at d = 2 and d = 8
    t2, t8 = sums_ms[2], sums_ms[8]
    G = (24.0 * t2 - 6.0 * t8) / (t8 - t2)
    res["G_lane_ops"] = G
    for rec in res["shapes"]:
        d = rec["d"]
        model = (3.0 * d + 8.0 * G) / (8.0 * (3.0 * d + G))
        rec["model_S8_over_8_sums"] = model
        rec["bar_S8"] = model * MARGIN
        rec["bar_S8_met"] = bool(rec["rows_gaussian_S8_over_8_sums"] <= model * MARGIN)
        rec["S8_faster_than_8_launches"] = bool(rec["rows_gaussian_S8_over_8_sums"] < 1.0)
    # 64 blocks of 1562 x 1562
    X, Z = make(rows_per_class, rows_per_class, 8, 8)
    R = Resident(X, Z, blocks)
    t, reps, _ = R.sums("gaussian")
    t1, reps1, nbytes, _, _ = R.rows("gaussian", 1)
    res["blocks"] = {"N": blocks, "block": [R.k, R.kz], "d": 8, "sums_ms": t, "rows_S1_ms": t1,
                     "rows_S1_over_sums": t1 / t, "reps": [reps, reps1], "work_bytes": nbytes,
                     "call_ms": host_ms(lambda: mv._rows_blocks(
                         X[:blocks * R.k], Z[:blocks * R.kz], np.arange(blocks + 1) * R.k,
                         np.arange(blocks + 1) * R.kz, 0, [-1.0 / 16.0]))}
    print(json.dumps(res["blocks"]), flush=True)
    # select_sigma end to end on a grid of 16
    X, Z = make(n, n, 8, 8)
    grid = list(math.sqrt(8) * np.geomspace(0.1, 10.0, 16))
    sel = mv.select_sigma(X, Z, grid)
    res["select_sigma"] = {"n": n, "m": n, "d": 8, "grid": 16, "index": sel.index,
                           "sigma": sel.sigma, "criterion_max": float(sel.criterion[sel.index]),
                           "call_ms": host_ms(lambda: mv.select_sigma(X, Z, grid)),
                           "Un_var_one_sigma_call_ms": host_ms(lambda: mv.Un_var(X, Z, sigma=grid[8])),
                           "Un_call_ms": host_ms(lambda: mm.Un(X, Z, sigma=grid[8]))}
    print(json.dumps(res["select_sigma"]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
