"""Time the incomplete drop-in with its block draws on the host and on the device.

  cs.UnNBT(X, Z, 64, 1_000_000, 2, "prop-SWOR", kernel="AUC") on host float64 arrays of 1e6 per
  class (BASELINE configs[2]) with _blocks.DEVICE_DRAWS off and on: one warm call of each, then
  the median of --reps timed calls (every call on fresh copies from the same seed);
  the draws alone, 128 x 1e6 with bound 15625: numpy_rng.randint_device (per --stream-blocks
  value) against numpy_rng.randint_batch;
  the generate kernel's words per second and the doubling's time per level (device events);
  the smallest batch (two calls of bound 15625) at which the device draws beat the host's.

Prints one JSON line.  --leg off times the host-draw call only and needs nothing this tool's
own change added (the leg that is run on the parent commit too); --root imports that tree.
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=str(pathlib.Path(__file__).resolve().parents[1]))
    ap.add_argument("--leg", choices=["both", "off"], default="both")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stream-blocks", type=int, nargs="*", default=[105, 420, 1680])
    ap.add_argument("--n", type=int, default=1_000_000)
    args = ap.parse_args()
    root = pathlib.Path(args.root)
    sys.path.insert(0, str(root))
    import torch
    import tuplewise.compute_stats as cs
    from tuplewise import _blocks as Bk, _lib as L, numpy_rng as R

    rng = np.random.RandomState(0)
    X0, Z0 = rng.normal(0.5, 1, args.n), rng.normal(0, 1, args.n)

    def call(on):
        if hasattr(Bk, "DEVICE_DRAWS"):
            Bk.DEVICE_DRAWS = on
        X, Z = X0.copy(), Z0.copy()
        np.random.seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = cs.UnNBT(X, Z, 64, 1_000_000, 2, "prop-SWOR", kernel="AUC")
        torch.cuda.synchronize()
        return time.perf_counter() - t0, v

    def timed(fn, reps=args.reps):
        fn()  # warm
        ts = [fn() for _ in range(reps)]
        return statistics.median(ts), min(ts), max(ts)

    res = {"tool": "time_unnbt_dropin", "n": args.n, "reps": args.reps,
           "device": torch.cuda.get_device_name(0)}
    gl = root / "tests" / "golden" / "golden_large.json"
    if gl.exists():
        for row in json.loads(gl.read_text()).get("cases", []):
            if "UnNBT" in json.dumps(row) and "ref_seconds" in row:
                res["ref_seconds"] = row["ref_seconds"]
    vals = {}
    for on in ([False] if args.leg == "off" else [False, True]):
        med, lo, hi = timed(lambda: call(on)[0])
        vals[on] = call(on)[1]
        res["call_on_s" if on else "call_off_s"] = {"median": med, "min": lo, "max": hi}
    if args.leg == "off":
        print(json.dumps(res))
        return
    res["value_equal"] = bool(vals[False] == vals[True])

    calls = [(0, 15625, 1_000_000)] * 128

    def draws_dev(sb, batch=calls):
        np.random.seed(7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = R.randint_device(batch, stream_blocks=sb)
        torch.cuda.synchronize()
        assert out is not None
        return time.perf_counter() - t0

    def draws_host(batch=calls):
        np.random.seed(7)
        t0 = time.perf_counter()
        R.randint_batch(batch)
        return time.perf_counter() - t0

    res["draws_host_s"] = timed(draws_host)[0]
    res["draws_device_s"] = {str(sb): timed(lambda: draws_dev(sb))[0] for sb in args.stream_blocks}

    # kernels alone, by device events: the doubling (per level) and the generate kernel
    sb = R.STREAM_BLOCKS
    key = np.random.RandomState(7).get_state()[1]
    S = int(np.ceil(1.35e8 / (624 * sb)))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    table = R.mt_states(key, S, sb)  # warm (polynomials cached)
    ev[0].record()
    table = R.mt_states(key, S, sb)
    ev[1].record()
    words = L.empty((S * sb * 624,), torch.int32)
    counts = L.empty((S * sb,), torch.int32)
    mask, rngs = np.array([16383], np.uint32), np.array([15624], np.uint32)
    gen = lambda: L.call("tw_mt_generate", L.ptr(table), S, sb, 1, mask.ctypes.data,
                         rngs.ctypes.data, L.ptr(words), L.ptr(counts), L.stream_handle())
    gen()
    ev[2].record()
    gen()
    ev[3].record()
    torch.cuda.synchronize()
    levels = max(1, (S - 1).bit_length())
    res["stream_blocks"] = sb
    res["states"] = S
    res["doubling_ms_per_level"] = ev[0].elapsed_time(ev[1]) / levels
    res["doubling_levels"] = levels
    res["generate_ms"] = ev[2].elapsed_time(ev[3])
    res["generate_words_per_s"] = S * sb * 624 / (ev[2].elapsed_time(ev[3]) * 1e-3)

    # crossover: the smallest batch (draws in all) at which the device draws win
    cross, sizes = None, {}
    for e in range(16, 25):
        half = (1 << e) // 2
        batch = [(0, 15625, half), (0, 15625, half)]
        d, h = timed(lambda: draws_dev(None, batch), 3)[0], timed(lambda: draws_host(batch), 3)[0]
        sizes[str(1 << e)] = {"device_s": d, "host_s": h}
        if cross is None and d < h:
            cross = 1 << e
    res["draws_crossover"] = cross
    res["draws_by_size"] = sizes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
