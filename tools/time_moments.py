"""Device time of the pair moments (tw_pair_moments, csrc/moments.hip) beside the existing sorted
count on the same blocks and the NumPy restatement on the host (GPU box).

Shapes: one block 1e5 x 1e5, 64 blocks of 15625 x 15625, one block 1e6 x 1e6, and a sweep of
square blocks from 64 to 65536 (1 block and 64 blocks per launch) with both algorithms forced,
which is where MOMENTS_SORTED_MIN_PAIRS comes from.  Every device time is the median of 5
windows after one warm call, each window `reps` back-to-back launches between two device
events (reps > 1 where one launch is far below a millisecond), reported per launch in ms.
Gaussian float64 scores, strict mode unless --half.

Usage: time_moments.py [--out profiles/time_moments.json] [--half] [--quick]"""
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

from tuplewise import _engine as E  # noqa: E402
from tuplewise import _lib as L  # noqa: E402


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


def host_ms(xs, zs, half):
    """np.sort + np.searchsorted moments of every block (the tests' oracle, without its NaN
    handling: the scores here are finite)."""
    def run():
        out = []
        for x, z in zip(xs, zs):
            sz, sx = np.sort(z), np.sort(x)
            lt = np.searchsorted(sz, x, "left").astype(np.uint64)
            gt = (len(sx) - np.searchsorted(sx, z, "right")).astype(np.uint64)
            if half:
                le = np.searchsorted(sz, x, "right").astype(np.uint64)
                ge = (len(sx) - np.searchsorted(sx, z, "left")).astype(np.uint64)
                a, b, q = lt + le, gt + ge, int((3 * lt + le).sum())
            else:
                a, b, q = lt, gt, int(lt.sum())
            out.append((int(a.sum()), int((a * a).sum()), int((b * b).sum()), q))
        return out
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = run()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), want


def measure(label, blocks, n, half, pairs_too=True, host=True):
    rng = np.random.RandomState(blocks * 131 + n % 9973)
    xs = [rng.normal(0.5, 1, n) for _ in range(blocks)]
    zs = [rng.normal(0.0, 1, n) for _ in range(blocks)]
    sh = E.Shards.from_blocks(xs, zs, L.TW_F64)
    xo, zo = sh.offsets_dev()
    mode, pred = ("half", L.TW_PRED_HALF) if half else ("gt", L.TW_PRED_GT)
    reps = 1 if blocks * n * n >= 1 << 33 else 20
    row = {"label": label, "blocks": blocks, "nx": n, "nz": n, "mode": mode, "reps": reps}

    def moments(algo):
        return E.moments_launch(sh.x, xo, sh.z, zo, blocks, n, n, blocks * n, blocks * n,
                                L.TW_F64, pred, algo)

    row["moments_sorted_ms"] = device_ms(lambda: moments("sorted"), reps)
    got = moments("sorted").cpu().numpy().view(np.uint64)
    if pairs_too:
        row["moments_pairs_ms"] = device_ms(lambda: moments("pairs"), reps)
        assert np.array_equal(moments("pairs").cpu().numpy().view(np.uint64), got), label
    row["count_sorted_ms"] = device_ms(
        lambda: E.count_launch(sh.x, xo, sh.z, zo, blocks, n, n, L.TW_F64, pred, "sorted"), reps)
    count = E.count_complete(sh, mode, "sorted")
    assert np.array_equal(count, got[:, 0]), label
    if host:
        row["numpy_host_ms"], want = host_ms(xs, zs, half)
        assert [tuple(int(v) for v in r) for r in got] == want, label
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_moments.json"))
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--quick", action="store_true", help="skip the 1e6 x 1e6 block")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0),
           "sorted_min_pairs": E.MOMENTS_SORTED_MIN_PAIRS,
           "timing": "median of 5 windows of `reps` launches after a warm call, device events, "
                     "ms per launch; numpy_host_ms: median of 3 host runs",
           "shapes": [], "sweep": []}
    res["shapes"].append(measure("1 x 1e5 x 1e5", 1, 100_000, a.half))
    res["shapes"].append(measure("64 x 15625 x 15625", 64, 15_625, a.half))
    if not a.quick:
        res["shapes"].append(measure("1 x 1e6 x 1e6", 1, 1_000_000, a.half))
    n = 64
    while n <= 65536:
        res["sweep"].append(measure(f"sweep 1 x {n}", 1, n, a.half, host=False))
        if n <= 16384:
            res["sweep"].append(measure(f"sweep 64 x {n}", 64, n, a.half, host=False))
        n *= 2
    out = pathlib.Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
