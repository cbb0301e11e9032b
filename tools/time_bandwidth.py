"""Device and call time of the exact median distance (tuplewise.bandwidth.median_distance,
csrc/distselect.hip) beside the permutation test it feeds (GPU box).

Shapes: pooled 1e4 + 1e4 rows at d in {2, 8, 64} and `within` 1e4 rows at d = 8.  Per shape:
  passes           the passes of one median_distance call in order, each timed alone on resident
                   operands (device events, the median of 5 windows of back-to-back calls after a
                   warm call): kind "hist" (tw_dist_hist over the pairs), "gather" (tw_dist_gather)
                   or "buf" (tw_keys_hist over the gathered keys), its groups, prefix bits, digit
                   and device_ms
  launches, reads  the native calls and the host reads of the histogram / count in one call
  call_ms          the whole median_distance call (checks, upload, passes, reads), host clock,
                   median of 5
  device_sum_ms    the passes' device_ms added
At pooled d = 8 also the bar: perm_device_ms is tw_mmd_perm_sums with 1000 permutations at the
median sigma on resident operands, in this process; ratio_call_to_perm = call_ms / perm_device_ms
(the target is <= 0.1).

Attribution (`make -C <package>/csrc ab-distsel` first): the histogram passes of the pooled d = 8
and d = 2 calls are timed again, each build in a fresh child process, with equal bins of a wave
combined before the LDS atomic (TW_DISTSEL_UPDATE=1; the product adds one LDS atomic per lane) and
with the update compiled out (=2); update_share = 1 - t(compiled out) / t(product) is the
histogram's share of a pass, for pass 1 (the exponent: one bin for nearly
every lane) and for a later pass.

Usage: time_bandwidth.py [--out profiles/time_bandwidth.json] [--quick] [--variants dir]"""
import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tuplewise import _lib as L  # noqa: E402

VARIANTS = {"wave_combined": "libtuplewise_distsel1.so", "no_update": "libtuplewise_distsel2.so"}


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


def timed(fn):
    return device_ms(fn, max(1, min(200, int(100 / max(device_ms(fn, 1), 1e-3)))))


def host_ms(fn, runs=5):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def data(pairs, n, m, d):
    rng = np.random.RandomState(d)
    X = rng.normal(size=(n, d))
    return (X, None) if pairs == "within" else (X, rng.normal(0.2, 1.0, size=(m, d)))


def time_passes(bw, X, Z, pairs, passes):
    """Each pass of `passes` alone, on resident operands."""
    A, B, pid, _ = bw._check(X, Z, pairs)
    src = bw._DeviceSource(A, B, pid)
    out, keys = [], None
    for p in passes:
        pre = np.array(p["groups"], dtype=np.uint64)
        pb = np.full(len(pre), p["bits"], dtype=np.int32)
        hp, hb = bw._host_ptr(pre), bw._host_ptr(pb)
        if p["kind"] == "gather":
            keys = L.empty((p["keys"],), torch.int64)

            def go(keys=keys):
                L.call("tw_dist_gather", src.xd, src.n, src.zd, src.m, src.d, pid, hp, hb,
                       len(pre), keys, keys.numel(), src.count_d, L.stream_handle())
        elif p["kind"] == "hist":
            def go():
                L.call("tw_dist_hist", src.xd, src.n, src.zd, src.m, src.d, pid, hp, hb, len(pre),
                       p["shift"], p["width"], src.hist_d, L.stream_handle())
        else:
            def go(keys=keys):
                L.call("tw_keys_hist", keys, keys.numel(), hp, hb, len(pre), p["shift"],
                       p["width"], src.hist_d, L.stream_handle())
        out.append(dict(p, device_ms=timed(go)))
    return out


def shape(bw, pairs, n, m, d):
    X, Z = data(pairs, n, m, d)
    log = []

    class Rec(bw._DeviceSource):
        def hist(self, groups, bits, shift, width, buffer):
            log.append({"kind": "hist" if buffer is None else "buf",
                        "groups": [int(g) for g in groups], "bits": bits, "shift": shift,
                        "width": width, "keys": 0 if buffer is None else int(buffer.numel())})
            Rec.last = self
            return super().hist(groups, bits, shift, width, buffer)

        def gather(self, groups, bits, count):
            log.append({"kind": "gather", "groups": [int(g) for g in groups], "bits": bits,
                        "shift": 0, "width": 0, "keys": int(count)})
            return super().gather(groups, bits, count)

    plain = bw._DeviceSource
    bw._DeviceSource = Rec
    try:
        sigma = float(bw.median_distance(X, Z, pairs))
    finally:
        bw._DeviceSource = plain
    rec = {"pairs": pairs, "n": n, "m": m, "d": d, "sigma": sigma,
           "pair_count": bw._pair_count(n, m, pairs), "launches": Rec.last.launches,
           "reads": Rec.last.reads}
    rec["call_ms"] = host_ms(lambda: bw.median_distance(X, Z, pairs))
    rec["passes"] = time_passes(bw, X, Z, pairs, log)
    rec["device_sum_ms"] = sum(p["device_ms"] for p in rec["passes"])
    return rec


def perm_device_ms(X, Z, sigma, P):
    import tuplewise.mmd as mm
    kid, c = mm._coef("gaussian", sigma)
    n, N, cols = X.shape[0], X.shape[0] + Z.shape[0], P + 1
    rng = np.random.RandomState(1)
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
        L.call("tw_mmd_perm_sums", wd, N, X.shape[1], ld, cols, kid, c, work, out,
               L.stream_handle())

    return timed(go)


def child(spec):
    """The histogram passes of `spec` under the library this process loaded: one JSON line."""
    import tuplewise.bandwidth as bw
    X, Z = data(spec["pairs"], spec["n"], spec["m"], spec["d"])
    res = time_passes(bw, X, Z, spec["pairs"], spec["passes"])
    print("CHILD " + json.dumps([p["device_ms"] for p in res]), flush=True)


def attribution(rec, variants_dir):
    hists = [p for p in rec["passes"] if p["kind"] == "hist"]
    spec = {k: rec[k] for k in ("pairs", "n", "m", "d")}
    spec["passes"] = [{k: p[k] for k in ("kind", "groups", "bits", "shift", "width", "keys")}
                      for p in hists]
    out = {"d": rec["d"], "passes": [{"bits": p["bits"], "groups": len(p["groups"]),
                                      "product_ms": p["device_ms"]} for p in hists]}
    for name, so in VARIANTS.items():
        path = variants_dir / so
        if not path.exists():
            out[name] = f"{so} is not built (make ab-distsel)"
            continue
        r = subprocess.run([sys.executable, __file__, "--lib", str(path), "--child",
                            json.dumps(spec)], capture_output=True, text=True, timeout=600)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("CHILD ")]
        if r.returncode != 0 or not line:
            out[name] = f"child failed ({r.returncode}): {r.stderr[-300:]}"
            continue
        for p, t in zip(out["passes"], json.loads(line[-1][6:])):
            p[name + "_ms"] = t
    for p in out["passes"]:
        if "no_update_ms" in p:
            p["update_share"] = 1.0 - p["no_update_ms"] / p["product_ms"]
            p["update_share_wave_combined"] = 1.0 - p["no_update_ms"] / p["wave_combined_ms"] \
                if "wave_combined_ms" in p else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_bandwidth.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    ap.add_argument("--lib", default=None, help="a variant build of libtuplewise.so to time")
    ap.add_argument("--variants", default=str(ROOT / "tools" / "variants"),
                    help="where `make ab-distsel` left the attribution builds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.lib:
        L.LIB_PATH = pathlib.Path(args.lib).resolve()
    assert torch.cuda.is_available(), "time_bandwidth.py needs a HIP device"
    if args.child:
        return child(json.loads(args.child))
    import tuplewise.bandwidth as bw
    big = 1000 if args.quick else 10_000
    res = {"device": torch.cuda.get_device_name(0), "lib": str(L.LIB_PATH.name),
           "digit_bits": int(L.lib().tw_dist_select_digit_bits()), "gather_cap": bw.GATHER_CAP,
           "shapes": [], "attribution": []}
    for pairs, n, m, d in (("pooled", big, big, 2), ("pooled", big, big, 8),
                           ("pooled", big, big, 64), ("within", big, 0, 8)):
        rec = shape(bw, pairs, n, m, d)
        if pairs == "pooled" and d == 8:
            X, Z = data(pairs, n, m, d)
            rec["perm_P"] = 1000
            rec["perm_device_ms"] = perm_device_ms(X, Z, rec["sigma"], 1000)
            rec["ratio_call_to_perm"] = rec["call_ms"] / rec["perm_device_ms"]
            rec["ratio_device_to_perm"] = rec["device_sum_ms"] / rec["perm_device_ms"]
        res["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    for rec in res["shapes"][:2]:
        res["attribution"].append(attribution(rec, pathlib.Path(args.variants)))
        print(json.dumps(res["attribution"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
