"""The headline count kernel's TRACED duration (the traced figure beside
bench.py's live `roofline.frac`): from a rocprofv3 --kernel-trace CSV of `bench.py --steps K`,
the strict k_count_chain launches of the largest grid and at least half the longest one's
duration (the K-step chunks of the headline's UnN_many calls; the strong_C3 and half-ties lines
launch shorter calls or the HALF kernel),
their mean and minimum duration, and the lane-op fraction they imply; in time order the first
is the bench's untimed warm-up call (a cold chip: its clock is still rising), the SECOND the
timed call whose HIP-event duration gives the live `frac` — `timed_ms` / `frac_timed` is that
same launch as the tracer saw it — and (round 5, late) a third the `first_call_ranking` line's
call of the same steps.
    python3 tools/traced_chain.py TRACE.csv K OUT.json"""
import csv
import json
import sys

PAIRS_PER_STEP = 64 * 15625 * 15625  # n = 1e6/class, N = 64 shards
PEAK = 256 * 64 * 2.4e9  # lane-op/s

path, K, out = sys.argv[1], int(sys.argv[2]), sys.argv[3]
# (the strict count: the packed k_count_chain<R, false>, the plane-reading
# k_count_chain_planes<NB>, whose launch's time includes its pre-pass k_chain_planes<NB>, the
# launch just before it on the stream, or its class-run form k_count_chain_classes<NB, K>, whose
# time includes both pre-passes: k_chain_planes<NB> and k_chain_zclasses, or the one launch
# that runs both, k_chain_prepass<NB>; k_count_chain_classes_lds<NB, K> is the class-run form
# with its low-field table in LDS)
every = list(csv.DictReader(open(path)))
rows = [r for r in every
        if ("k_count_chain<" in r["Kernel_Name"] and ", false>" in r["Kernel_Name"])
        or "k_count_chain_planes<" in r["Kernel_Name"]
        or "k_count_chain_classes<" in r["Kernel_Name"]
        or "k_count_chain_classes_lds<" in r["Kernel_Name"]]
pre = sorted((r for r in every if "k_chain_planes<" in r["Kernel_Name"]),
             key=lambda r: int(r["Start_Timestamp"]))
pre2 = sorted((r for r in every if "k_chain_zclasses" in r["Kernel_Name"]),
              key=lambda r: int(r["Start_Timestamp"]))
fused = sorted((r for r in every if "k_chain_prepass<" in r["Kernel_Name"]),
               key=lambda r: int(r["Start_Timestamp"]))
grid = lambda r: int(r.get("Grid_Size_X") or r.get("Grid_Size") or 0)
dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
g = max(grid(r) for r in rows)
big = sorted((r for r in rows if grid(r) == g), key=lambda r: int(r["Start_Timestamp"]))


def last_row_before(qs, r):
    before = [q for q in qs if int(q["Start_Timestamp"]) < int(r["Start_Timestamp"])]
    return before[-1] if before else None


def last_before(qs, r):
    q = last_row_before(qs, r)
    return dur(q) if q is not None else 0.0


def prepass_ms(r):
    if "k_count_chain_classes<" in r["Kernel_Name"] or "k_count_chain_classes_lds<" in r["Kernel_Name"]:
        f, z = last_row_before(fused, r), last_row_before(pre2, r)
        # (the form of THIS launch: whichever pre-pass ran last before it)
        if f is not None and (z is None or int(f["Start_Timestamp"]) > int(z["Start_Timestamp"])):
            return dur(f)
        return last_before(pre, r) + last_before(pre2, r)
    if "k_count_chain_planes<" not in r["Kernel_Name"]:
        return 0.0
    return last_before(pre, r)


pre_ds = [prepass_ms(r) for r in big]
ds = [dur(r) + q for r, q in zip(big, pre_ds)]
pre_ds = [q for q, d in zip(pre_ds, ds) if d >= 0.5 * max(ds)]
# (round 5, late: the z chunks are sized for a fixed count of work items, so calls of other
# step counts — the bench's 5-step settle calls — launch the same grid; the K-step launches
# are the long ones)
ds = [d for d in ds if d >= 0.5 * max(ds)]
mean, lo = sum(ds) / len(ds), min(ds)
res = {"kernel": rows[0]["Kernel_Name"].split("(")[0], "grid": g, "launches": len(ds),
       "steps_per_launch": K, "mean_ms": mean, "min_ms": lo,
       "frac_mean": K * PAIRS_PER_STEP / (mean * 1e-3) / PEAK,
       "frac_min": K * PAIRS_PER_STEP / (lo * 1e-3) / PEAK, "launch_ms_in_order": ds,
       "prepass_ms_in_order": pre_ds,
       "timed_ms": ds[min(1, len(ds) - 1)],
       "frac_timed": K * PAIRS_PER_STEP / (ds[min(1, len(ds) - 1)] * 1e-3) / PEAK,
       "source": path}
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res, indent=1))
