"""In-process A/B of the class-run form of the plane-reading chain count (csrc/chainclass.h,
DESIGN §4.1g) on tools/count_planes_ab.py's shapes: tw_count_pairs_chain_planes with classes off
(tw_count_chain_set_class_bits 0: k_count_chain_planes, the baseline), under the automatic rule
(-1) and under forced class bits 4 .. 8, each under the automatic plan; with a second argument
"sweep" also forced bits x forced z chunks (default 256, 400, 602, 1024).  Interleaved over 7
rounds; per variant the median, min and max ms of the whole native call (both pre-passes +
count) and the ratio of medians to k = 0; counts must agree exactly.
Run on the GPU box:  python tools/count_classes_ab.py [out.json [sweep [z chunks ...]]]"""
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import tuplewise  # noqa: F401
from tuplewise import _lib as L
from tuplewise.device import prop_swor_layout

gen = torch.Generator(device="cuda").manual_seed(1)
ROUNDS = 7
SWEEP = len(sys.argv) > 2 and sys.argv[2] == "sweep"
ZCS = [int(v) for v in sys.argv[3:]] or [256, 400, 602, 1024]
# (name, class bits, z_chunk)
VARIANTS = [("k=0", 0, 0), ("automatic", -1, 0)] + [(f"k={k}", k, 0) for k in (4, 5, 6, 7, 8)]
if SWEEP:
    VARIANTS += [(f"k={k} zc={zc}", k, zc) for k in (4, 5, 6, 7, 8) for zc in ZCS]
shapes = [("headline K=20", 1, 20), ("headline K=32", 1, 32), ("headline K=4", 1, 4),
          ("G=2 K=20", 2, 20), ("G=4 K=4", 4, 4), ("G=4 K=20", 4, 20), ("G=8 K=4", 8, 4),
          ("G=8 K=20", 8, 20), ("C2", 0, 1)]
report = []
for name, G, K in shapes:
    if G == 0:  # C2: one bag of 1e5 x 1e5
        nl, Nl, bound = 100_000, 1, 100_000
    else:  # a rank's share of the strong problem: images are ranks against all 1e6 Z
        nl, Nl, bound = 1_000_000 // G, 64 // G, 1_000_000
    x_off, z_off, _ = prop_swor_layout(nl, nl, Nl)
    xo, zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    k, kz = int(np.diff(x_off).max()), int(np.diff(z_off).max())
    xb = torch.randint(0, bound + 1, (K, nl), device="cuda", generator=gen).float()
    zb = -torch.randint(0, bound + 1, (K, nl), device="cuda", generator=gen).float()
    out = torch.empty((K, Nl), dtype=torch.int64, device="cuda")
    wb = int(L.lib().tw_chain_planes_work_bytes(Nl, K, k, kz, 0, bound))
    work = torch.empty(max(wb, 256), dtype=torch.uint8, device="cuda")
    ts = {v[0]: [] for v in VARIANTS}
    ref = None

    def call():
        L.call("tw_count_pairs_chain_planes", xb, xo, nl, zb, zo, nl, Nl, K, k, kz, 0, bound,
               out, L.stream_handle(), work, wb)
    for rnd in range(ROUNDS):
        for vname, bits, zc in VARIANTS:
            L.call("tw_count_chain_set_plan", 0, zc)
            L.call("tw_count_chain_set_class_bits", bits)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call()  # warm
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if ref is None:
                ref = out.clone()
            assert torch.equal(out, ref), (name, vname)
            ts[vname].append(e0.elapsed_time(e1))
    L.call("tw_count_chain_set_plan", 0, 0)
    L.call("tw_count_chain_set_class_bits", -1)
    row = {"shape": name, "bags": K * Nl, "nx": k, "nz": kz, "image_bound": bound,
           "work_bytes": wb,
           "ms": {v: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
                  for v, t in ts.items()}}
    row["ratio to k=0"] = {v: row["ms"][v]["median"] / row["ms"]["k=0"]["median"] for v in ts}
    report.append(row)
    print(f"{name} ({K * Nl} bags of {k} x {kz}):\n  " + "\n  ".join(
        f"{v}: {m['median']:.4f} [{m['min']:.4f}, {m['max']:.4f}]  x{row['ratio to k=0'][v]:.4f}"
        for v, m in row["ms"].items()), flush=True)
    if len(sys.argv) > 1:
        pathlib.Path(sys.argv[1]).write_text(json.dumps(report, indent=1) + "\n")
