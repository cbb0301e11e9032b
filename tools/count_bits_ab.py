"""In-process A/B of the chain count's two kernels (csrc/chain.hip) on tools/count_plan_ab.py's
shapes: tw_count_pairs_chain (packed f32, k_count_chain) against the bounded count HipOps
issues (tw_count_pairs_chain_planes: bit-sliced on planes built once per bag, k_chain_planes +
k_count_chain_planes or its class-run form, where chainplan.h's chain_count_sliced lets it)
under the automatic plan, and forced to R = 2 and R = 4 plane groups.  Interleaved over 7
rounds; per variant the median, min and max ms; counts must agree exactly.  The automatic rule is right
where "bound" is no slower than "packed" beyond the packed rounds' own spread.
Run on the GPU box:  python tools/count_bits_ab.py [out.json]"""
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import tuplewise  # noqa: F401
from tuplewise import _lib as L
from tuplewise.device import HipOps, prop_swor_layout

ops = HipOps()
gen = torch.Generator(device="cuda").manual_seed(1)
ROUNDS = 7
VARIANTS = [("packed", None, 0), ("bound", True, 0), ("bits R=2", True, 2), ("bits R=4", True, 4)]
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
    ts = {v[0]: [] for v in VARIANTS}
    ref = None

    def call(bounded):
        if bounded:
            with ops.bounded_images(bound):
                ops.count_chain(xb, xo, zb, zo, Nl, K, nl, nl, k, kz, False, out)
        else:
            ops.count_chain(xb, xo, zb, zo, Nl, K, nl, nl, k, kz, False, out)
    for rnd in range(ROUNDS):
        for vname, bounded, R in VARIANTS:
            L.call("tw_count_chain_set_plan", R, 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            call(bounded)  # warm
            e0.record()
            call(bounded)
            e1.record()
            torch.cuda.synchronize()
            if ref is None:
                ref = out.clone()
            assert torch.equal(out, ref), (name, vname)
            ts[vname].append(e0.elapsed_time(e1))
    L.call("tw_count_chain_set_plan", 0, 0)
    row = {"shape": name, "bags": K * Nl, "nx": k, "nz": kz, "image_bound": bound,
           "ms": {v: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
                  for v, t in ts.items()}}
    row["bound_over_packed"] = row["ms"]["bound"]["median"] / row["ms"]["packed"]["median"]
    report.append(row)
    print(f"{name} ({K * Nl} bags of {k} x {kz}): " + ", ".join(
        f"{v} {m['median']:.4f} [{m['min']:.4f}, {m['max']:.4f}]" for v, m in row["ms"].items())
        + f"  bound/packed {row['bound_over_packed']:.3f}", flush=True)
if len(sys.argv) > 1:
    pathlib.Path(sys.argv[1]).write_text(json.dumps(report, indent=1) + "\n")
