"""A/B of how the class-run count's pre-passes are launched on
tools/count_classform_ab.py's ten shapes.  One fresh child process per pass, REPS passes; inside
each child tw_count_pairs_chain_planes under tw_count_chain_prepass 1 (the separate launches:
the zeroing, k_chain_planes, k_chain_zclasses), 2 (the fused k_chain_prepass wherever the class
form runs) and 0 (automatic), interleaved over 7 rounds, everything else automatic; per mode the
median, min and max ms of the whole native call, the ratio of medians to mode 1 of the same
process, mode 1's own spread (max - min) / median, and the form each mode ran
(tw_count_chain_prepass_of).  Counts must agree exactly.
Run on the GPU box:  python tools/count_prepass_ab.py [out.json]"""
import json
import os
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
from count_classform_ab import REPS, ROUNDS, SHAPES  # noqa: E402

MODES = [("separate", 1), ("fused", 2), ("automatic", 0)]
BASE = "separate"


def child():
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    import tuplewise  # noqa: F401
    from tuplewise import _lib as L
    from tuplewise.device import prop_swor_layout

    gen = torch.Generator(device="cuda").manual_seed(1)
    report = []
    for name, G, K in SHAPES:
        if G == 0:  # C2: one bag of 1e5 x 1e5
            nl, Nl, bound = 100_000, 1, 100_000
        elif G < 0:
            nl, Nl, bound = 64 * (7 * 2048 + 100), 64, 1_000_000
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
        ts = {m[0]: [] for m in MODES}
        forms, ref = {}, None

        def call():
            L.call("tw_count_pairs_chain_planes", xb, xo, nl, zb, zo, nl, Nl, K, k, kz, 0, bound,
                   out, L.stream_handle(), work, wb)
        try:
            for _ in range(ROUNDS):
                for mname, mode in MODES:
                    assert L.lib().tw_count_chain_prepass(mode) in (0, 1, 2)
                    forms[mname] = int(L.lib().tw_count_chain_prepass_of(Nl, K, k, kz, bound))
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    call()  # warm
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    if ref is None:
                        ref = out.clone()
                    assert torch.equal(out, ref), (name, mname)
                    ts[mname].append(e0.elapsed_time(e1))
        finally:
            L.lib().tw_count_chain_prepass(0)
        ms = {s: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
              for s, t in ts.items()}
        report.append({"shape": name, "bags": K * Nl, "nx": k, "nz": kz, "form": forms, "ms": ms,
                       f"ratio to {BASE}": {s: ms[s]["median"] / ms[BASE]["median"] for s in ms},
                       f"spread of {BASE}": (ms[BASE]["max"] - ms[BASE]["min"]) / ms[BASE]["median"]})
    print(json.dumps(report))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    env = dict(os.environ)
    env.pop("TW_LIB_PATH", None)
    passes = []
    for rep in range(REPS):
        r = subprocess.run([sys.executable, __file__, "--child"], env=env, capture_output=True,
                           text=True, timeout=600)
        if r.returncode != 0:
            print("failed:", r.stderr[-1500:], flush=True)
            sys.exit(1)
        rows = json.loads(r.stdout.strip().splitlines()[-1])
        passes.append(rows)
        for row in rows:
            print(f"pass {rep} {row['shape']}: spread of {BASE} {row[f'spread of {BASE}']:.4f}  "
                  + "  ".join(f"{m[0]} {row[f'ratio to {BASE}'][m[0]]:.4f} (form "
                              f"{row['form'][m[0]]})" for m in MODES[1:]), flush=True)
        if out:
            pathlib.Path(out).write_text(json.dumps(
                {"what": "tw_count_pairs_chain_planes under tw_count_chain_prepass 1 (separate "
                         "launches), 2 (fused) and 0 (automatic), everything else automatic: ms of "
                         "the whole native call and the ratio of medians to the separate launches "
                         "inside each child; one child per pass", "passes": passes},
                indent=1) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--child"]:
        child()
    else:
        main()
