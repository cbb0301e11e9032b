"""Sweeps of the class count's run-time hooks on tools/count_classes_ab.py's shapes, with the
library as built (the class loop's build-time forms this tool once compared are retired: DESIGN
§4.1h, §4.1i).  One fresh child process per pass, REPS passes; inside each child
tw_count_pairs_chain_planes under every setting of the sweep, interleaved over 7 rounds; per
setting the median, min and max ms of the whole native call (both pre-passes + count) and the
ratio of medians to the sweep's base setting in the same process.  Counts must agree exactly.
Run on the GPU box:  python tools/count_classform_ab.py --spans|--digits [out.json]

--spans [out.json]: the span sweep of DESIGN §4.1j: under the automatic class bits and swap
rule, tw_count_chain_class_span forced to 1, 2, 4, 8, 16, 32 and the whole bag, and the automatic rule, interleaved over the rounds; per shape and
span the median, min and max ms, the ratio of medians to M = 1 of the same process, and M = 1's
own spread (max - min) / median, against which a shape's automatic setting is judged.

--digits [out.json]: the digit-width sweep of DESIGN §4.1k, same shapes, one process per
pass: under the automatic class bits, swap rule and span, tw_count_chain_class_digits
forced to 3 (the four-digit loop), to 4 (the wide digits where NB - K = 12) and automatic,
interleaved over the rounds; per shape the ratio of medians of the whole native call to the
four-digit loop and the four-digit loop's own spread.  Shapes whose automatic class bits leave a
low field other than 12 planes run the same kernel under every setting.

--lds [out.json]: the LDS-table sweep of DESIGN §4.1m, same shapes, one process per pass: under
the automatic class bits, swap rule and digit width, tw_count_chain_class_lds at 1 (off: the
digit loops), 2 (on wherever the form fits) and automatic, interleaved over the rounds; per
shape the ratio of medians of the whole native call to off, off's own spread, the launch's
(bag, x tile) blocks and whether each setting ran the form (tw_count_chain_class_lds_of).  The
span and digit sweeps above run with the form off: they measure the loops they name.

--lds-blocks [out.json]: the same three settings over launches of 128 .. 1024 (bag, tile)
blocks (G = 4: 16 bags of 4 tiles per step, K = 2 .. 16 steps), around the whole multiples of
the chip's 256 CUs: the form runs one block per CU at a time."""
import json
import os
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
ROUNDS, REPS = 7, 2
# (name, class bits, swap, span): span 0 is the automatic rule
WHOLE_BAG = 1 << 20  # (clamped to the launch's table capacity)
SPAN_SETTINGS = [("M=1", -1, 1, 1)] + [(f"M={m}", -1, 1, m) for m in (2, 4, 8, 16, 32)] + [
    ("M=whole bag", -1, 1, WHOLE_BAG), ("automatic", -1, 1, 0)]
# (name, class bits, swap, span, planes per digit)
DIGIT_SETTINGS = [("digits=3", -1, 1, 0, 3), ("digits=4", -1, 1, 0, 4), ("automatic", -1, 1, 0, 0)]
# (name, class bits, swap, span, planes per digit, tw_count_chain_class_lds)
LDS_SETTINGS = [("lds=off", -1, 1, 0, 0, 1), ("lds=on", -1, 1, 0, 0, 2), ("automatic", -1, 1, 0, 0, 0)]
# (name, G, K): G ranks share the strong problem; G = 0: C2; G = -1: 64 bags per step of
# 7 * 2048 + 100 x images, a remainder small enough that class_swap_mode keeps it swapped
SHAPES = [("headline K=20", 1, 20), ("headline K=32", 1, 32), ("headline K=4", 1, 4),
          ("G=2 K=20", 2, 20), ("G=4 K=4", 4, 4), ("G=4 K=20", 4, 20), ("G=8 K=4", 8, 4),
          ("G=8 K=20", 8, 20), ("C2", 0, 1), ("remainder 100 K=20", -1, 20)]


# launches of 64 K (bag, tile) blocks
BLOCK_SHAPES = [(f"G=4 K={K}", 4, K) for K in (2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16)]


def child(settings, base, shapes=None):
    sys.path.insert(0, str(ROOT))
    import numpy as np
    import torch

    import tuplewise  # noqa: F401
    from tuplewise import _lib as L
    from tuplewise.device import prop_swor_layout

    gen = torch.Generator(device="cuda").manual_seed(1)
    report = []
    for name, G, K in shapes or SHAPES:
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
        ts = {s[0]: [] for s in settings}
        form = {}
        ref = None

        def call():
            L.call("tw_count_pairs_chain_planes", xb, xo, nl, zb, zo, nl, Nl, K, k, kz, 0, bound,
                   out, L.stream_handle(), work, wb)
        try:
            for _ in range(ROUNDS):
                for sname, bits, swap, span, *digits in settings:
                    assert L.lib().tw_count_chain_class_digits(digits[0] if digits else 0) != 1
                    # (sweeps that do not name the LDS-table form run with it off)
                    assert L.lib().tw_count_chain_class_lds(digits[1] if len(digits) > 1 else 1) >= 0
                    L.call("tw_count_chain_set_class_bits", bits)
                    L.call("tw_count_chain_set_swap", swap)
                    L.lib().tw_count_chain_class_span(span)
                    form[sname] = int(L.lib().tw_count_chain_class_lds_of(Nl, K, k, kz, bound))
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    call()  # warm
                    e0.record()
                    call()
                    e1.record()
                    torch.cuda.synchronize()
                    if ref is None:
                        ref = out.clone()
                    assert torch.equal(out, ref), (name, sname)
                    ts[sname].append(e0.elapsed_time(e1))
        finally:
            L.call("tw_count_chain_set_class_bits", -1)
            L.call("tw_count_chain_set_swap", 1)
            L.lib().tw_count_chain_class_span(0)
            L.lib().tw_count_chain_class_digits(0)
            L.lib().tw_count_chain_class_lds(0)
        ms = {s: {"median": float(np.median(t)), "min": float(min(t)), "max": float(max(t))}
              for s, t in ts.items()}
        report.append({"shape": name, "bags": K * Nl, "nx": k, "nz": kz, "ms": ms,
                       "blocks of (bag, tile of 2 groups)": K * Nl * -(-(-(-k // 2048)) // 2),
                       "runs the LDS-table form": form,
                       f"ratio to {base}": {s: ms[s]["median"] / ms[base]["median"] for s in ms},
                       f"spread of {base}": (ms[base]["max"] - ms[base]["min"]) / ms[base]["median"]})
    print(json.dumps(report))


def spans_main(flag="--spans-child", settings=SPAN_SETTINGS, base="M=1",
               what="tw_count_pairs_chain_planes under forced spans (tw_count_chain_class_span)"
                    " and the automatic rule: ms of the whole native call and the ratio of "
                    "medians to M = 1 inside each child; one child per pass"):
    """One child per pass, the product library: the span sweep (or, with the arguments of
    --digits, the digit-width sweep)."""
    out = sys.argv[2] if len(sys.argv) > 2 else None
    env = dict(os.environ)
    env.pop("TW_LIB_PATH", None)
    passes = []
    for rep in range(REPS):
        r = subprocess.run([sys.executable, __file__, flag], env=env,
                           capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            print("failed:", r.stderr[-1500:], flush=True)
            sys.exit(1)
        rows = json.loads(r.stdout.strip().splitlines()[-1])
        passes.append(rows)
        for row in rows:
            print(f"pass {rep} {row['shape']}: spread of {base} {row[f'spread of {base}']:.4f}  "
                  + "  ".join(f"{s[0]} {row[f'ratio to {base}'][s[0]]:.4f}" for s in settings[1:]),
                  flush=True)
        if out:
            pathlib.Path(out).write_text(json.dumps({"what": what, "passes": passes},
                                                    indent=1) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["--spans-child"]:
        child(SPAN_SETTINGS, "M=1")
    elif sys.argv[1:2] == ["--spans"]:
        spans_main()
    elif sys.argv[1:2] == ["--digits-child"]:
        child(DIGIT_SETTINGS, "digits=3")
    elif sys.argv[1:2] == ["--digits"]:
        spans_main("--digits-child", DIGIT_SETTINGS, "digits=3",
                   "tw_count_pairs_chain_planes under tw_count_chain_class_digits 3, 4 and the "
                   "automatic rule (automatic class bits, swap and span): ms of the whole native "
                   "call and the ratio of medians to the four-digit loop inside each child; one "
                   "child per pass")
    elif sys.argv[1:2] == ["--lds-child"]:
        child(LDS_SETTINGS, "lds=off")
    elif sys.argv[1:2] == ["--lds-blocks-child"]:
        child(LDS_SETTINGS, "lds=off", BLOCK_SHAPES)
    elif sys.argv[1:2] == ["--lds-blocks"]:
        spans_main("--lds-blocks-child", LDS_SETTINGS, "lds=off",
                   "the --lds sweep over launches of 128 .. 1024 (bag, tile) blocks")
    elif sys.argv[1:2] == ["--lds"]:
        spans_main("--lds-child", LDS_SETTINGS, "lds=off",
                   "tw_count_pairs_chain_planes under tw_count_chain_class_lds 1 (off), 2 (on) and "
                   "the automatic rule (automatic class bits, swap, span and digit width): ms of "
                   "the whole native call and the ratio of medians to off inside each child; one "
                   "child per pass")
    else:
        sys.exit(__doc__)
