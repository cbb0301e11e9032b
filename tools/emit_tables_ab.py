"""The chain emission with its Feistel rounds looked up (tw_chain_set_emit_tables 2), computed (1)
and under the automatic rule (0), interleaved in one process: 2e6, 1e6, 500k and 250k elements
x K = 4 and 20 steps, one process (64 shards, into step bags) and the exchange (one rank of
G = 2 holding that many elements, into send buckets: the domains are twice as large).  Per
shape the median launch time of each setting over ROUNDS interleaved rounds of REPS launches,
the ratio to `off` and off's own spread (min - max of its per-round medians) — the evidence
for the automatic rule and for kEmTabMaxHB.  Run on the GPU box:
    python tools/emit_tables_ab.py [out.json]"""
import json
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np
import torch

import tuplewise  # noqa: F401
from tuplewise import _lib as L
from tuplewise.device import HipOps

ROUNDS, REPS = 7, 5
MODES = (1, 2, 0)
M64 = 2 ** 64 - 1
ops = HipOps()
gen = torch.Generator(device="cuda").manual_seed(1)
rows = []
for xchg in (False, True):
    for E in (2_000_000, 1_000_000, 500_000, 250_000):
        n = E // 2
        G = 2 if xchg else 1
        N = 64 // G
        xr = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device="cuda", generator=gen)
        zr = torch.randint(0, 1 << 24, (n,), dtype=torch.int64, device="cuda", generator=gen)
        xpos = torch.empty(n, dtype=torch.int32, device="cuda")
        zpos = torch.empty(n, dtype=torch.int32, device="cuda")
        k = n // N
        for K in (4, 20):
            kxs = [(2 * i) & M64 for i in range(K)]
            kzs = [(2 * i + 1) & M64 for i in range(K)]
            if xchg:
                cap = E // G + E // (8 * G) + 1024
                send = torch.empty(G * K * (cap + 1), dtype=torch.int64, device="cuda")
                flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                kw = dict(send=send, cap=cap, flag=flag)
            else:
                kw = dict(x_bag=torch.empty((K, n), dtype=torch.float32, device="cuda"),
                          z_bag=torch.empty((K, n), dtype=torch.float32, device="cuda"),
                          cursors=torch.empty(K * 2 * (N + 1), dtype=torch.int32, device="cuda"))

            def call():
                ops.chain_emit(xr, zr, False, xpos, zpos, True, G - 1, G, kxs, kzs, k, k, N, **kw)

            per = {m: [] for m in MODES}
            runs = {}
            for rnd in range(ROUNDS):
                for m in MODES:
                    L.lib().tw_chain_set_emit_tables(m)
                    runs[m] = int(L.lib().tw_chain_emit_tables_of(n, n, G, 0, int(xchg), N))
                    call()  # warm
                    ts = []
                    for _ in range(REPS):
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        call()
                        e1.record()
                        torch.cuda.synchronize()
                        ts.append(e0.elapsed_time(e1) * 1e3)
                    per[m].append(float(np.median(ts)))
            L.lib().tw_chain_set_emit_tables(0)
            med = {m: float(np.median(per[m])) for m in MODES}
            row = dict(mode="exchange G=2" if xchg else "one process", elements=E, K=K,
                       off_us=med[1], on_us=med[2], auto_us=med[0], auto_runs_tables=runs[0],
                       on_over_off=med[2] / med[1], auto_over_off=med[0] / med[1],
                       off_spread=(max(per[1]) - min(per[1])) / med[1])
            rows.append(row)
            print(json.dumps(row), flush=True)
if len(sys.argv) > 1:
    pathlib.Path(sys.argv[1]).write_text(json.dumps(rows, indent=1) + "\n")
