"""Device time of triplet metric learning (tuplewise.triplet_learning, csrc/triplet_grad.hip)
beside the NumPy oracle of tests/test_triplet_learning_cpu.py on one core (GPU box).

Shapes: n = m = 1e5 rows per class, (d, p) in {(8, 8), (64, 64), (64, 8)}, N = 100 blocks,
B in {100, 1000} triplets per block and step.

The gradient launch alone (tw_triplet_grad: the gradient kernel and its reduction, on resident
operands and one step's resident draws) and the gradient kernel's share of it (the same launch
with want_grad = 0 has the same reduction grid but for G's elements, so the split is not exact:
both are given) are device times, the median of 5 windows after one warm call, each window `reps`
back-to-back launches between two device events, per launch in ms.  From the launch's time:
f64 lane-ops/s — a triplet costs 2 p d multiply-adds for u and v and, when active, 2 p d for its
outer products, each multiply-add one lane-op — beside the 3.93e13 lane-op/s VALU issue peak, and
gathered bytes/s — three rows of d doubles and three int32 indices per triplet — beside the HBM
rate the microarchitecture guide gives as achievable (6.3e12 B/s).

The steps/s are of 200 steps of learning_process without evaluations (eval_mod beyond n_it: the
one evaluation at step 0 has nothing to monitor; reshuffle_mod = 50), host clock around the whole
call — permutations, draws, uploads, launches, the final read-back — the median of 3 after one
warm call.  The oracle runs the first 10 of those steps once, on one core; its final map is
compared with the device's for the same 10 steps.

Usage: time_triplet_learning.py [--out profiles/time_triplet_learning.json] [--quick]"""
import argparse
import json
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tuplewise.triplet_learning as tl  # noqa: E402
from tuplewise import _lib as L  # noqa: E402
from test_triplet_learning_cpu import o_learning_process  # noqa: E402

VALU_PEAK = 3.93e13  # lane-op/s (256 CU x 64 lanes x 2.4 GHz)
HBM_ACHIEVABLE = 6.3e12  # B/s


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


def host_s(fn, runs=3):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def one_thread():
    """The oracle's matrix products on one BLAS thread (threadpoolctl, where it is installed;
    else whatever the environment gives NumPy: `oracle_note` says which)."""
    try:
        import threadpoolctl
        return threadpoolctl.threadpool_limits(limits=1)
    except ImportError:
        import contextlib
        return contextlib.nullcontext()


def oracle_note():
    try:
        import threadpoolctl  # noqa: F401
        return "one core"
    except ImportError:
        return "NumPy's BLAS threads as the environment sets them"


def reps_for(ms_guess):
    """Windows of about 0.1 s."""
    return max(1, min(500, int(100 / max(ms_guess, 1e-3))))


def p_learn_of(L0, N, B, n_it):
    return {"n_it": n_it, "N": N, "B": B, "margin": 1.0, "reg": 0.01, "learning_rate": 0.01,
            "reshuffle_mod": 50, "eval_mod": 10 ** 9, "L_init": L0}


def shape(n, d, p, N, B, steps, seed):
    rng = np.random.RandomState(seed)
    X, Z = rng.normal(size=(n, d)), rng.normal(0.5, 1.0, size=(n, d))
    L0 = rng.normal(size=(p, d)) / np.sqrt(d)
    k = n // N
    # one step's draws on one partition, resident
    px, pz = rng.permutation(n), rng.permutation(n)
    i = rng.randint(0, k, size=(N, B))
    j = rng.randint(0, k - 1, size=(N, B))
    j += j >= i
    q = rng.randint(0, k, size=(N, B))
    base = (np.arange(N) * k)[:, None]
    xd, zd, ld, id_, jd, kd, od = L.to_device_many(
        [X.reshape(-1), Z.reshape(-1), L0.reshape(-1), px[base + i].astype(np.int32).reshape(-1),
         px[base + j].astype(np.int32).reshape(-1), pz[base + q].astype(np.int32).reshape(-1),
         np.arange(N + 1, dtype=np.int64) * B])
    g = tl._Grad(N, B, d, p)

    def launch(want_grad):
        g.launch(xd, zd, ld, id_, jd, kd, od, 1.0, want_grad, L.stream_handle())

    reps = reps_for(device_ms(lambda: launch(1), 1))
    t_grad, t_loss = device_ms(lambda: launch(1), reps), device_ms(lambda: launch(0), reps)
    active = int(g.active.cpu().numpy()[:N].sum())
    trip = N * B
    lane_ops = 2 * p * d * (trip + active)
    gathered = trip * (3 * 8 * d + 12)
    rec = {"n": n, "m": n, "d": d, "p": p, "N": N, "B": B, "block": [k, k], "triplets": trip,
           "active_share": active / trip, "reps": reps, "grad_launch_ms": t_grad,
           "loss_only_launch_ms": t_loss, "triplets_per_s": trip / (t_grad * 1e-3),
           "lane_ops": lane_ops, "lane_ops_per_s": lane_ops / (t_grad * 1e-3),
           "valu_peak_lane_ops_per_s": VALU_PEAK,
           "share_of_valu_peak": lane_ops / (t_grad * 1e-3) / VALU_PEAK,
           "gathered_bytes": gathered, "gathered_bytes_per_s": gathered / (t_grad * 1e-3),
           "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "share_of_hbm": gathered / (t_grad * 1e-3) / HBM_ACHIEVABLE,
           "work_bytes": int(L.lib().tw_triplet_grad_work_bytes(N, B, d, p))}

    def run(n_it):
        np.random.seed(seed)
        return tl.learning_process(X, Z, p_learn_of(L0, N, B, n_it), "momentum")

    run(steps)  # warm
    t_run = host_s(lambda: run(steps))
    rec.update(steps=steps, learning_process_s=t_run, steps_per_s=steps / t_run,
               device_only_steps_per_s_bound=1e3 / t_grad)
    o_steps = min(10, steps)
    np.random.seed(seed)
    with one_thread():
        t0 = time.perf_counter()
        Lo, low = o_learning_process(X, Z, p_learn_of(L0, N, B, o_steps), "momentum")
        t_o = time.perf_counter() - t0
    Lg = run(o_steps)
    rec.update(oracle_steps=o_steps, oracle_s=t_o, oracle_steps_per_s=o_steps / t_o,
               oracle_note=oracle_note(), speedup=(steps / t_run) / (o_steps / t_o),
               oracle_min_abs_S=low, max_abs_diff_vs_oracle=float(np.abs(Lg - Lo).max()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "time_triplet_learning.json"))
    ap.add_argument("--quick", action="store_true", help="small shapes (a rehearsal)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_triplet_learning.py needs a HIP device"
    n, N, steps = (4000, 10, 20) if args.quick else (100_000, 100, 200)
    res = {"device": torch.cuda.get_device_name(0), "tile": int(L.lib().tw_triplet_grad_tile()),
           "shapes": []}
    for d, p in ((8, 8), (64, 64), (64, 8)):
        for B in (100, 1000):
            res["shapes"].append(shape(n, d, p, N, B, steps, 10 * d + p))
            print(json.dumps(res["shapes"][-1]), flush=True)
    pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    pathlib.Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
