"""The learning path's fast kernels swept across their shape gates: tw_sgd_step
(k_sgd_step_narrow, csrc/hinge.hip) and the persistent narrow segment (k_sgd_segment_narrow,
csrc/sgdseg.hip: tw_sgd_segment_narrow, _swr, _tables) against one gradient + one update launch
per step, bit for bit, and that slow path against a float64 NumPy restatement built from the
oracle's pieces (O._sgd_draw, O._mulhi64, O.pair_grad, O.sgd_step).

The shapes enter the branches the golden (d = 10, N = 10, B = 20) and shuttle (d = 10,
N = B = 100) problems never reach: several LDS chunks with the fused and the per-step kernel
chunking differently, the 8-unrolled shard / row loops with a count below 8, exactly 8 and
8k + 1, N*d = 4096, d = 1 / 31 / 32 / 33, the arriver lane on both sides of B = 192, two pairs
per thread (B > 256), and every refusal of a gate (LDS above 64 KiB, N above the CU count,
d or N*d past the fused step's limits).

Tolerance against the restatement: rtol 1e-10, atol 1e-14 — the bar tests/test_gpu_learning.py
holds trajectories to (the device repeats NumPy's operation order except BLAS's dot-product
order inside the filter test).  test_inputs_have_no_rounding_dependent_filter_decision (CPU)
makes "no hinge decision of these inputs depends on that order" a checked property."""
import functools
import logging

import numpy as np
import pytest

from oracle import oracle as O

# (d, N, B, kx, kz, fused, narrow) — narrow: the persistent segment on a 256-CU MI355X
SHAPES = [
    (1, 1, 1, 1, 1, True, True),          # every minimum
    (10, 7, 7, 5, 3, True, True),         # unrolled loops: tail only
    (10, 8, 8, 40, 30, True, True),       # exactly one 8-batch
    (10, 9, 9, 41, 29, True, True),       # 8 + 1
    (31, 16, 192, 50, 20, True, True),    # arriver = the last wave; 53376 B of LDS
    (32, 12, 193, 50, 20, True, True),    # arriver = thread 0; d at the gate
    (4, 5, 257, 30, 9, True, True),       # two pairs per thread
    (32, 128, 60, 6, 4, True, True),      # N*d = 4096; 128 resident blocks
    (32, 16, 300, 25, 10, True, False),   # 83552 B of LDS; fused CH 231 vs per-step 234
    (10, 10, 1500, 91, 7, True, False),   # three chunks on both kernels
    (4, 300, 16, 3, 2, True, False),      # N above the CU count
    (33, 4, 20, 20, 10, False, False),    # d past the gate
    (32, 129, 8, 4, 3, False, False),     # N*d = 4128
]
NARROW = [s for s in SHAPES if s[6]]
MARGIN, REG, LR = 1, 0.05, 0.01
SEED = 12345
# device draws: (steps, reshuffle first); replay draws: fresh tables, then these segments
DEV_SEGMENTS = ((1, True), (2, False), (7, True), (7, False))
REPLAY_SEGMENTS = (1, 2, 7)
RTOL, ATOL = 1e-10, 1e-14


def _id(shape):
    return "d{}-N{}-B{}".format(*shape[:3])


@functools.lru_cache(maxsize=None)
def _problem(shape):
    d, N, B, kx, kz = shape[:5]
    rng = np.random.RandomState(1000 * d + N + B)
    X = rng.normal(0, 1, (N * kx, d))
    Z = rng.normal(0.4, 1.2, (N * kz, d))
    w0 = rng.normal(0, 1, (d, 1)) / np.sqrt(d)
    return X, Z, w0


@functools.lru_cache(maxsize=None)
def _replay_inputs(shape):
    """The replay runs' own draws: SWR row tables (N, kx) / (N, kz) and per segment the
    (n, 2, N, B) pair draws."""
    d, N, B, kx, kz = shape[:5]
    rr = np.random.RandomState(9 + d + N + B)
    rows_x = np.stack([rr.randint(0, N * kx, kx) for _ in range(N)]).astype(np.int64)
    rows_z = np.stack([rr.randint(0, N * kz, kz) for _ in range(N)]).astype(np.int64)
    draws = [np.stack([np.stack([rr.randint(0, kx, (N, B)), rr.randint(0, kz, (N, B))])
                       for _ in range(n)]).astype(np.int64) for n in REPLAY_SEGMENTS]
    return rows_x, rows_z, draws


def _device_rows(shape, counter):
    """tw_swr_rows_rng's tables at step counter `counter`, restated."""
    d, N, B, kx, kz = shape[:5]
    rx = np.stack([O._mulhi64(O._sgd_draw(SEED, counter, np.arange(kx), s, 0x40000000)[0],
                              N * kx) for s in range(N)])
    rz = np.stack([O._mulhi64(O._sgd_draw(SEED, counter, np.arange(kz), s, 0x20000000)[0],
                              N * kz) for s in range(N)])
    return rx, rz


@functools.lru_cache(maxsize=None)
def _plan(shape, mode):
    """Per step the absolute X and Z rows of every shard's B pairs ((N, B) each), and the step
    counts after which a segment ends."""
    d, N, B, kx, kz = shape[:5]
    steps, ends = [], []
    if mode == "device":
        c = 0
        for n, resh in DEV_SEGMENTS:
            if resh:  # the reshuffle reads the step counter where the test asked for it
                rx, rz = _device_rows(shape, c)
            for _ in range(n):
                RX, RZ = np.empty((N, B), np.int64), np.empty((N, B), np.int64)
                for s in range(N):
                    u, v = O._sgd_draw(SEED, c, np.arange(B), s, 0x80000000)
                    RX[s] = rx[s][O._mulhi64(u, kx)]
                    RZ[s] = rz[s][O._mulhi64(v, kz)]
                steps.append((RX, RZ))
                c += 1
            ends.append(c)
    else:
        rows_x, rows_z, draws = _replay_inputs(shape)
        sh = np.arange(N)[:, None]
        for seg in draws:
            for k in range(seg.shape[0]):
                steps.append((rows_x[sh, seg[k, 0]], rows_z[sh, seg[k, 1]]))
            ends.append(len(steps))
    return steps, ends


@functools.lru_cache(maxsize=None)
def _reference(shape, mode, loss, optim):
    """float64 NumPy restatement: (w before every step, w after every segment)."""
    X, Z, w0 = _problem(shape)
    N, B = shape[1], shape[2]
    steps, ends = _plan(shape, mode)
    w, dw = w0, 0
    before, after = [], []
    for i, (RX, RZ) in enumerate(steps):
        before.append(np.array(w, copy=True))
        grads = [O.pair_grad(Z[RZ[s]] - X[RX[s]], w, MARGIN, B, loss) for s in range(N)]
        w, dw = O.sgd_step(w, dw, np.mean(grads, axis=0), REG, LR, optim_type=optim)
        if i + 1 in ends:
            after.append(np.array(w, copy=True))
    return before, after


def _expected_gates(shape, cus):
    d, N, B = shape[:3]
    lds = 8 * (B * d + B + 32 + N * d)
    narrow = shape[5] and lds <= 65536 and N <= cus
    if 128 <= cus < 300:  # the range of CU counts over which the table's last column holds
        assert narrow == shape[6], (shape, cus, lds)
    return shape[5], narrow


def _cus():
    import torch
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _engine(shape, loss, optim, path):
    """An engine forced onto path A (one gradient + one update launch per step), B (tw_sgd_step)
    or C (the persistent narrow segment), after its own gates were checked."""
    import tuplewise.learning as lr
    X, Z, w0 = _problem(shape)
    eng = lr.SGDEngine(X, Z, w0, shape[1], shape[2], MARGIN, REG, LR, optim, loss=loss)
    fused, narrow = _expected_gates(shape, _cus())
    assert (eng.fused, eng.narrow_seg) == (fused, narrow), (shape, eng.fused, eng.narrow_seg)
    if path == "A":
        eng.fused = eng.narrow_seg = False
    elif path == "B":
        assert fused
        eng.narrow_seg = False
    else:
        assert fused and narrow
    return eng


def _run(shape, loss, optim, path, mode, graphs):
    """(w, dw) after every segment."""
    import torch
    eng = _engine(shape, loss, optim, path)
    out = []
    if mode == "device":
        eng.enable_device_rng(SEED)
        for n, resh in DEV_SEGMENTS:
            eng.run_segment(n, resh, graphs)
            out.append((eng.w_host(), eng.dw.cpu().numpy()))
    else:
        rows_x, rows_z, draws = _replay_inputs(shape)
        eng.set_shards(list(rows_x), list(rows_z))
        for tag, seg in enumerate(draws):
            eng.run_replay_segment(torch.from_numpy(seg).cuda(), seg.shape[0], graphs, tag)
            out.append((eng.w_host(), eng.dw.cpu().numpy()))
    torch.cuda.synchronize()
    eng.check()
    return out


# ------------------------------------------------------------------------------ (a) gates
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_gates(gpu, shape):
    """SGDEngine picks the fused step and the persistent narrow segment exactly where the
    shape table says (the CU count read from the device): a sweep that silently ran the slow
    path everywhere fails here.  The C entry points agree with the engine."""
    import tuplewise.learning as lr
    from tuplewise import _lib as L
    X, Z, w0 = _problem(shape)
    d, N, B = shape[:3]
    eng = lr.SGDEngine(X, Z, w0, N, B, MARGIN, REG, LR, "momentum")
    fused, narrow = _expected_gates(shape, _cus())
    assert eng.fused == fused
    assert eng.narrow_seg == narrow
    assert bool(L.lib().tw_sgd_step_fusable(d, N)) == fused
    assert bool(L.lib().tw_sgd_segment_narrow_ok(d, N, B)) == narrow


# ----------------------------------------------- (b) path equality, (c) against the reference
@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
@pytest.mark.parametrize("optim", ["momentum", "SGD"])
@pytest.mark.parametrize("loss", ["hinge", "logistic"])
def test_paths_equal_and_match_reference(gpu, shape, loss, optim):
    """Device and replay draws, segments of 1, 2 and 7 steps: after every segment w and dw of
    tw_sgd_step (B) and of the persistent segment (C, where the gate allows it), eager and
    hipGraph, are the bits of one gradient + one update launch per step (A); A's w is within
    rtol 1e-10 / atol 1e-14 of the float64 NumPy restatement."""
    w0 = _problem(shape)[2]
    fused, narrow = _expected_gates(shape, _cus())
    worst = 0.0
    for mode in ("device", "replay"):
        ref = _run(shape, loss, optim, "A", mode, False)
        assert all(np.all(np.isfinite(w)) for w, _ in ref)
        assert np.abs(ref[-1][0] - w0).max() > 0
        want = _reference(shape, mode, loss, optim)[1]
        assert len(want) == len(ref)
        for (w, _), ww in zip(ref, want):
            err = np.abs(w - ww) / (ATOL + RTOL * np.abs(ww))
            worst = max(worst, float(err.max()))
        for path in ("B",) * fused + ("C",) * narrow:
            for graphs in (False, True):
                got = _run(shape, loss, optim, path, mode, graphs)
                for seg, ((w, dw), (rw, rdw)) in enumerate(zip(got, ref)):
                    assert np.array_equal(w, rw) and np.array_equal(dw, rdw), \
                        (mode, path, graphs, seg)
    print(f"path A vs restatement, {_id(shape)} {loss} {optim}: max error = {worst:.3g} of "
          f"the bar")
    assert worst <= 1.0, worst


# ------------------------------------------------------------------ (d) in-kernel reshuffles
@pytest.mark.gpu
@pytest.mark.parametrize("shape", NARROW, ids=_id)
@pytest.mark.parametrize("mod", [1, 3])
@pytest.mark.parametrize("loss", ["hinge", "logistic"])
def test_swr_in_kernel_equals_row_tables(gpu, shape, loss, mod):
    """tw_sgd_segment_narrow_swr (the segment draws each reshuffle's SWR rows itself) for two
    segments of 7 steps — the second starts between two reshuffles at mod = 3 — against one
    gradient + one update launch per step with reshuffle_device() at every step counter
    divisible by mod: w and dw bit for bit."""
    n = 7
    ref_eng = _engine(shape, loss, "momentum", "A")
    ref_eng.enable_device_rng(SEED)
    ref = []
    for step in range(2 * n):
        if step % mod == 0:
            ref_eng.reshuffle_device()
        ref_eng.run_segment(1, False, False)
        if (step + 1) % n == 0:
            ref.append((ref_eng.w_host(), ref_eng.dw.cpu().numpy()))
    eng = _engine(shape, loss, "momentum", "C")
    eng.enable_device_rng(SEED)
    assert eng.swr_segments_ok(n)
    for seg in range(2):
        eng.run_segment(n, False, swr_mod=mod)
        w, dw = eng.w_host(), eng.dw.cpu().numpy()
        eng.check()
        assert np.all(np.isfinite(w))
        assert np.array_equal(w, ref[seg][0]) and np.array_equal(dw, ref[seg][1]), seg


# ------------------------------------------------------------------------- (e) whole loop
LOOP_SHAPES = [s for s in SHAPES if s[:3] in ((32, 12, 193), (4, 5, 257), (32, 128, 60))]
HIST = ("iter", "norm_w", "bc_AUC", "br_AUC", "tc_AUC", "tr_AUC")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=_id)
@pytest.mark.parametrize("mod", [1, 3, 10000])
@pytest.mark.parametrize("mode", ["replay", "device"])
def test_whole_loop_fast_paths_equal_slow(gpu, shape, mod, mode, monkeypatch):
    """learning_process with the module defaults (persistent segments through their
    reshuffles, draws made ahead) against NARROW_SEGMENT, SWR_IN_KERNEL, REPLAY_THROUGH and
    DRAW_AHEAD all off: the evaluation lists bit for bit; the per-step trajectory, and the
    default run's norm_w at its evaluations, against the oracle's restatement."""
    import tuplewise.learning as lr
    logging.disable(logging.CRITICAL)
    X, Z, w0 = _problem(shape)
    d, N, B = shape[:3]
    assert _expected_gates(shape, _cus()) == (True, True)
    rs = np.random.RandomState(77)
    test_X, test_Z = rs.normal(0, 1, (60, d)), rs.normal(0.4, 1.2, (40, d))
    mon = list(zip(rs.randint(0, X.shape[0], 300), rs.randint(0, Z.shape[0], 300)))

    def p_learn():
        return {"n_it": 47, "margin": MARGIN, "N": N, "B": B, "reshuffle_mod": mod, "reg": REG,
                "learning_rate": LR, "eval_mod": 20, "w_init": w0, "test_X": test_X,
                "test_Z": test_Z, "train_X": X, "train_Z": Z, "train_mon_pairs": mon}

    def run(**kw):
        lr._ENGINE["key"] = lr._ENGINE["eng"] = None  # neither run reuses the other's engine
        p = p_learn()
        np.random.seed(31)
        lr.learning_process(X, Z, p, rng_mode=mode, **kw)
        return p

    fast = run()
    traj = []
    run(trajectory=traj)
    for flag in ("NARROW_SEGMENT", "SWR_IN_KERNEL", "REPLAY_THROUGH", "DRAW_AHEAD"):
        monkeypatch.setattr(lr, flag, False)
    slow = run()
    lr._ENGINE["key"] = lr._ENGINE["eng"] = None
    assert fast["iter"] == [0, 20, 40]
    for k in HIST:
        assert fast[k] == slow[k], k
    np.random.seed(31)
    if mode == "replay":
        ws, _ = O.learning_trajectory(X, Z, p_learn())
    else:
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        ws, _ = O.device_rng_learning_trajectory(X, Z, p_learn(), seed)
    ws = np.stack(ws)
    np.testing.assert_allclose(np.stack(traj), ws, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(fast["norm_w"], [np.linalg.norm(ws[i]) for i in fast["iter"]],
                               rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------- (f) the inputs (CPU)
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_inputs_have_no_rounding_dependent_filter_decision(shape):
    """At every step of the restatements the GPU tests compare with, every pair's hinge score
    S = diff . w + margin (sequential-j float64 dot, the kernels' order) is at least 1e6 times
    its rounding bound (d + 2) eps sum_j |diff_j w_j| + eps away from zero, and BLAS's
    diff.dot(w) takes the same filter decisions: the 1e-10 bar of the GPU tests never has to
    absorb a flipped decision.  If a seed change breaks this, pick another seed."""
    X, Z, _ = _problem(shape)
    d, N = shape[:2]
    eps = np.finfo(np.float64).eps
    worst = np.inf
    for mode in ("device", "replay"):
        steps, _ = _plan(shape, mode)
        for optim in ("momentum", "SGD"):
            before, _ = _reference(shape, mode, "hinge", optim)
            assert len(before) == len(steps)
            for (RX, RZ), w in zip(steps, before):
                for s in range(N):
                    diff = Z[RZ[s]] - X[RX[s]]
                    S = np.zeros(diff.shape[0])
                    for j in range(d):
                        S = S + diff[:, j] * w[j, 0]
                    S = S + MARGIN
                    bound = (d + 2) * eps * (np.abs(diff) @ np.abs(w[:, 0])) + eps
                    worst = min(worst, float((np.abs(S) / bound).min()))
                    blas = (diff.dot(w) + MARGIN).ravel()
                    assert np.array_equal(S > 0, blas > 0)
    assert worst >= 1e6, worst
