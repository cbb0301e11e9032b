"""tuplewise.triplet_learning without a GPU: the NumPy oracle the GPU tests compare against (the
projection in the contract's arithmetic order, the triplet hinge and its gradient, the learning
loop restated literally with the same np.random calls in the same order, the evaluation through
the oracle of tests/test_triplets_cpu.py), the oracle's gradient against central differences of
its own loss and against the second algebraic form, every argument error before any device work
or RNG draw, and the native argument errors."""
import ctypes

import numpy as np
import pytest

from test_triplets_cpu import o_UB_indices, o_Un, same_state


# ------------------------------------------------------------------------------------ oracle
def o_project(A, Lmap):
    """A Lmap^T, (rows, p): acc = 0.0; for c: acc = acc + L[r, c] * A[row, c] — NumPy's
    elementwise multiply and add never fuse.  A NaN is np.nan itself."""
    A, Lmap = np.asarray(A), np.asarray(Lmap)
    acc = np.zeros((A.shape[0], Lmap.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(A.shape[1]):
            acc = acc + Lmap[None, :, c] * A[:, None, c]
    acc[np.isnan(acc)] = np.nan
    return acc


def o_hinge(X, Z, Lmap, i, j, k, margin):
    """(S, a, b, u, v) of the given triplets, one row each."""
    a, b = X[i] - X[j], X[i] - Z[k]
    u, v = a.dot(Lmap.T), b.dot(Lmap.T)
    S = margin + np.sum(u * u, axis=1) - np.sum(v * v, axis=1)
    return S, a, b, u, v


def o_shard(X, Z, Lmap, i, j, k, margin):
    """(mean loss, mean gradient, #{S > 0}, min |S|) of one non-empty shard."""
    S, a, b, u, v = o_hinge(X, Z, Lmap, i, j, k, margin)
    act = S > 0  # strict
    G = 2.0 * (u[act].T.dot(a[act]) - v[act].T.dot(b[act])) / len(S)
    return np.sum(S[act]) / len(S), G, int(act.sum()), float(np.min(np.abs(S)))


def o_loss_grad(X, Z, Lmap, i, j, k, margin=1.0, trip_off=None):
    """(loss, G, active, min |S|): the means over non-empty shards of the shard means, the
    per-shard counts (uint64) and the smallest |S| met."""
    off = [0, len(i)] if trip_off is None else list(trip_off)
    losses, grads, active, low = [], [], [], np.inf
    for s0, s1 in zip(off, off[1:]):
        if s1 == s0:
            active.append(0)
            continue
        ls, G, act, mn = o_shard(X, Z, Lmap, i[s0:s1], j[s0:s1], k[s0:s1], margin)
        losses.append(ls)
        grads.append(G)
        active.append(act)
        low = min(low, mn)
    G = np.mean(grads, axis=0) if grads else np.zeros(Lmap.shape)
    loss = np.float64(np.mean(losses)) if losses else np.float64("nan")
    return loss, G, np.array(active, dtype=np.uint64), low


def o_update(Lmap, delta, G, reg, lr, optim_type):
    """(L, delta) after one update, elementwise in this order."""
    g = G + reg * Lmap
    if optim_type == "SGD":
        delta = lr * g
    if optim_type == "momentum":
        delta = 0.9 * delta + lr * g
    return Lmap - delta, delta


def o_draw_triplets(n, m, B):
    i = np.random.randint(0, n, B)
    j = np.random.randint(0, n - 1, B)
    j += (j >= i)
    k = np.random.randint(0, m, B)
    return i, j, k


def o_evaluation_step(it, Lmap, p_learn, X, Z, mon_train, mon_test):
    """The module's evaluation_step from the oracle's pieces; draws nothing."""
    penalty = p_learn["reg"] * float(np.sum(Lmap * Lmap)) / 2
    p_learn.setdefault("iter", []).append(it)
    tX, tZ = p_learn.get("test_X"), p_learn.get("test_Z")
    for name, A, B, mon in (("train", X, Z, mon_train), ("test", tX, tZ, mon_test)):
        if mon is None or A is None:
            continue
        loss = o_loss_grad(A, B, Lmap, *mon, p_learn["margin"])[0]
        p_learn.setdefault(name + "_loss", []).append(np.float64(loss + penalty))
        p_learn.setdefault(name + "_stat", []).append(
            o_UB_indices(o_project(A, Lmap), o_project(B, Lmap), *mon, "gt"))
    if p_learn.get("test_complete", False) and tX is not None:
        p_learn.setdefault("test_stat_complete", []).append(
            o_Un(o_project(tX, Lmap), o_project(tZ, Lmap), "gt"))


def o_learning_process(X, Z, p_learn, optim_type="momentum"):
    """(the final L, the smallest |S| of every training triplet of the run)."""
    n, m = X.shape[0], Z.shape[0]
    N, B = p_learn["N"], p_learn["B"]
    Lmap, delta, low = p_learn["L_init"].copy(), 0, np.inf
    mon_train = mon_test = None
    if p_learn.get("n_monitor", 0) > 0:
        mon_train = o_draw_triplets(n, m, p_learn["n_monitor"])
        if p_learn.get("test_X") is not None and p_learn.get("test_Z") is not None:
            mon_test = o_draw_triplets(p_learn["test_X"].shape[0], p_learn["test_Z"].shape[0],
                                       p_learn["n_monitor"])
    k, kz = int(n / N), int(m / N)
    for it in range(p_learn["n_it"]):
        if it % p_learn["reshuffle_mod"] == 0:
            px = np.random.permutation(n)
            pz = np.random.permutation(m)
        if it % p_learn["eval_mod"] == 0:
            o_evaluation_step(it, Lmap, p_learn, X, Z, mon_train, mon_test)
        grads = []
        for b in range(N):
            i, j, q = o_draw_triplets(k, kz, B)
            _, G, _, mn = o_shard(X, Z, Lmap, px[b * k + i], px[b * k + j], pz[b * kz + q],
                                  p_learn["margin"])
            grads.append(G)
            low = min(low, mn)
        Lmap, delta = o_update(Lmap, delta, np.mean(grads, axis=0), p_learn["reg"],
                               p_learn["learning_rate"], optim_type)
    return Lmap, low


def make(n, m, d, p, seed):
    rng = np.random.RandomState(seed)
    return (rng.normal(size=(n, d)), rng.normal(0.3, 1.0, size=(m, d)),
            rng.normal(size=(p, d)) / np.sqrt(d))


def draw(rng, n, m, T):
    i, k = rng.randint(0, n, T), rng.randint(0, m, T)
    j = rng.randint(0, n - 1, T)
    return i, j + (j >= i), k


# ------------------------------------------------------------------- the oracle's own checks
def test_oracle_gradient_is_the_central_difference():
    n, m, d, p, T, h = 40, 36, 5, 3, 50, 1e-6
    X, Z, Lmap = make(n, m, d, p, 3)
    i, j, k = draw(np.random.RandomState(4), n, m, T)
    loss, G, active, low = o_loss_grad(X, Z, Lmap, i, j, k, 1.0)
    assert low > 1e-4  # no triplet near the hinge's kink
    assert 0 < int(active[0]) < T  # both sides of the hinge are exercised
    num = np.zeros_like(Lmap)
    for r in range(p):
        for c in range(d):
            E = np.zeros_like(Lmap)
            E[r, c] = h
            num[r, c] = (o_loss_grad(X, Z, Lmap + E, i, j, k, 1.0)[0]
                         - o_loss_grad(X, Z, Lmap - E, i, j, k, 1.0)[0]) / (2 * h)
    err = np.abs(num - G).max()
    print("central differences: max|num - G| =", err, "max|G| =", np.abs(G).max())
    assert err <= 1e-8 * max(1.0, np.abs(G).max())


def test_oracle_gradient_forms_agree():
    n, m, d, p, T = 40, 36, 5, 3, 50
    X, Z, Lmap = make(n, m, d, p, 3)
    i, j, k = draw(np.random.RandomState(4), n, m, T)
    S, a, b, u, v = o_hinge(X, Z, Lmap, i, j, k, 1.0)
    one, two = np.zeros_like(Lmap), np.zeros_like(Lmap)
    for t in range(T):
        if S[t] > 0:
            one += 2 * (np.outer(u[t], a[t]) - np.outer(v[t], b[t]))
            two += 2 * (np.outer(u[t] - v[t], X[i[t]]) - np.outer(u[t], X[j[t]])
                        + np.outer(v[t], Z[k[t]]))
    assert np.abs(one - two).max() <= 1e-13 * T
    G = o_loss_grad(X, Z, Lmap, i, j, k, 1.0)[1]
    assert np.abs(one / T - G).max() <= 1e-13 and np.abs(two / T - G).max() <= 1e-13


def test_oracle_project_is_the_double_loop():
    rng = np.random.RandomState(5)
    A, Lmap = rng.normal(size=(7, 17)), rng.normal(size=(5, 17))
    A[2, 3], A[4, 0], A[5, 16] = np.nan, np.inf, -np.inf
    want = np.zeros((7, 5))
    with np.errstate(invalid="ignore"):
        for row in range(7):
            for r in range(5):
                acc = 0.0
                for c in range(17):
                    acc = acc + float(Lmap[r, c]) * float(A[row, c])
                want[row, r] = np.nan if acc != acc else acc
    got = o_project(A, Lmap)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.isnan(got[2]).all() and np.isinf(got[4]).all()


def test_oracle_update_and_shards():
    rng = np.random.RandomState(6)
    Lmap, G = rng.normal(size=(3, 5)), rng.normal(size=(3, 5))
    L1, d1 = o_update(Lmap, 0, G, 0.1, 0.5, "SGD")
    assert np.array_equal(d1, 0.5 * (G + 0.1 * Lmap)) and np.array_equal(L1, Lmap - d1)
    L2, d2 = o_update(L1, d1, G, 0.1, 0.5, "momentum")
    assert np.array_equal(d2, 0.9 * d1 + 0.5 * (G + 0.1 * L1)) and np.array_equal(L2, L1 - d2)
    # an empty shard contributes nothing: the mean is over the non-empty ones
    X, Z, Lm = make(12, 9, 4, 2, 7)
    i, j, k = draw(rng, 12, 9, 10)
    loss, Gs, act, _ = o_loss_grad(X, Z, Lm, i, j, k, 1.0, [0, 4, 4, 10])
    la, Ga = o_loss_grad(X, Z, Lm, i[:4], j[:4], k[:4], 1.0)[:2]
    lb, Gb = o_loss_grad(X, Z, Lm, i[4:], j[4:], k[4:], 1.0)[:2]
    assert np.allclose(Gs, (Ga + Gb) / 2, rtol=0, atol=1e-15) and act[1] == 0
    assert abs(loss - (la + lb) / 2) <= 1e-15


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import sys
    import tuplewise.triplet_learning as tl
    for name in ("project", "loss_grad", "learning_process", "evaluation_step"):
        assert callable(getattr(tl, name)), name
    assert tl.MAX_DIM == 64 and tl.OPTIMS == ("SGD", "momentum")
    assert sys.modules["tuplewise.triplet_learning"] is tl
    assert "triplet_learning" not in tw.__all__  # not one of the package's eager imports


def p_learn_of(Lmap, **over):
    p = {"n_it": 4, "N": 2, "B": 3, "margin": 1.0, "reg": 0.01, "learning_rate": 0.1,
         "reshuffle_mod": 2, "eval_mod": 2, "L_init": Lmap}
    p.update(over)
    return p


def test_argument_errors_need_no_device(tw):
    import tuplewise.triplet_learning as tl
    X, Z = np.arange(40.0).reshape(10, 4), np.arange(24.0).reshape(6, 4) + 0.5
    Lm = np.arange(8.0).reshape(2, 4) / 8
    X0, Z0, L0 = X.copy(), Z.copy(), Lm.copy()
    wide, Lwide = np.zeros((4, 65)), np.zeros((2, 65))
    i, j, k = np.array([0, 1, 2]), np.array([1, 2, 0]), np.array([0, 5, 3])
    state = np.random.get_state()
    lp = tl.learning_process
    calls = [
        # dtype
        lambda: tl.project(X.astype(np.float32), Lm), lambda: tl.project(X, Lm.astype(np.float32)),
        lambda: tl.loss_grad(X, Z.astype(np.int64), Lm, i, j, k),
        lambda: tl.loss_grad(X, Z, Lm.astype(np.float32), i, j, k),
        lambda: tl.loss_grad(X, Z, Lm, i.astype(np.float64), j, k),
        lambda: lp(X.astype(np.float32), Z, p_learn_of(Lm)),
        lambda: lp(X, Z, p_learn_of(Lm.astype(np.float16))),
        # layout
        lambda: tl.project(X[:, ::2], Lm[:, ::2]), lambda: tl.project(X, np.asfortranarray(Lm)),
        lambda: tl.loss_grad(X.T, Z.T, Lm, i, j, k), lambda: tl.project(X, Lm.reshape(-1)),
        lambda: tl.project(X, Lm.tolist()), lambda: lp(X, Z, p_learn_of(Lm.T.copy().T)),
        lambda: tl.loss_grad(X, Z, Lm, i.reshape(3, 1), j.reshape(3, 1), k.reshape(3, 1)),
        # d or p out of range, mismatched d
        lambda: tl.project(wide, Lwide), lambda: tl.loss_grad(wide, wide, Lwide, i, j, k),
        lambda: tl.project(X, np.zeros((65, 4))), lambda: tl.project(X, np.zeros((0, 4))),
        lambda: tl.project(np.zeros((3, 0)), np.zeros((2, 0))),
        lambda: tl.project(X, np.zeros((2, 5))), lambda: tl.loss_grad(X, Z[:, :3].copy(), Lm, i, j, k),
        lambda: tl.loss_grad(X, Z, np.zeros((2, 3)), i, j, k),
        lambda: lp(X, Z, p_learn_of(np.zeros((2, 5)))), lambda: lp(X, Z, p_learn_of(np.zeros((65, 4)))),
        lambda: lp(X, Z, p_learn_of(Lm, test_X=np.zeros((5, 3)), test_Z=np.zeros((5, 3)))),
        lambda: lp(X, Z, p_learn_of(Lm, test_X=X)),
        # an index out of range, i == j, lengths, offsets
        lambda: tl.loss_grad(X, Z, Lm, [10, 1, 2], j, k), lambda: tl.loss_grad(X, Z, Lm, i, [-1, 2, 0], k),
        lambda: tl.loss_grad(X, Z, Lm, i, j, [0, 6, 3]), lambda: tl.loss_grad(X, Z, Lm, i, i, k),
        lambda: tl.loss_grad(X, Z, Lm, i, j[:2], k),
        lambda: tl.loss_grad(X, Z, Lm, i, j, k, trip_off=[0, 2]),
        lambda: tl.loss_grad(X, Z, Lm, i, j, k, trip_off=[1, 3]),
        lambda: tl.loss_grad(X, Z, Lm, i, j, k, trip_off=[0, 2, 1, 3]),
        lambda: tl.loss_grad(X, Z, Lm, i, j, k, margin=float("nan")),
        # blocks too small, B < 1, the other knobs
        lambda: lp(X, Z, p_learn_of(Lm, N=6)), lambda: lp(X, Z[:4], p_learn_of(Lm, N=5)),
        lambda: lp(X, Z, p_learn_of(Lm, N=0)), lambda: lp(X, Z, p_learn_of(Lm, B=0)),
        lambda: lp(X, Z, p_learn_of(Lm, B=-3)), lambda: lp(X, Z, p_learn_of(Lm, B=2.5)),
        lambda: lp(X, Z, p_learn_of(Lm, reshuffle_mod=0)), lambda: lp(X, Z, p_learn_of(Lm, eval_mod=0)),
        lambda: lp(X, Z, p_learn_of(Lm, n_it=-1)), lambda: lp(X, Z, p_learn_of(Lm, n_monitor=-1)),
        lambda: lp(X, Z, p_learn_of(Lm, margin="wide")),
        lambda: lp(X, Z, {key: v for key, v in p_learn_of(Lm).items() if key != "reg"}),
        # optim_type
        lambda: lp(X, Z, p_learn_of(Lm), optim_type="adam"), lambda: lp(X, Z, p_learn_of(Lm), None),
        # evaluation_step: a map that does not fit the samples
        lambda: tl.evaluation_step(0, np.zeros((2, 3)), dict(p_learn_of(Lm), train_X=X, train_Z=Z)),
        lambda: tl.evaluation_step(0, Lm, dict(p_learn_of(Lm), train_X=X, train_Z=Z,
                                               train_monitor=(i, i, k))),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    assert np.array_equal(X, X0) and np.array_equal(Z, Z0) and np.array_equal(Lm, L0)
    p = p_learn_of(Lm, N=6)
    with pytest.raises(ValueError, match="at least 2 rows"):
        lp(X, Z, p)
    assert "iter" not in p and "train_X" not in p  # nothing was begun


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.triplet_learning as tl
    X, Z, Lm = make(10, 6, 4, 2, 0)
    state = np.random.get_state()
    with pytest.raises(RuntimeError, match="no HIP device"):
        tl.project(X, Lm)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tl.loss_grad(X, Z, Lm, [0, 1], [2, 3], [0, 1])
    with pytest.raises(RuntimeError, match="no HIP device"):
        tl.learning_process(X, Z, p_learn_of(Lm))
    assert same_state(np.random.get_state(), state)


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    q = ctypes.cast(buf, ctypes.c_void_p)

    def grad(d=3, p=2, n_shards=1, max_t=4, margin=1.0, want=1, ptr=q, G=q):
        return lib.tw_triplet_grad(q, ptr, d, q, p, q, q, q, q, n_shards, max_t, margin, want, q,
                                   G, q, q, None)

    def proj(rows=2, d=3, p=2, ptr=q):
        return lib.tw_triplet_project(q, rows, d, ptr, p, q, None)

    def upd(count=6, momentum=1, ptr=q):
        return lib.tw_triplet_sgd_update(q, ptr, q, count, 0.1, 0.1, momentum, None)

    cases = [
        (b"tw_triplet_grad", [(lambda: grad(ptr=None), b"null pointer"),
                              (lambda: grad(G=None), b"null pointer"),
                              (lambda: grad(d=0), b"d 0 outside [1, 64]"),
                              (lambda: grad(d=65), b"d 65 outside [1, 64]"),
                              (lambda: grad(p=0), b"p 0 outside [1, 64]"),
                              (lambda: grad(p=65), b"p 65 outside [1, 64]"),
                              (lambda: grad(n_shards=-1), b"n_shards"),
                              (lambda: grad(max_t=-1), b"max_triplets"),
                              (lambda: grad(want=2), b"want_grad"),
                              (lambda: grad(margin=float("nan")), b"margin")]),
        (b"tw_triplet_project", [(lambda: proj(ptr=None), b"null pointer"),
                                 (lambda: proj(d=0), b"outside [1, 64]"),
                                 (lambda: proj(d=65), b"outside [1, 64]"),
                                 (lambda: proj(p=0), b"outside [1, 64]"),
                                 (lambda: proj(p=65), b"outside [1, 64]"),
                                 (lambda: proj(rows=-1), b"rows")]),
        (b"tw_triplet_sgd_update", [(lambda: upd(ptr=None), b"null pointer"),
                                    (lambda: upd(count=0), b"count"),
                                    (lambda: upd(count=64 * 64 + 1), b"count"),
                                    (lambda: upd(momentum=2), b"momentum")]),
    ]
    for name, rows in cases:
        for call, word in rows:
            assert call() == L.TW_ERR_ARG, word
            msg = lib.tw_last_error()
            assert word in msg and name in msg, msg
    assert proj(rows=0) == L.TW_OK  # no rows: nothing to do
    tile = lib.tw_triplet_grad_tile()
    assert 64 <= tile <= 4096 and tile % 64 == 0
    wb = lib.tw_triplet_grad_work_bytes
    small, big = wb(1, 1, 1, 1), wb(100, 1000, 64, 64)
    assert 8 <= small <= big < 1 << 28
    # one partial of p d doubles, a loss and a count per workgroup
    assert wb(3, 2 * tile + 3, 5, 7) == 3 * 3 * (16 + 5 * 7 * 8)
    assert wb(-1, 1, 1, 1) == 0 and wb(1, 1, 65, 1) == 0 and wb(1, 1, 1, 0) == 0
