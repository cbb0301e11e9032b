"""tuplewise.hsic_var without a GPU: the NumPy oracle the GPU tests compare against (the five row
sums by math.fsum over the terms of tests/test_hsic_cpu.py's K and L, the component h restated
from the module's docstring), the oracle against the brute-force symmetrised kernel over all
4-tuples and against o_Un, the first-order variance against the empirical variance over
replications, every argument error before any device work or RNG draw, the native entry's argument
checks, and — with the device glue stubbed to the oracle — select_sigma's rules and UnN_var
against hsic.UnN."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from test_hsic_cpu import KERNELS, o_components, o_fsum, o_KL, o_Un, paired, sig
from test_triplets_cpu import o_dist_rows, same_state


# ------------------------------------------------------------------------------------ oracle
def o_rows_of(K, L):
    """(p, k, l, u, v) of the matrices K and L (zero diagonals), every sum an fsum of its terms."""
    with np.errstate(invalid="ignore"):
        p = np.array([o_fsum(a * b) for a, b in zip(K, L)])
        k, l = np.array([o_fsum(a) for a in K]), np.array([o_fsum(b) for b in L])  # noqa: E741
        u, v = np.array([o_fsum(a * l) for a in K]), np.array([o_fsum(b * k) for b in L])
    return p, k, l, u, v


def o_rows(X, Y, kernel, sigma=None):
    return o_rows_of(*o_KL(X, Y, kernel, sigma))


def o_h_terms(p, k, l, u, v):  # noqa: E741
    """The (n, 8) terms of h_i's formula, each divided by 2 (n - 1)(n - 2)(n - 3)."""
    n = len(p)
    s_kl, r_k, r_l = o_fsum(p) / 2.0, o_fsum(k), o_fsum(l)
    with np.errstate(invalid="ignore"):
        r_kl = o_fsum(k * l)
        one = np.ones(n)
        t = np.stack([(n - 2.0) ** 2 * p, (n - 2.0) * 2.0 * s_kl * one, -(n - 2.0) * u,
                      -(n - 2.0) * v, -n * k * l, r_l * k, r_k * l, -r_kl * one], axis=1)
    return t / (2.0 * (n - 1.0) * (n - 2.0) * (n - 3.0))


def o_h(p, k, l, u, v):  # noqa: E741
    return np.array([o_fsum(t) for t in o_h_terms(p, k, l, u, v)])


def o_h_scale(p, k, l, u, v):  # noqa: E741
    """The sum of the absolute values of the terms of every h_i (NaN rows as 0)."""
    return np.nan_to_num(np.abs(o_h_terms(p, k, l, u, v)).sum(axis=1), nan=0.0)


def o_var_of_rows(p, k, l, u, v):  # noqa: E741
    """(value, var, se, h, zeta) from the rows, as the module states it."""
    n = len(p)
    h = o_h(p, k, l, u, v)
    with np.errstate(invalid="ignore"):
        zeta = np.var(h, ddof=1)
        var = 16.0 * zeta / n
        return np.float64(np.mean(h)), np.float64(var), np.float64(math.sqrt(max(var, 0.0))
                                                                     if var == var else var), h, zeta


def o_Un_var(X, Y, kernel, sigma=None):
    return o_var_of_rows(*o_rows(X, Y, kernel, sigma))


def o_UnN_var(X, Y, N, kernel, sigma=None):
    """hsic.UnN's draw and blocks; (mean of the blocks' values, mean of their var / N)."""
    perm = np.random.permutation(X.shape[0])
    X[:] = X[perm]
    Y[:] = Y[perm]
    k = int(X.shape[0] / N)
    v = [o_Un_var(X[b * k:(b + 1) * k], Y[b * k:(b + 1) * k], kernel, sigma) for b in range(N)]
    return np.mean([t[0] for t in v]), np.mean([t[1] for t in v]) / N


def o_select(X, Y, pairs, reg=1e-8):
    """(index, criterion, value, var) of the grid of pairs."""
    v = [o_Un_var(X, Y, "gaussian", tuple(s)) for s in pairs]
    value, var = np.array([t[0] for t in v]), np.array([t[1] for t in v])
    crit = value / np.sqrt(np.maximum(var, 0.0) + reg)
    return int(np.nanargmax(crit)), crit, value, var


def fake_rows_blocks(calls=None):
    """The device glue hsic_var._rows_blocks restated on the oracle (Gaussian: exp(D * c) with the
    module's own c, not a rebuilt sigma)."""
    def rows_blocks(Xf, Yf, off, kid, cs):
        if calls is not None:
            calls.append(len(cs))
        first = np.full((len(cs), int(off[-1]), 3), -7.0)
        second = np.full((len(cs), int(off[-1]), 3), -7.0)
        for s, (cx, cy) in enumerate(cs):
            for b in range(len(off) - 1):
                x, y = Xf[off[b]:off[b + 1]], Yf[off[b]:off[b + 1]]
                with np.errstate(invalid="ignore", over="ignore"):
                    if KERNELS[kid] == "gaussian":
                        K, L = np.exp(o_dist_rows(x, x) * cx), np.exp(o_dist_rows(y, y) * cy)
                    else:
                        K, L = np.sqrt(o_dist_rows(x, x)), np.sqrt(o_dist_rows(y, y))
                np.fill_diagonal(K, 0.0)
                np.fill_diagonal(L, 0.0)
                p, k, l, u, v = o_rows_of(K, L)  # noqa: E741
                first[s, off[b]:off[b + 1]] = np.stack([p, k, l], axis=1)
                second[s, off[b]:off[b + 1]] = np.stack([p, u, v], axis=1)
        return first, second
    return rows_blocks


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [6, 7])
def test_h_is_the_mean_of_the_symmetrised_kernel_over_the_tuples_of_i(kernel, n):
    """Over the ordered 4-tuples of distinct items, f(a, b, c, d) = K_ab (L_ab + L_cd - 2 L_ac);
    the mean over every tuple that holds i, in any place, is the mean of the symmetrised kernel
    over the 4-subsets that hold i."""
    X, Y = paired(n, 3, 2, n)
    sigma = sig(kernel, 3, 2)
    K, L = o_KL(X, Y, kernel, sigma)
    tot, cnt = [[] for _ in range(n)], np.zeros(n)
    for t in itertools.permutations(range(n), 4):
        a, b, c, d = t
        f = K[a, b] * (L[a, b] + L[c, d] - 2.0 * L[a, c])
        for i in t:
            tot[i].append(f)
            cnt[i] += 1
    brute = np.array([math.fsum(t) for t in tot]) / cnt
    h = o_h(*o_rows(X, Y, kernel, sigma))
    assert np.abs(h - brute).max() <= 1e-13
    assert abs(np.mean(h) - o_Un(X, Y, kernel, sigma)) <= 1e-13
    # and the leave-one-out form it expands: (T - T_{-i}) / (4 (n - 1)(n - 2)(n - 3))
    def T(K, L):
        m, k, l = len(K), K.sum(1), L.sum(1)  # noqa: E741
        return (m - 1) * (m - 2) * (K * L).sum() + k.sum() * l.sum() - 2 * (m - 1) * (k @ l)
    cut = [T(np.delete(np.delete(K, i, 0), i, 1), np.delete(np.delete(L, i, 0), i, 1))
           for i in range(n)]
    loo = (T(K, L) - np.array(cut)) / (4.0 * (n - 1) * (n - 2) * (n - 3))
    assert np.abs(h - loo).max() <= 1e-12 * max(1.0, np.abs(K).max() * np.abs(L).max())


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,dx,dy", [(4, 1, 1), (9, 3, 2), (31, 8, 9)])
def test_oracle_value_is_o_Un_and_the_sums_are_the_components(kernel, n, dx, dy):
    X, Y = paired(n, dx, dy, 4)
    sigma = sig(kernel, dx, dy)
    p, k, l, u, v = o_rows(X, Y, kernel, sigma)  # noqa: E741
    value = o_Un_var(X, Y, kernel, sigma)[0]
    assert abs(value - o_Un(X, Y, kernel, sigma)) <= 1e-13 * max(1.0, abs(value))
    c = o_components(X, Y, kernel, sigma)
    tol = 1e-14
    assert abs(o_fsum(p) - 2.0 * c[0]) <= tol * c[0]
    assert abs(o_fsum(k) - c[3]) <= tol * c[3] and abs(o_fsum(l) - c[4]) <= tol * c[4]
    assert abs(o_fsum(u) - c[5]) <= tol * c[5] and abs(o_fsum(v) - c[5]) <= tol * c[5]


def np_Un_var(X, Y, sigma):
    """(value, var) of the Gaussian kernel by plain NumPy sums (the Monte Carlo's restatement)."""
    c = -1.0 / (2.0 * sigma * sigma)

    def gram(A):
        sq = (A * A).sum(1)[:, None] + (A * A).sum(1)[None, :] - 2.0 * A @ A.T
        G = np.exp(np.maximum(sq, 0.0) * c)
        np.fill_diagonal(G, 0.0)
        return G

    n = len(X)
    K, L = gram(X), gram(Y)
    p, k, l = (K * L).sum(1), K.sum(1), L.sum(1)  # noqa: E741
    u, v = K @ l, L @ k
    s_kl, r_k, r_l, r_kl = p.sum() / 2.0, k.sum(), l.sum(), k @ l
    h = ((n - 2.0) ** 2 * p + (n - 2.0) * (2.0 * s_kl - u - v) - n * k * l + r_l * k + r_k * l
         - r_kl) / (2.0 * (n - 1.0) * (n - 2.0) * (n - 3.0))
    return h.mean(), 16.0 * np.var(h, ddof=1) / n


def test_restatement_is_the_oracle():
    X, Y = paired(40, 2, 1, 9)
    value, var = np_Un_var(X, Y, 1.0)
    want = o_Un_var(X, Y, "gaussian", 1.0)
    assert abs(value - want[0]) <= 1e-12 and abs(var - want[1]) <= 1e-9 * want[1]


@pytest.mark.parametrize("n,noise", [(100, 1.0), (200, 2.0)])
def test_var_estimates_the_variance_of_the_value(n, noise):
    """Away from independence the first-order term carries the variance: over 400 replications
    (X ~ N(0, I_2), Y = X_0 + noise N(0, 1), sigma = 1) the mean of var lies within 0.8 - 1.35 of
    the empirical variance of the value."""
    rng = np.random.RandomState(1234)
    out = []
    for _ in range(400):
        X = rng.normal(size=(n, 2))
        Y = X[:, :1] + noise * rng.normal(size=(n, 1))
        out.append(np_Un_var(X, Y, 1.0))
    out = np.array(out)
    ratio = out[:, 1].mean() / np.var(out[:, 0], ddof=1)
    print(f"n={n} noise={noise}: mean(var) / var(value) = {ratio:.3f}")
    assert 0.8 <= ratio <= 1.35


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.hsic_var as hv
    for name in ("row_sums", "Un_var", "Un_ci", "UnN_var", "select_sigma"):
        assert callable(getattr(hv, name)), name
    assert hv.HSICRows._fields == ("p", "k", "l", "u", "v")
    assert hv.HSICVariance._fields == ("value", "var", "se", "h", "zeta")
    assert hv.SigmaSelection._fields == ("sigma", "index", "criterion", "value", "var")
    assert "hsic_perm" in hv.__doc__ and "hsic_perm" in hv.Un_var.__doc__


def test_argument_errors_need_no_device(tw, monkeypatch):
    import tuplewise.hsic_var as hv
    L = tw._lib

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks were done")

    for name in ("call", "to_device_many", "to_device", "empty", "device"):
        monkeypatch.setattr(L, name, no_device)
    X, Y = np.arange(48.0).reshape(12, 4), np.arange(36.0).reshape(12, 3) + 0.5
    X0, Y0 = X.copy(), Y.copy()
    x1 = np.arange(12.0)
    wide = np.zeros((6, 65))
    D = dict(kernel="distance")
    G = dict(sigma=1.0)
    nan, inf = float("nan"), float("inf")
    state = np.random.get_state()

    def refused(fn):
        return [
            # everything hsic.Un refuses: dtype, layout, rank
            lambda: fn(X.astype(np.float32), Y, **D), lambda: fn(X, Y.astype(np.int64), **G),
            lambda: fn(X[:, ::2], Y, **D), lambda: fn(X.T[:3].T, Y, **G),
            lambda: fn(X.reshape(6, 2, 4), Y[:6], **D), lambda: fn(x1[::2], x1[:6], **D),
            # d above 64, none
            lambda: fn(wide, Y[:6], **G), lambda: fn(X[:6], wide, **D),
            lambda: fn(np.zeros((6, 0)), Y[:6], **D), lambda: fn(X, np.zeros((12, 0)), **G),
            # rows of X != rows of Y; n < 4
            lambda: fn(X, Y[:11], **D), lambda: fn(X[:5], Y, **G), lambda: fn(X[:3], Y[:3], **D),
            lambda: fn(X[:0], Y[:0], **G),
            # the kernel and its sigma
            lambda: fn(X, Y, kernel="laplace", sigma=1.0), lambda: fn(X, Y, kernel=None),
            lambda: fn(X, Y, kernel="energy"), lambda: fn(X, Y), lambda: fn(X, Y, kernel="gaussian"),
            lambda: fn(X, Y, sigma=0.0), lambda: fn(X, Y, sigma=-1.0), lambda: fn(X, Y, sigma=nan),
            lambda: fn(X, Y, sigma=inf), lambda: fn(X, Y, sigma="wide"), lambda: fn(X, Y, sigma=1e-200),
            lambda: fn(X, Y, sigma=(1.0,)), lambda: fn(X, Y, sigma=(1.0, 2.0, 3.0)),
            lambda: fn(X, Y, sigma=(1.0, 0.0)), lambda: fn(X, Y, sigma=(nan, 1.0)),
            lambda: fn(X, Y, sigma=(1.0, None)), lambda: fn(X, Y, sigma=[]), lambda: fn(X, Y, sigma=()),
            lambda: fn(X, Y, kernel="distance", sigma=1.0),
            lambda: fn(X, Y, kernel="distance", sigma=(1.0, 2.0)),
            # grids: empty, a bad entry, a bad shape, the distance kernel
            lambda: fn(X, Y, sigma=np.zeros((0, 2))), lambda: fn(X, Y, sigma=np.ones((2, 3))),
            lambda: fn(X, Y, sigma=np.ones((2, 2, 2))), lambda: fn(X, Y, sigma=[(1.0, 2.0), (1.0, 0.0)]),
            lambda: fn(X, Y, sigma=[(1.0, 2.0), (-1.0, 1.0)]), lambda: fn(X, Y, sigma=[(nan, 1.0)]),
            lambda: fn(X, Y, sigma=((1.0, inf),)), lambda: fn(X, Y, sigma=[(1.0, "wide")]),
            lambda: fn(X, Y, sigma=[(1.0, None)]), lambda: fn(X, Y, sigma=[(1.0, 2.0), 3.0]),
            lambda: fn(X, Y, sigma=[(1.0, 2.0, 3.0)]), lambda: fn(X, Y, sigma=[(1.0,)]),
            lambda: fn(X, Y, sigma=[[(1.0, 2.0)]]), lambda: fn(X, Y, sigma=[(1.0, 2.0), "median"]),
            lambda: fn(X, Y, kernel="distance", sigma=[(1.0, 2.0)]),
            lambda: fn(X, Y, kernel="distance", sigma=np.ones((1, 2))),
            lambda: fn(X, Y, kernel="x", sigma=[(1.0, 2.0)]),
        ]

    calls = refused(hv.row_sums) + refused(hv.Un_var) + refused(
        lambda X, Y, **k: hv.Un_ci(X, Y, 0.9, **k)) + refused(
        lambda X, Y, **k: hv.UnN_var(X, Y, 2, **k))
    calls += [
        # the interval's level
        lambda: hv.Un_ci(X, Y, 0.0, **G), lambda: hv.Un_ci(X, Y, 1.0, **D),
        lambda: hv.Un_ci(X, Y, -0.5, **G), lambda: hv.Un_ci(X, Y, 1.5, **G),
        lambda: hv.Un_ci(X, Y, nan, **D), lambda: hv.Un_ci(X, Y, "x", **G),
        lambda: hv.Un_ci(X, Y, None, **G), lambda: hv.Un_ci(X, Y, level=95, **G),
        # the block estimator: partitions out of scope, short blocks, lists, a grid
        lambda: hv.UnN_var(X, Y, 2, "SWOR", **D), lambda: hv.UnN_var(X, Y, 2, "prop-SWR", **G),
        lambda: hv.UnN_var(X, Y, 4, **D), lambda: hv.UnN_var(X, Y, 13, **G),
        lambda: hv.UnN_var(X, Y, 0, **D),
        lambda: hv.UnN_var(X.tolist(), Y, 2, **G), lambda: hv.UnN_var(X, Y.tolist(), 2, **D),
        lambda: hv.UnN_var(X, Y, 2, sigma=[(1.0, 2.0)]),
        lambda: hv.UnN_var(X, Y, 2, sigma=np.ones((2, 2))),
        # select_sigma: the distance kernel, no grid, reg
        lambda: hv.select_sigma(X, Y, [(1.0, 1.0)], kernel="distance"),
        lambda: hv.select_sigma(X, Y, 1.0), lambda: hv.select_sigma(X, Y, (1.0, 2.0)),
        lambda: hv.select_sigma(X, Y, []), lambda: hv.select_sigma(X, Y, np.zeros((0, 2))),
        lambda: hv.select_sigma(X, Y, [(1.0, 0.0)]),
        lambda: hv.select_sigma(X, Y, [(1.0, 1.0)], reg=-1e-9),
        lambda: hv.select_sigma(X, Y, [(1.0, 1.0)], reg=nan),
        lambda: hv.select_sigma(X, Y, [(1.0, 1.0)], reg=inf),
        lambda: hv.select_sigma(X, Y, [(1.0, 1.0)], reg="x"),
        lambda: hv.select_sigma(X[:3], Y[:3], [(1.0, 1.0)]),
        lambda: hv.select_sigma(X, Y.astype(np.float32), [(1.0, 1.0)]),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    with pytest.raises(ValueError, match="empty"):
        hv.Un_var(X, Y, sigma=np.zeros((0, 2)))
    with pytest.raises(ValueError, match="no sigma"):
        hv.Un_var(X, Y, kernel="distance", sigma=[(1.0, 2.0)])
    with pytest.raises(ValueError, match="Gaussian kernel only"):
        hv.select_sigma(X, Y, [(1.0, 1.0)], kernel="distance")
    with pytest.raises(ValueError, match="reg"):
        hv.select_sigma(X, Y, [(1.0, 1.0)], reg=-1.0)
    with pytest.raises(ValueError, match="level"):
        hv.Un_ci(X, Y, 1.0, **G)
    with pytest.raises(ValueError, match="prop-SWOR"):
        hv.UnN_var(X, Y, 2, "SWOR", **D)
    with pytest.raises(ValueError, match="at least 4 rows"):
        hv.UnN_var(X, Y, 4, **D)
    # a shape whose partials would pass the device work budget, alone and as one block
    big = np.zeros(300_000)
    for call in (lambda: hv.Un_var(big, big.copy(), **D), lambda: hv.row_sums(big, big.copy(), **G),
                 lambda: hv.UnN_var(big, big.copy(), 1, **D)):
        with pytest.raises(ValueError, match="1 GiB|work budget"):
            call()
        assert same_state(np.random.get_state(), state)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.hsic_var as hv
    X, Y = paired(8, 3, 2, 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        hv.row_sums(X, Y, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        hv.Un_var(X, Y, kernel="distance")
    with pytest.raises(RuntimeError, match="no HIP device"):
        hv.Un_ci(X, Y, 0.9, sigma=(1.0, 2.0))
    with pytest.raises(RuntimeError, match="no HIP device"):
        hv.select_sigma(X, Y, [(0.5, 1.0), (1.0, 1.0)])
    with pytest.raises(RuntimeError, match="no HIP device"):
        hv.UnN_var(X, Y, 2, sigma=1.0)


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    S = lib.tw_hsic_rows_max_sigma()
    assert 2 <= S <= 64

    def rows(dx=3, dy=2, n_blocks=1, max_n=4, kern=L.TW_HSIC_GAUSSIAN, c=p, n_sigma=1, w=None,
             ptr=p, work=p, out=p):
        return lib.tw_hsic_rows(p, dx, ptr, dy, p, n_blocks, max_n, kern, c, n_sigma, w, work, out,
                                None)

    D = dict(kern=L.TW_HSIC_DISTANCE)
    for call, word in ((lambda: rows(ptr=None), b"null pointer"),
                       (lambda: rows(out=None), b"null pointer"),
                       (lambda: rows(work=None), b"null pointer"),
                       (lambda: rows(c=None), b"null pointer"),
                       (lambda: rows(n_blocks=-1), b"negative size"),
                       (lambda: rows(max_n=-1), b"negative size"),
                       (lambda: rows(dx=0), b"dx 0 outside [1, 64]"),
                       (lambda: rows(dx=65), b"dx 65 outside [1, 64]"),
                       (lambda: rows(dy=0), b"dy 0 outside [1, 64]"),
                       (lambda: rows(dy=65), b"dy 65 outside [1, 64]"),
                       (lambda: rows(kern=2), b"unknown kernel"),
                       (lambda: rows(kern=-1), b"unknown kernel"),
                       (lambda: rows(n_sigma=0), b"n_sigma"),
                       (lambda: rows(n_sigma=-3), b"n_sigma"),
                       (lambda: rows(n_sigma=S + 1), b"n_sigma"),
                       (lambda: rows(n_sigma=2, **D), b"distance kernel"),
                       (lambda: rows(max_n=3), b"at least 4 rows"),
                       (lambda: rows(max_n=0), b"at least 4 rows"),
                       (lambda: rows(max_n=1 << 31), b"2^31"),
                       (lambda: rows(n_blocks=2 ** 31 - 1, max_n=4), b"grid too large"),
                       (lambda: rows(max_n=10 ** 5), b"d_work past"),
                       (lambda: rows(n_blocks=1024, max_n=1562, n_sigma=S), b"d_work past")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_hsic_rows" in msg, msg
    # nothing to do: no blocks (the distance kernel reads no coefficient; d_w may be NULL or not)
    assert rows(n_blocks=0) == L.TW_OK and rows(n_blocks=0, c=None, **D) == L.TW_OK
    assert rows(n_blocks=0, w=p) == L.TW_OK
    with pytest.raises(ValueError, match="n_sigma"):
        L.call("tw_hsic_rows", p, 3, p, 2, p, 1, 4, 0, p, 0, None, p, p, None)
    wb = lib.tw_hsic_rows_work_bytes
    P = lib.tw_hsic_tile()
    # one tile: 2 columns of 4 rows of 3 sums per pair
    assert wb(1, 4, 1) == 2 * 4 * 3 * 8 and wb(1, 4, S) == S * wb(1, 4, 1)
    assert wb(5, P + 1, 2) == 5 * 2 * 3 * (P + 1) * 3 * 8
    assert 0 < wb(1, 10 ** 4, S) <= 1 << 30 and 0 < wb(64, 1562, S) <= 1 << 30
    for bad in ((0, 4, 1), (-1, 4, 1), (1, 3, 1), (1, -1, 1), (1, 4, 0), (1, 4, S + 1),
                (1, 1 << 31, 1), (2 ** 31 - 1, 4, 1), (1, 10 ** 5, 1), (1024, 1562, S)):
        assert wb(*bad) == 0, bad


# -------------------------------------------------- the host arithmetic on the oracle's rows
def test_public_functions_on_stubbed_rows(tw, monkeypatch):
    import statistics
    import tuplewise.hsic_var as hv
    monkeypatch.setattr(hv, "_rows_blocks", fake_rows_blocks())
    X, Y = paired(23, 3, 2, 5)
    for kernel, sigma in (("gaussian", (1.5, 2.5)), ("gaussian", 1.2), ("distance", None)):
        rows, want = hv.row_sums(X, Y, kernel, sigma), o_rows(X, Y, kernel, sigma)
        for g, w in zip(rows, want):
            assert g.shape == w.shape == (23,) and g.dtype == np.float64
            assert np.allclose(g, w, rtol=1e-14, atol=0)
        v, w = hv.Un_var(X, Y, kernel, sigma), o_Un_var(X, Y, kernel, sigma)
        assert all(isinstance(t, np.float64) for t in (v.value, v.var, v.se, v.zeta))
        assert abs(v.value - w[0]) <= 1e-13 and abs(v.var - w[1]) <= 1e-11 * w[1]
        assert abs(v.se - w[2]) <= 1e-11 * w[2] and v.se == math.sqrt(v.var)
        assert np.allclose(v.h, w[3], rtol=0, atol=1e-13) and v.h.shape == (23,)
        assert abs(v.zeta - w[4]) <= 1e-11 * w[4] and v.var == 16.0 * v.zeta / 23
        assert abs(v.value - o_Un(X, Y, kernel, sigma)) <= 1e-13
        assert abs(np.mean(v.h) - v.value) <= 1e-16
        value, lo, hi = hv.Un_ci(X, Y, 0.9, kernel, sigma)
        z = statistics.NormalDist().inv_cdf(0.95)
        assert value == v.value and lo == v.value - z * v.se and hi == v.value + z * v.se
    grid = [(0.5, 1.0), (1.5, 2.5), (4.0, 0.7)]
    rows = hv.row_sums(X, Y, sigma=grid)
    assert all(r.shape == (3, 23) for r in rows)
    v = hv.Un_var(X, Y, sigma=np.array(grid))
    assert v.value.shape == v.var.shape == v.se.shape == v.zeta.shape == (3,) and v.h.shape == (3, 23)
    value, lo, hi = hv.Un_ci(X, Y, sigma=tuple(grid))
    assert value.shape == lo.shape == hi.shape == (3,) and np.all(lo < value) and np.all(value < hi)
    for s, sigma in enumerate(grid):
        one = hv.Un_var(X, Y, sigma=sigma)
        assert v.value[s] == one.value and v.var[s] == one.var and v.se[s] == one.se
        assert np.array_equal(v.h[s], one.h)
        assert np.array_equal(rows.u[s], hv.row_sums(X, Y, sigma=sigma).u)
    assert hv.row_sums(X, Y, sigma=[(1.5, 2.5)]).p.shape == (1, 23)


def test_select_sigma_rules_and_split(tw, monkeypatch):
    import tuplewise.hsic_var as hv
    S = tw._lib.lib().tw_hsic_rows_max_sigma()
    launches = []
    monkeypatch.setattr(hv, "_rows_blocks", fake_rows_blocks(launches))
    rng = np.random.RandomState(2)
    X = rng.normal(size=(30, 2))
    Y = X[:, :1] + 0.5 * rng.normal(size=(30, 1))
    side = np.geomspace(0.05, 20.0, 2 * S + 3)
    grid = [(float(s), float(s)) for s in side]
    sel = hv.select_sigma(X, Y, grid)
    assert launches == [S, S, 3]  # launches of the native maximum, then the rest
    index, crit, value, var = o_select(X, Y, grid)
    assert sel.index == index and sel.sigma == grid[index] and isinstance(sel.sigma, tuple)
    assert all(isinstance(t, float) for t in sel.sigma)
    assert np.allclose(sel.criterion, crit, rtol=1e-9, atol=0)
    assert np.allclose(sel.value, value, rtol=0, atol=1e-13) and np.allclose(sel.var, var, rtol=1e-9)
    assert sel.criterion.shape == sel.value.shape == sel.var.shape == (2 * S + 3,)
    assert 0 < index < 2 * S + 2  # an interior maximum: the grid brackets the planted scale
    # an (S, 2) array is the same grid
    arr = hv.select_sigma(X, Y, np.array(grid))
    assert arr.index == index and np.array_equal(arr.criterion, sel.criterion)
    # reg enters as stated
    big = hv.select_sigma(X, Y, grid, reg=4.0)
    assert np.allclose(big.criterion, value / np.sqrt(var + 4.0), rtol=1e-9, atol=0)
    # ties: the first wins
    tie = hv.select_sigma(X, Y, [(0.3, 0.3), grid[index], (7.0, 7.0), grid[index]])
    assert tie.index == 1 and tie.criterion[1] == tie.criterion[3]
    # a NaN criterion never wins; all NaN is an error
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        hv.select_sigma(Xn, Y, [(0.5, 0.5), (1.0, 1.0)])
    real = hv._variance

    def nan_at_the_best(p, k, l, u, v):  # noqa: E741
        r = real(p, k, l, u, v)
        value = r.value.copy()
        value[index] = np.nan
        return r._replace(value=value)

    monkeypatch.setattr(hv, "_variance", nan_at_the_best)
    masked = hv.select_sigma(X, Y, grid)
    c = crit.copy()
    c[index] = np.nan
    assert masked.index == int(np.nanargmax(c)) != index and np.isnan(masked.criterion[index])


@pytest.mark.parametrize("kernel", KERNELS)
def test_UnN_var_is_UnN_with_a_variance(tw, monkeypatch, kernel):
    import tuplewise.hsic as hs
    import tuplewise.hsic_var as hv
    sigma = (1.3, 0.8) if kernel == "gaussian" else None
    launches = []
    monkeypatch.setattr(hv, "_rows_blocks", fake_rows_blocks(launches))

    def sums_blocks(Xf, Yf, off, kid, cx, cy, want_rows=False, group=0):  # hsic's glue, oracle
        return np.array([o_components(Xf[off[b]:off[b + 1]], Yf[off[b]:off[b + 1]], kernel, sigma)
                         for b in range(len(off) - 1)]), None

    monkeypatch.setattr(hs, "_sums_blocks", sums_blocks)
    X, Y = paired(41, 3, 2, 6)
    N = 4
    X1, Y1, X2, Y2, X3, Y3 = X.copy(), Y.copy(), X.copy(), Y.copy(), X.copy(), Y.copy()
    np.random.seed(77)
    value, var = hv.UnN_var(X1, Y1, N, kernel=kernel, sigma=sigma)
    s1 = np.random.get_state()
    np.random.seed(77)
    want = hs.UnN(X2, Y2, N, kernel=kernel, sigma=sigma)
    s2 = np.random.get_state()
    np.random.seed(77)
    o_value, o_var = o_UnN_var(X3, Y3, N, kernel, sigma)
    assert launches == [1]  # all N blocks in one pair of launches of one sigma pair
    assert isinstance(value, np.float64) and isinstance(var, np.float64)
    assert abs(value - want) <= 1e-13 and abs(value - o_value) <= 1e-13
    assert abs(var - o_var) <= 1e-11 * o_var and var > 0
    assert same_state(s1, s2) and same_state(s1, np.random.get_state())
    assert np.array_equal(X1, X2) and np.array_equal(Y1, Y2) and not np.array_equal(X1, X)
    assert np.array_equal(X1, X3) and np.array_equal(Y1, Y3)
