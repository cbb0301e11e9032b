"""tuplewise.mmd's permutation test without a GPU: the NumPy oracles the GPU tests compare against
(o_perm_sums calls o_components of tests/test_mmd_cpu.py on every relabelled pool; o_perm_test
draws with np.random.permutation), the oracle against the identities the kernel uses on a full
Gram matrix, every argument error before any draw or device work, and the native entry points'
argument checks."""
import ctypes
import math

import numpy as np
import pytest

from test_mmd_cpu import KERNELS, o_components, o_g, o_sign
from test_triplets_cpu import data, o_dist_rows, same_state


# ------------------------------------------------------------------------------------ oracle
def o_perm_sums(X, Z, labels, kernel, sigma=None):
    """(P, 3): o_components of the pool [X; Z] relabelled by every row of labels (the rows a label
    marks are the first sample, in pool order)."""
    W = np.concatenate([X.reshape(len(X), -1), Z.reshape(len(Z), -1)])
    return np.array([o_components(W[s], W[~s], kernel, sigma) for s in labels], dtype=np.float64)


def o_value(s, n, m, kernel):
    return np.float64(o_sign(kernel) * (2.0 * s[0] / (n * (n - 1)) + 2.0 * s[1] / (m * (m - 1))
                                        - 2.0 * s[2] / (n * m)))


def o_scale(s, n, m):
    """The magnitude a value's tolerance is taken from: the sum of |terms| of V (§4.12)."""
    return abs(2.0 * s[0] / (n * (n - 1))) + abs(2.0 * s[1] / (m * (m - 1))) + abs(2.0 * s[2] / (n * m))


def o_perm_labels(n, m, n_perm):
    """Row 0 the observed split, rows 1 .. n_perm from np.random.permutation(n + m)[:n]."""
    labels = np.zeros((n_perm + 1, n + m), dtype=bool)
    labels[0, :n] = True
    for p in range(1, n_perm + 1):
        labels[p, np.random.permutation(n + m)[:n]] = True
    return labels


def o_perm_test(X, Z, n_perm, kernel, sigma=None):
    """(statistic, null, pvalue, scales): the test restated with the oracle's sums; scales[p] is
    the tolerance magnitude of column p (0 the observed one)."""
    n, m = len(X), len(Z)
    sums = o_perm_sums(X, Z, o_perm_labels(n, m, n_perm), kernel, sigma)
    values = np.array([o_value(s, n, m, kernel) for s in sums])
    scales = np.array([o_scale(s, n, m) for s in sums])
    stat, null = values[0], values[1:]
    return stat, null, (1 + int(np.sum(null >= stat))) / (1 + n_perm), scales


def random_labels(rng, P, n, N):
    labels = np.zeros((P, N), dtype=bool)
    for p in range(P):
        labels[p, rng.permutation(N)[:n]] = True
    return labels


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("kernel", KERNELS)
def test_oracle_is_the_gram_identities(kernel):
    """Sxx = sum_{i<j} s_i s_j g_ij, A = sum_i s_i r_i, Sxz = A - 2 Sxx, Szz = T - A + Sxx on the
    full Gram matrix, at 1e-13 of T."""
    n, m, P = 5, 6, 8
    X, Z = data("gauss", n, m, 3, 12)
    sigma = 1.4 if kernel == "gaussian" else None
    labels = random_labels(np.random.RandomState(3), P, n, n + m)
    labels[0] = False
    labels[0, :n] = True
    W = np.concatenate([X, Z])
    G = o_g(o_dist_rows(W, W), kernel, sigma)
    np.fill_diagonal(G, 0.0)
    r = G.sum(axis=1)
    T = 0.5 * r.sum()
    got = o_perm_sums(X, Z, labels, kernel, sigma)
    assert np.array_equal(got[0], o_components(X, Z, kernel, sigma))
    for p in range(P):
        s = labels[p].astype(np.float64)
        sxx = 0.5 * (s @ G @ s)
        A = s @ r
        want = np.array([sxx, T - A + sxx, A - 2.0 * sxx])
        assert np.all(np.abs(got[p] - want) <= 1e-13 * T), (p, got[p], want)


@pytest.mark.parametrize("kernel", KERNELS)
def test_oracle_test_is_numpy_permutations(kernel):
    n, m, d, P = 7, 5, 2, 9
    X, Z = data("gauss", n, m, d, 4)
    sigma = 1.1 if kernel == "gaussian" else None
    np.random.seed(3)
    stat, null, pvalue, scales = o_perm_test(X, Z, P, kernel, sigma)
    state = np.random.get_state()
    np.random.seed(3)
    W = np.concatenate([X, Z])
    want = []
    for _ in range(P):
        pi = np.random.permutation(n + m)
        a, b = W[np.sort(pi[:n])], W[np.sort(pi[n:])]
        want.append(o_value(o_components(a, b, kernel, sigma), n, m, kernel))
    assert same_state(state, np.random.get_state())
    assert np.array_equal(null, np.array(want)) and null.shape == (P,) and scales.shape == (P + 1,)
    assert stat == o_value(o_components(X, Z, kernel, sigma), n, m, kernel)
    assert pvalue == (1 + sum(v >= stat for v in want)) / (1 + P) and 1 / (1 + P) <= pvalue <= 1


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.mmd as mm
    assert callable(mm.permutation_sums) and callable(mm.permutation_test)
    r = mm.PermutationResult(np.float64(1.0), np.zeros(3), 0.25)
    assert r.statistic == 1.0 and r.null.shape == (3,) and r.pvalue == 0.25


def test_argument_errors_need_no_device(tw):
    import tuplewise.mmd as mm
    X, Z = np.arange(40.0).reshape(10, 4), np.arange(24.0).reshape(6, 4) + 0.5
    X0, Z0 = X.copy(), Z.copy()
    x1 = np.arange(10.0)
    wide = np.zeros((4, 65))
    E = dict(kernel="energy")
    G = dict(sigma=1.0)
    ok = np.zeros((3, 16), dtype=bool)
    ok[:, :10] = True
    few, many = ok.copy(), ok.copy()
    few[1, 0] = False
    many[2, 12] = True
    state = np.random.get_state()
    calls = [
        # labels: not an array, dtype, rank, width, no rows, a wrong count in one row
        lambda: mm.permutation_sums(X, Z, ok.tolist(), **E),
        lambda: mm.permutation_sums(X, Z, ok.astype(np.uint8), **E),
        lambda: mm.permutation_sums(X, Z, ok.astype(np.float64), **G),
        lambda: mm.permutation_sums(X, Z, ok[0], **E),
        lambda: mm.permutation_sums(X, Z, ok[:, :15], **G),
        lambda: mm.permutation_sums(X, Z, ok.T.copy(), **E),
        lambda: mm.permutation_sums(X, Z, ok[:0], **E),
        lambda: mm.permutation_sums(X, Z, few, **E), lambda: mm.permutation_sums(X, Z, many, **G),
        lambda: mm.permutation_sums(X, Z, ~ok, **E),
        # n_perm
        lambda: mm.permutation_test(X, Z, 0, **E), lambda: mm.permutation_test(X, Z, -1, **G),
        lambda: mm.permutation_test(X, Z, 2.5, **E), lambda: mm.permutation_test(X, Z, None, **E),
        lambda: mm.permutation_test(X, Z, True, **G), lambda: mm.permutation_test(X, Z, "3", **E),
        # the _check cases: dtype, layout, rank, d, rows, the kernel and its sigma
        lambda: mm.permutation_test(X.astype(np.float32), Z, 3, **E),
        lambda: mm.permutation_sums(X, Z.astype(np.int64), ok, **G),
        lambda: mm.permutation_test(X[:, ::2], Z[:, ::2], 3, **E),
        lambda: mm.permutation_sums(X.T, Z.T, ok, **G),
        lambda: mm.permutation_test(X.reshape(5, 2, 4), Z, 3, **E),
        lambda: mm.permutation_test(X, x1, 3, **E), lambda: mm.permutation_test(wide, wide, 3, **G),
        lambda: mm.permutation_sums(wide, wide, np.ones((1, 8), dtype=bool), **E),
        lambda: mm.permutation_test(np.zeros((4, 0)), np.zeros((3, 0)), 3, **E),
        lambda: mm.permutation_test(X[:1], Z, 3, **E), lambda: mm.permutation_test(X, Z[:1], 3, **G),
        lambda: mm.permutation_sums(X[:1], Z, ok[:, :7], **E),
        lambda: mm.permutation_test(X, Z, 3, kernel="laplace", sigma=1.0),
        lambda: mm.permutation_test(X, Z, 3), lambda: mm.permutation_sums(X, Z, ok),
        lambda: mm.permutation_test(X, Z, 3, sigma=0.0), lambda: mm.permutation_test(X, Z, 3, sigma=-1.0),
        lambda: mm.permutation_sums(X, Z, ok, sigma=float("nan")),
        lambda: mm.permutation_test(X, Z, 3, sigma=float("inf")),
        lambda: mm.permutation_test(X, Z, 3, sigma="wide"),
        lambda: mm.permutation_test(X, Z, 3, kernel="energy", sigma=1.0),
        lambda: mm.permutation_sums(X, Z, ok, kernel="energy", sigma=2),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), k
    with pytest.raises(ValueError, match="n_perm"):
        mm.permutation_test(X, Z, 0, **E)
    with pytest.raises(ValueError, match="marks 9 rows"):
        mm.permutation_sums(X, Z, few, **E)
    with pytest.raises(ValueError, match="bool"):
        mm.permutation_sums(X, Z, ok.astype(np.int8), **E)
    assert np.array_equal(X, X0) and np.array_equal(Z, Z0)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.mmd as mm
    X, Z = data("gauss", 6, 4, 3, 0)
    labels = np.zeros((2, 10), dtype=bool)
    labels[:, :6] = True
    state = np.random.get_state()
    with pytest.raises(RuntimeError, match="no HIP device"):
        mm.permutation_sums(X, Z, labels, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        mm.permutation_test(X, Z, 5, kernel="energy")
    assert same_state(np.random.get_state(), state)  # nothing drawn for a device that is not there


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")

    def sums(w=p, n_rows=4, d=3, labels=p, n_perm=1, kern=L.TW_MMD_GAUSSIAN, c=-0.5, work=p, out=p):
        return lib.tw_mmd_perm_sums(w, n_rows, d, labels, n_perm, kern, c, work, out, None)

    G, E = dict(kern=L.TW_MMD_GAUSSIAN), dict(kern=L.TW_MMD_ENERGY)
    for call, word in ((lambda: sums(w=None), b"null pointer"),
                       (lambda: sums(labels=None), b"null pointer"),
                       (lambda: sums(work=None), b"null pointer"),
                       (lambda: sums(out=None), b"null pointer"),
                       (lambda: sums(d=0), b"outside [1, 64]"),
                       (lambda: sums(d=65, **E), b"outside [1, 64]"),
                       (lambda: sums(n_rows=3), b"n_rows"),
                       (lambda: sums(n_rows=0, **E), b"n_rows"),
                       (lambda: sums(n_rows=-5), b"n_rows"),
                       (lambda: sums(n_rows=2 ** 31), b"n_rows"),
                       (lambda: sums(n_perm=0), b"n_perm"),
                       (lambda: sums(n_perm=-1, **E), b"n_perm"),
                       (lambda: sums(kern=2), b"unknown kernel"),
                       (lambda: sums(kern=-1), b"unknown kernel"),
                       (lambda: sums(c=0.5, **G), b"Gaussian"),
                       (lambda: sums(c=nan, **G), b"Gaussian"),
                       (lambda: sums(c=-inf, **G), b"Gaussian"),
                       (lambda: sums(c=inf, **G), b"Gaussian"),
                       # 2^30 rows are 2^23 tiles: 512 workgroups a pass, 2^24 passes
                       (lambda: sums(n_rows=2 ** 30, n_perm=2 ** 31 - 1, **E), b"grid too large")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_mmd_perm_sums" in msg, msg
    with pytest.raises(ValueError, match="n_perm"):
        L.call("tw_mmd_perm_sums", p, 4, 3, p, 0, L.TW_MMD_ENERGY, 0.0, p, p, None)
    C = lib.tw_mmd_perm_cols()
    assert C % 16 == 0 and 16 <= C <= 4096
    wb = lib.tw_mmd_perm_work_bytes
    assert wb(3, 1) == 0 and wb(4, 0) == 0 and wb(-1, 5) == 0 and wb(2 ** 31, 1) == 0
    small = wb(4, 1)
    assert small >= 3 * 8 and small % 8 == 0
    # whole passes of C columns: the same inside a pass, more past it, and more rows never less
    assert wb(4, C) == small and wb(4, C + 1) == 2 * small and wb(4, 2 * C + 1) == 3 * small
    T = lib.tw_mmd_tile()
    assert wb(T + 1, 1) == 3 * small  # three tile pairs, one workgroup each
    assert small <= wb(20000, 1000) < 1 << 28
    assert math.isfinite(wb(2 ** 31 - 1, 1)) and wb(2 ** 31 - 1, 1) >= wb(20000, 1)
