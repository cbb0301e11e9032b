"""tuplewise.hsic_perm (the permutation test of tuplewise.hsic's statistic) without a GPU: the NumPy oracle the GPU tests compare against
(S_p and Rab_p are S_KL and R_KL of tests/test_hsic_cpu.py's o_components on (X, Y[pi]), by
math.fsum), the oracle against the brute-force mean over ordered 4-tuples and against the
moved-X form with the inverse permutation, the oracle's test against np.random.permutation's
order and final state, every argument error of permutation_sums / permutation_test before any
device work or RNG draw, and the native entry's argument checks."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from test_hsic_cpu import (KERNELS, o_components, o_fsum, o_KL, o_row_sums, o_U, o_U_scale, paired,
                           sig)
from test_triplets_cpu import same_state


# ------------------------------------------------------------------------------------ oracle
def o_perm_sums_literal(X, Y, perms, kernel, sigma=None):
    """(P, 2): S_KL and R_KL of o_components on the sample (X[i], Y[perms[p, i]]), row by row."""
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    out = np.empty((len(perms), 2))
    for p, pi in enumerate(np.asarray(perms)):
        c = o_components(X, Y[pi], kernel, sigma)
        out[p] = c[0], c[5]
    return out


def o_perm_sums(X, Y, perms, kernel, sigma=None):
    """The same doubles with K, L and the row sums formed once: L of (X, Y[pi]) is L[pi][:, pi]
    (the same distances of the same rows) and its row sums are l[pi] (fsum of the same terms), so
    every fsum below meets the terms o_perm_sums_literal's meets."""
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    K, L = o_KL(X, Y, kernel, sigma)
    k, l = o_row_sums(X, Y, kernel, sigma)  # noqa: E741
    iu = np.triu_indices(len(X), 1)
    Ku = K[iu]
    out = np.empty((len(perms), 2))
    with np.errstate(invalid="ignore"):
        for p, pi in enumerate(np.asarray(perms)):
            out[p] = o_fsum(Ku * L[pi][:, pi][iu]), o_fsum(k * l[pi])
    return out


def o_perm_values(X, Y, perms, kernel, sigma=None):
    """((P,) values, (P,) scales): U(S_p, R_K, R_L, Rab_p) with the two invariant R of the
    unpermuted sample, and the magnitude a value's tolerance is taken from."""
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    n = len(X)
    c = o_components(X, Y, kernel, sigma)
    s = o_perm_sums(X, Y, perms, kernel, sigma)
    return (np.array([o_U(sp, c[3], c[4], rab, n) for sp, rab in s]),
            np.array([o_U_scale(sp, c[3], c[4], rab, n) for sp, rab in s]))


def o_perm_test(X, Y, n_perm, kernel, sigma=None):
    """(statistic, null, pvalue, perms): permutation p = 1 .. n_perm is np.random.permutation(n),
    column 0 the identity."""
    n = len(X)
    perms = np.stack([np.arange(n)] + [np.random.permutation(n) for _ in range(n_perm)])
    values = o_perm_values(X, Y, perms, kernel, sigma)[0]
    stat, null = values[0], values[1:]
    return stat, null, (1 + int(np.count_nonzero(null >= stat))) / (1 + n_perm), perms


def some_perms(n, P, seed):
    """(P, n): the identity, the reversal, the rotation by one, then seeded random ones."""
    rng = np.random.RandomState(seed)
    rows = [np.arange(n), np.arange(n)[::-1], np.roll(np.arange(n), -1)]
    rows += [rng.permutation(n) for _ in range(max(0, P - 3))]
    return np.stack(rows[:P]).astype(np.int64)


def inverse(perms):
    inv = np.empty_like(perms)
    inv[np.arange(len(perms))[:, None], perms] = np.arange(perms.shape[1])
    return inv


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [5, 7])
def test_oracle_is_the_mean_over_ordered_4_tuples_of_the_permuted_sample(kernel, n):
    X, Y = paired(n, 3, 2, n)
    s = sig(kernel, 3, 2)
    perms = some_perms(n, 6, n)
    values, scales = o_perm_values(X, Y, perms, kernel, s)
    for p, pi in enumerate(perms):
        K, L = o_KL(X, Y[pi], kernel, s)
        terms = [K[i, j] * (L[i, j] + L[q, r] - 2.0 * L[i, q])
                 for i, j, q, r in itertools.permutations(range(n), 4)]
        want = math.fsum(terms) / len(terms)
        assert abs(values[p] - want) <= 1e-13 * scales[p], (p, values[p], want)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", ["gauss", "ties", "nan"])
def test_oracle_is_o_components_of_the_permuted_sample(kernel, kind):
    n = 37
    X, Y = paired(n, 4, 3, 2, kind)
    s = sig(kernel, 4, 3)
    perms = some_perms(n, 8, 1)
    got, want = o_perm_sums(X, Y, perms, kernel, s), o_perm_sums_literal(X, Y, perms, kernel, s)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) or (
        kind == "nan" and np.isnan(got).all() and np.isnan(want).all())
    # a NaN coordinate on the other side as well
    if kind == "nan":
        got = o_perm_sums(Y, X, perms, kernel, (s[1], s[0]) if s else None)
        assert np.isnan(got).all()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dx,dy,n", [(3, 2, 7), (2, 5, 23)])
def test_oracle_moved_x_form(kernel, dx, dy, n):
    """Moving X by the inverse permutation gives the same two sums: sum_{a<b} L_ab K_{s a, s b}
    and sum_a l_a k_{s a}, s = pi^-1 (the same products in another order; fsum is exact)."""
    X, Y = paired(n, dx, dy, 3 * n)
    s = sig(kernel, dx, dy)
    perms = some_perms(n, 7, n)
    want = o_perm_sums(X, Y, perms, kernel, s)
    sw = (s[1], s[0]) if s else None
    got = o_perm_sums(Y, X, inverse(perms), kernel, sw)
    assert np.all(np.abs(got - want) <= 1e-15 * np.abs(want)), (got, want)
    # the identity column is the unpermuted sample's S_KL and R_KL
    c = o_components(X, Y, kernel, s)
    assert want[0, 0] == c[0] and want[0, 1] == c[5]


def test_oracle_test_draws_in_numpy_order():
    n, n_perm = 11, 13
    X, Y = paired(n, 2, 2, 4)
    np.random.seed(17)
    stat, null, pvalue, perms = o_perm_test(X, Y, n_perm, "distance")
    state = np.random.get_state()
    np.random.seed(17)
    want = [np.random.permutation(n) for _ in range(n_perm)]
    assert same_state(state, np.random.get_state())
    assert np.array_equal(perms[0], np.arange(n)) and np.array_equal(perms[1:], np.stack(want))
    c = o_components(X, Y, "distance")
    assert stat == o_U(c[0], c[3], c[4], c[5], n)
    for p in range(n_perm):
        cp = o_components(X, Y[want[p]], "distance")
        assert null[p] == o_U(cp[0], c[3], c[4], cp[5], n)
        # R_K and R_L do not move under a permutation
        assert abs(cp[3] - c[3]) <= 1e-15 * c[3] and abs(cp[4] - c[4]) <= 1e-15 * c[4]
    assert pvalue == (1 + sum(v >= stat for v in null)) / (1 + n_perm)
    assert 1 / (1 + n_perm) <= pvalue <= 1.0


def test_oracle_separates_dependent_from_independent():
    """The seeded pairs of tests/test_gpu_hsic_perm.py, on the oracle alone."""
    for kernel in KERNELS:
        X, Y = paired(60, 2, 2, 12)
        s = sig(kernel, 2, 2)
        np.random.seed(1)
        assert o_perm_test(X, Y, 19, kernel, s)[2] == 0.05
        Z = np.random.RandomState(13).normal(size=Y.shape)
        np.random.seed(1)
        assert o_perm_test(X, Z, 19, kernel, s)[2] > 0.05


# ------------------------------------------------------------------------ the module, no GPU
def test_module_has_the_permutation_test(tw):
    import tuplewise.hsic_perm as hs
    import tuplewise.mmd as mm
    assert callable(hs.permutation_sums) and callable(hs.permutation_test)
    assert hs.PermutationResult._fields == mm.PermutationResult._fields == ("statistic", "null",
                                                                            "pvalue")
    assert int(tw._lib.lib().tw_hsic_perm_cols()) >= 1


def test_argument_errors_need_no_device(tw):
    import tuplewise.hsic_perm as hs
    n = 12
    X, Y = np.arange(48.0).reshape(n, 4), np.arange(36.0).reshape(n, 3) + 0.5
    X0, Y0 = X.copy(), Y.copy()
    wide = np.zeros((6, 65))
    D = dict(kernel="distance")
    G = dict(sigma=1.0)
    good = some_perms(n, 4, 0)
    rep, out, neg = good.copy(), good.copy(), good.copy()
    rep[2, 5] = rep[2, 6]
    out[3, 0] = n
    neg[1, 3] = -1
    state = np.random.get_state()
    calls = [
        # bad shapes, dtype, layout
        lambda: hs.permutation_test(X.astype(np.float32), Y, 5, **D),
        lambda: hs.permutation_test(X[:, ::2], Y, 5, **G),
        lambda: hs.permutation_test(X.reshape(6, 2, 4), Y[:6], 5, **D),
        lambda: hs.permutation_test(wide, Y[:6], 5, **G),
        lambda: hs.permutation_test(X, np.zeros((n, 0)), 5, **D),
        lambda: hs.permutation_test(X, Y[:11], 5, **D),
        lambda: hs.permutation_sums(X, Y.astype(np.int64), good, **D),
        lambda: hs.permutation_sums(X, Y[:11], good, **G),
        lambda: hs.permutation_sums(wide, Y[:6], good[:, :6], **D),
        # n < 4
        lambda: hs.permutation_test(X[:3], Y[:3], 5, **D),
        lambda: hs.permutation_test(X[:0], Y[:0], 5, **G),
        lambda: hs.permutation_sums(X[:3], Y[:3], np.arange(3).reshape(1, 3), **D),
        # n_perm < 1 or not an integer
        lambda: hs.permutation_test(X, Y, 0, **D), lambda: hs.permutation_test(X, Y, -3, **G),
        lambda: hs.permutation_test(X, Y, 2.0, **D), lambda: hs.permutation_test(X, Y, "9", **D),
        lambda: hs.permutation_test(X, Y, None, **G), lambda: hs.permutation_test(X, Y, True, **D),
        lambda: hs.permutation_test(X, Y, 2 ** 31 - 1, **D),
        # a perms row with a repeat, an out-of-range entry, the wrong length; not an integer array
        lambda: hs.permutation_sums(X, Y, rep, **D), lambda: hs.permutation_sums(X, Y, out, **G),
        lambda: hs.permutation_sums(X, Y, neg, **D),
        lambda: hs.permutation_sums(X, Y, good[:, :n - 1], **D),
        lambda: hs.permutation_sums(X, Y, np.concatenate([good, good], axis=1), **G),
        lambda: hs.permutation_sums(X, Y, good[0], **D),
        lambda: hs.permutation_sums(X, Y, good[:0], **D),
        lambda: hs.permutation_sums(X, Y, good.astype(np.float64), **G),
        lambda: hs.permutation_sums(X, Y, good.tolist(), **D),
        lambda: hs.permutation_sums(X, Y, good.astype(bool), **D),
        # a bad kernel or sigma
        lambda: hs.permutation_test(X, Y, 5, kernel="laplace", sigma=1.0),
        lambda: hs.permutation_test(X, Y, 5), lambda: hs.permutation_test(X, Y, 5, sigma=0.0),
        lambda: hs.permutation_test(X, Y, 5, sigma=(1.0,)),
        lambda: hs.permutation_test(X, Y, 5, sigma=float("nan")),
        lambda: hs.permutation_test(X, Y, 5, kernel="distance", sigma=1.0),
        lambda: hs.permutation_sums(X, Y, good, kernel=None),
        lambda: hs.permutation_sums(X, Y, good), lambda: hs.permutation_sums(X, Y, good, sigma=-1.0),
        lambda: hs.permutation_sums(X, Y, good, sigma=(1.0, float("inf"))),
        lambda: hs.permutation_sums(X, Y, good, kernel="distance", sigma=(1.0, 2.0)),
    ]
    for k, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), k
    with pytest.raises(ValueError, match="repeats a row"):
        hs.permutation_sums(X, Y, rep, **D)
    with pytest.raises(ValueError, match=r"perms\[3\] has an entry outside"):
        hs.permutation_sums(X, Y, out, **D)
    with pytest.raises(ValueError, match="n_perm"):
        hs.permutation_test(X, Y, 0, **D)
    # a shape tw_hsic_sums refuses: before any draw
    big = np.zeros(300_000)
    with pytest.raises(ValueError, match="work budget"):
        hs.permutation_test(big, big.copy(), 3, **D)
    assert same_state(np.random.get_state(), state)
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.hsic_perm as hs
    X, Y = paired(6, 3, 2, 0)
    state = np.random.get_state()
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.permutation_test(X, Y, 5, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.permutation_test(Y, X, 5, kernel="distance")
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.permutation_sums(X, Y, some_perms(6, 3, 0), kernel="distance")
    assert same_state(np.random.get_state(), state)  # nothing was drawn


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")
    wb = lib.tw_hsic_perm_work_bytes
    C = int(lib.tw_hsic_perm_cols())
    T = int(lib.tw_hsic_tile())
    assert C >= 1

    def sums(held=p, d_h=3, moved=p, d_m=2, n=4, idx=p, n_cols=1, rh=p, rm=p,
             kern=L.TW_HSIC_GAUSSIAN, ch=-0.5, cm=-0.25, wgs=0, work=p, out=p):
        return lib.tw_hsic_perm_sums(held, d_h, moved, d_m, n, idx, n_cols, rh, rm, kern, ch, cm,
                                     wgs, work, out, None)

    for call, word in ([(lambda k=k: sums(**{k: None}), b"null pointer")
                        for k in ("held", "moved", "idx", "rh", "rm", "work", "out")] +
                       [(lambda: sums(d_h=0), b"d_h 0 outside [1, 64]"),
                        (lambda: sums(d_h=65), b"d_h 65 outside [1, 64]"),
                        (lambda: sums(d_m=0), b"d_m 0 outside [1, 64]"),
                        (lambda: sums(d_m=65), b"d_m 65 outside [1, 64]"),
                        (lambda: sums(n=3), b"n 3 outside"),
                        (lambda: sums(n=0), b"n 0 outside"),
                        (lambda: sums(n=-1), b"outside"),
                        (lambda: sums(n=2 ** 31), b"outside"),
                        (lambda: sums(n_cols=0), b"n_cols 0 < 1"),
                        (lambda: sums(n_cols=-5), b"n_cols -5 < 1"),
                        (lambda: sums(kern=2), b"unknown kernel"),
                        (lambda: sums(kern=-1), b"unknown kernel"),
                        (lambda: sums(ch=0.5), b"Gaussian"), (lambda: sums(cm=0.5), b"Gaussian"),
                        (lambda: sums(ch=nan), b"Gaussian"), (lambda: sums(cm=nan), b"Gaussian"),
                        (lambda: sums(ch=-inf), b"Gaussian"), (lambda: sums(cm=inf), b"Gaussian"),
                        (lambda: sums(wgs=-1), b"wgs -1 < 0"),
                        (lambda: sums(n=2 ** 31 - 1, n_cols=2 ** 31 - 1), b"grid too large")]):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_hsic_perm_sums" in msg, msg
    with pytest.raises(ValueError, match="unknown kernel"):
        L.call("tw_hsic_perm_sums", p, 3, p, 2, 4, p, 1, p, p, 7, -0.5, -0.5, 0, p, p, None)
    # the work size is 0 exactly where the entry refuses on (n, n_cols, wgs)
    for n, cols, wgs in ((3, 1, 0), (0, 1, 0), (-1, 1, 0), (2 ** 31, 1, 0), (4, 0, 0), (4, -5, 0),
                         (4, 1, -1), (2 ** 31 - 1, 2 ** 31 - 1, 0)):
        assert wb(n, cols, wgs) == 0, (n, cols, wgs)
        assert sums(n=n, n_cols=cols, wgs=wgs) == L.TW_ERR_ARG
    # one double per workgroup and column: the plan depends on n and wgs alone
    assert wb(4, 1, 0) == 8 * C and wb(4, C, 0) == 8 * C and wb(4, C + 1, 0) == 16 * C
    n = 4 * T + 5  # 5 tiles, 15 tile pairs
    assert [wb(n, 1, w) // (8 * C) for w in (0, 1, 2, 4, 15, 16, 1000)] == [15, 1, 2, 4, 15, 15, 15]
    assert wb(n, 2 * C + 1, 4) == 3 * 4 * 8 * C
    assert wb(10 ** 4, 1, 0) // (8 * C) <= 512 < wb(10 ** 4, 1, 10 ** 4) // (8 * C)
