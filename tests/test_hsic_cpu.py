"""tuplewise.hsic without a GPU: the NumPy oracle the GPU tests compare against (distances by the
oracle of tests/test_triplets_cpu.py, the eight sums by math.fsum over the terms, row sums by
fsum per row, the estimators restated literally with the same np.random calls in the same order),
the oracle against the brute-force mean over ordered 4-tuples and the U-centred inner product,
the 4-tuple draw, the paired shuffle, every argument error before any device work or RNG draw,
and the native entry points' argument checks."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from test_triplets_cpu import o_dist_pairs, o_dist_rows, same_state

KERNELS = ["gaussian", "distance"]
NAMES = ("S_KL", "S_KK", "S_LL", "R_K", "R_L", "R_KL", "R_KK", "R_LL")


# ------------------------------------------------------------------------------------ oracle
def o_sigmas(sigma):
    return tuple(sigma) if isinstance(sigma, (tuple, list)) else (sigma, sigma)


def o_g(D, kernel, sigma):
    """g of an array of squared distances: np.exp(D * c) or np.sqrt(D)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if kernel == "gaussian":
            return np.exp(D * (-1.0 / (2.0 * sigma * sigma)))
        return np.sqrt(D)


def o_fsum(terms):
    """math.fsum of the terms, NaN if any term is NaN."""
    terms = np.asarray(terms, dtype=np.float64).reshape(-1)
    if np.isnan(terms).any():
        return float("nan")
    return math.fsum(terms.tolist())


def o_KL(X, Y, kernel, sigma=None):
    """The (n, n) matrices K and L, zero diagonals."""
    sx, sy = o_sigmas(sigma)
    K, L = o_g(o_dist_rows(X, X), kernel, sx), o_g(o_dist_rows(Y, Y), kernel, sy)
    np.fill_diagonal(K, 0.0)
    np.fill_diagonal(L, 0.0)
    return K, L


def o_row_sums(X, Y, kernel, sigma=None):
    K, L = o_KL(X, Y, kernel, sigma)
    return (np.array([o_fsum(row) for row in K]), np.array([o_fsum(row) for row in L]))


def o_components(X, Y, kernel, sigma=None):
    """(S_KL, S_KK, S_LL, R_K, R_L, R_KL, R_KK, R_LL), every sum an fsum of its terms."""
    K, L = o_KL(X, Y, kernel, sigma)
    iu = np.triu_indices(len(K), 1)
    k, l = o_row_sums(X, Y, kernel, sigma)  # noqa: E741
    with np.errstate(invalid="ignore"):
        return (o_fsum(K[iu] * L[iu]), o_fsum(K[iu] * K[iu]), o_fsum(L[iu] * L[iu]),
                o_fsum(k), o_fsum(l), o_fsum(k * l), o_fsum(k * k), o_fsum(l * l))


def o_U(s, ra, rb, rab, n):
    return (2.0 * s + ra * rb / ((n - 1) * (n - 2)) - 2.0 * rab / (n - 2)) / (n * (n - 3))


def o_U_scale(s, ra, rb, rab, n):
    """The magnitude a statistic's tolerance is taken from: the sum of |terms| of U."""
    return (abs(2.0 * s) + abs(ra * rb) / ((n - 1) * (n - 2)) + abs(2.0 * rab) / (n - 2)) / (n * (n - 3))


def o_three(X, Y, kernel, sigma=None):
    """((v_xy, scale), (v_xx, scale), (v_yy, scale)): the three statistics correlation uses."""
    c, n = o_components(X, Y, kernel, sigma), len(X)
    args = ((c[0], c[3], c[4], c[5]), (c[1], c[3], c[3], c[6]), (c[2], c[4], c[4], c[7]))
    return tuple((o_U(*a, n), o_U_scale(*a, n)) for a in args)


def o_Un(X, Y, kernel, sigma=None):
    return np.float64(o_three(X, Y, kernel, sigma)[0][0])


def o_Un_scale(X, Y, kernel, sigma=None):
    return o_three(X, Y, kernel, sigma)[0][1]


def o_correlation(X, Y, kernel, sigma=None):
    (vxy, _), (vxx, _), (vyy, _) = o_three(X, Y, kernel, sigma)
    return np.float64(vxy / math.sqrt(vxx * vyy)) if vxx * vyy > 0.0 else np.float64("nan")


def o_idx_sums(X, Y, i, j, q, r, kernel, sigma=None):
    """(A, B, C) = sums of K_ij L_ij, K_ij L_qr, K_ij L_iq."""
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    sx, sy = o_sigmas(sigma)
    kij = o_g(o_dist_pairs(X[i], X[j]), kernel, sx)
    with np.errstate(invalid="ignore"):
        return tuple(o_fsum(kij * o_g(o_dist_pairs(Y[a], Y[b]), kernel, sy))
                     for a, b in ((i, j), (q, r), (i, q)))


def o_UB_indices(X, Y, i, j, q, r, kernel, sigma=None):
    if len(i) == 0:
        return np.float64("nan")
    a, b, c = o_idx_sums(X, Y, i, j, q, r, kernel, sigma)
    return np.float64((a + b - 2.0 * c) / len(i))


def o_UB_scale(X, Y, i, j, q, r, kernel, sigma=None):
    a, b, c = o_idx_sums(X, Y, i, j, q, r, kernel, sigma)
    return (a + b + 2.0 * c) / len(i)


def o_map(a0, a1, a2, a3):
    """Four distinct rows from the four draws: each later one stepped past the earlier ones in
    ascending order, one element at a time."""
    out = []
    for t in zip(np.asarray(a0).tolist(), np.asarray(a1).tolist(), np.asarray(a2).tolist(),
                 np.asarray(a3).tolist()):
        i = t[0]
        j = t[1] + (t[1] >= i)
        q = t[2]
        for v in sorted((i, j)):
            q += q >= v
        r = t[3]
        for v in sorted((i, j, q)):
            r += r >= v
        out.append((i, j, q, r))
    return tuple(np.array(c, dtype=np.int64) for c in zip(*out)) if out else (np.zeros(0, np.int64),) * 4


def o_draw(n, B):
    a = [np.random.randint(0, n - t, B) for t in range(4)]
    return o_map(*a)


def o_UB(X, Y, B, kernel, sigma=None):
    return o_UB_indices(X, Y, *o_draw(X.shape[0], B), kernel, sigma)


def o_UN(X, Y, N, f_block):
    perm = np.random.permutation(X.shape[0])
    X[:] = X[perm]
    Y[:] = Y[perm]
    k = int(X.shape[0] / N)
    return np.mean([f_block(X[b * k:(b + 1) * k], Y[b * k:(b + 1) * k]) for b in range(N)])


def paired(n, dx, dy, seed, kind="gauss"):
    """A dependent paired sample: Y = X A + 0.5 noise.  "ties": rows 0, n // 2 and n - 1 equal on
    both sides; "nan": one NaN coordinate in X."""
    rng = np.random.RandomState(seed)
    X = rng.normal(size=(n, dx))
    Y = X @ rng.normal(size=(dx, dy)) + 0.5 * rng.normal(size=(n, dy))
    if kind == "ties":
        X[n - 1] = X[n // 2] = X[0]
        Y[n - 1] = Y[n // 2] = Y[0]
    if kind == "nan":
        X[n // 3, dx // 2] = np.nan
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def sig(kernel, dx, dy):
    return (math.sqrt(dx), 1.5 * math.sqrt(dy)) if kernel == "gaussian" else None


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [4, 5, 7])
def test_oracle_is_the_mean_over_ordered_4_tuples(kernel, n):
    X, Y = paired(n, 3, 2, n)
    s = sig(kernel, 3, 2)
    K, L = o_KL(X, Y, kernel, s)
    terms = [K[i, j] * (L[i, j] + L[q, r] - 2.0 * L[i, q])
             for i, j, q, r in itertools.permutations(range(n), 4)]
    want = math.fsum(terms) / len(terms)
    assert len(terms) == n * (n - 1) * (n - 2) * (n - 3)
    assert abs(o_Un(X, Y, kernel, s) - want) <= 1e-13 * o_Un_scale(X, Y, kernel, s)
    # and through the indexed oracle
    i, j, q, r = (np.array(c) for c in zip(*itertools.permutations(range(n), 4)))
    got = o_UB_indices(X, Y, i, j, q, r, kernel, s)
    assert abs(got - want) <= 1e-13 * o_UB_scale(X, Y, i, j, q, r, kernel, s)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", [4, 6, 23])
def test_oracle_is_the_u_centred_inner_product(kernel, n):
    X, Y = paired(n, 4, 3, 10 + n)
    s = sig(kernel, 4, 3)

    def centred(A):
        row = A.sum(axis=1, keepdims=True) / (n - 2)
        C = A - row - row.T + A.sum() / ((n - 1) * (n - 2))
        np.fill_diagonal(C, 0.0)
        return C

    K, L = o_KL(X, Y, kernel, s)
    want = (centred(K) * centred(L)).sum() / (n * (n - 3))
    assert abs(o_Un(X, Y, kernel, s) - want) <= 1e-12 * o_Un_scale(X, Y, kernel, s)


@pytest.mark.parametrize("kernel", KERNELS)
def test_oracle_correlation(kernel):
    X, Y = paired(40, 3, 3, 5)
    s = 1.3 if kernel == "gaussian" else None
    assert abs(o_correlation(X, X.copy(), kernel, s) - 1.0) <= 1e-12
    Z = np.random.RandomState(6).normal(size=Y.shape)  # independent of X
    dep, ind = o_correlation(X, Y, kernel, s), o_correlation(X, Z, kernel, s)
    assert dep > 0.2 > abs(ind), (dep, ind)
    assert o_Un(X, Y, kernel, s) > 10.0 * abs(o_Un(X, Z, kernel, s))
    # a constant side: both of its statistics vanish, the correlation is NaN
    assert np.isnan(o_correlation(X, np.ones_like(Y), "distance"))


def test_oracle_nan_and_ties():
    X, Y = paired(9, 4, 2, 8, "nan")  # one NaN coordinate in X: the L-only outputs stay finite
    c = dict(zip(NAMES, o_components(X, Y, "distance")))
    assert all(np.isnan(c[k]) == (k not in ("S_LL", "R_L", "R_LL")) for k in NAMES), c
    k, l = o_row_sums(X, Y, "distance")  # noqa: E741
    assert np.isnan(k).all() and not np.isnan(l).any()
    X4 = np.ones((4, 3))
    assert o_components(X4, X4, "gaussian", 1.0) == (6.0, 6.0, 6.0, 12.0, 12.0, 36.0, 36.0, 36.0)
    assert o_components(X4, X4, "distance") == (0.0,) * 8


def test_the_draw_is_uniform_over_distinct_4_tuples(tw):
    import tuplewise.hsic as hs
    n = 5
    a = np.array(list(itertools.product(range(n), range(n - 1), range(n - 2), range(n - 3)))).T
    got = hs._tuples_from(*a)
    want = o_map(*a)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    tuples = list(zip(*(g.tolist() for g in got)))
    assert all(len(set(t)) == 4 and min(t) >= 0 and max(t) < n for t in tuples)
    # a bijection onto the n (n - 1)(n - 2)(n - 3) ordered 4-tuples: each exactly once
    assert sorted(tuples) == sorted(itertools.permutations(range(n), 4))
    # and from the RNG: the four calls in their order, nothing else drawn
    np.random.seed(3)
    i, j, q, r = hs._draw_tuples(11, 1000)
    state = np.random.get_state()
    np.random.seed(3)
    want = o_draw(11, 1000)
    assert all(np.array_equal(g, w) for g, w in zip((i, j, q, r), want))
    assert same_state(state, np.random.get_state())
    assert all(len({a, b, c, d}) == 4 for a, b, c, d in zip(i, j, q, r))


def test_UN_shuffles_both_arrays_by_one_permutation(tw):
    import tuplewise.hsic as hs
    n, N = 23, 4
    X, Y = paired(n, 3, 2, 1)
    X[:, 0] = Y[:, 0] = np.arange(n)  # the pairing shows in the first column
    Xo, Yo = X.copy(), Y.copy()
    seen = []

    def block(x, y):
        assert np.array_equal(x[:, 0], y[:, 0])
        seen.append(x.shape[0])
        return float(x[0, 0] + y[-1, 1])

    np.random.seed(9)
    got = hs.UN(X, Y, N, block)
    state = np.random.get_state()
    np.random.seed(9)
    want = o_UN(Xo, Yo, N, lambda x, y: float(x[0, 0] + y[-1, 1]))
    assert got == want and seen == [5] * N
    assert np.array_equal(X, Xo) and np.array_equal(Y, Yo)
    assert same_state(state, np.random.get_state())
    np.random.seed(9)
    assert np.array_equal(X[:, 0], np.random.permutation(n).astype(np.float64))


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.hsic as hs
    for name in ("components", "row_sums", "Un", "correlation", "UB_indices", "UB", "UN", "UnN",
                 "UnNB", "UnNT", "UnNBT"):
        assert callable(getattr(hs, name)), name
    assert hs.MAX_D == 64 and hs.Components._fields == NAMES
    assert not hasattr(hs, "pvalue") and not hasattr(hs, "permutation_test")


def test_argument_errors_need_no_device(tw):
    import tuplewise.hsic as hs
    X, Y = np.arange(48.0).reshape(12, 4), np.arange(36.0).reshape(12, 3) + 0.5
    X0, Y0 = X.copy(), Y.copy()
    x1 = np.arange(12.0)
    wide = np.zeros((6, 65))
    D = dict(kernel="distance")
    G = dict(sigma=1.0)
    state = np.random.get_state()
    calls = [
        # dtype, layout, rank
        lambda: hs.Un(X.astype(np.float32), Y, **D), lambda: hs.Un(X, Y.astype(np.int64), **G),
        lambda: hs.Un(X[:, ::2], Y, **D), lambda: hs.components(X.T[:3].T, Y, **G),
        lambda: hs.Un(X.reshape(6, 2, 4), Y[:6], **D), lambda: hs.UB(X, Y.reshape(6, 2, 3), 5, **G),
        lambda: hs.row_sums(x1[::2], x1[:6], **D),
        # d above 64, none
        lambda: hs.Un(wide, Y[:6], **G), lambda: hs.UB(X[:6], wide, 3, **D),
        lambda: hs.Un(np.zeros((6, 0)), Y[:6], **D), lambda: hs.correlation(X, np.zeros((12, 0)), **G),
        # rows of X != rows of Y; n < 4
        lambda: hs.Un(X, Y[:11], **D), lambda: hs.components(X[:5], Y, **G),
        lambda: hs.row_sums(X, x1[:4], **D), lambda: hs.UB(X[:7], Y, 4, **D),
        lambda: hs.Un(X[:3], Y[:3], **D), lambda: hs.correlation(X[:0], Y[:0], **G),
        lambda: hs.UB(X[:3], Y[:3], 4, **D), lambda: hs.UB_indices(X[:3], Y[:3], [0], [1], [2], [2], **G),
        lambda: hs.UnN(X[:3], Y[:3], 1, **D),
        # the kernel and its sigma
        lambda: hs.Un(X, Y, kernel="laplace", sigma=1.0), lambda: hs.UB(X, Y, 3, kernel=None),
        lambda: hs.Un(X, Y, kernel="energy"),
        lambda: hs.Un(X, Y), lambda: hs.Un(X, Y, kernel="gaussian"), lambda: hs.UB(X, Y, 3),
        lambda: hs.Un(X, Y, sigma=0.0), lambda: hs.Un(X, Y, sigma=-1.0),
        lambda: hs.components(X, Y, sigma=float("nan")), lambda: hs.UB(X, Y, 3, sigma=float("inf")),
        lambda: hs.Un(X, Y, sigma="wide"), lambda: hs.Un(X, Y, sigma=1e-200),
        lambda: hs.Un(X, Y, sigma=(1.0,)), lambda: hs.Un(X, Y, sigma=(1.0, 2.0, 3.0)),
        lambda: hs.Un(X, Y, sigma=(1.0, 0.0)), lambda: hs.row_sums(X, Y, sigma=(float("nan"), 1.0)),
        lambda: hs.correlation(X, Y, sigma=(1.0, None)), lambda: hs.Un(X, Y, sigma=[[1.0, 2.0]]),
        lambda: hs.Un(X, Y, kernel="distance", sigma=1.0),
        lambda: hs.UB(X, Y, 3, kernel="distance", sigma=(1.0, 2.0)),
        lambda: hs.UnN(X, Y, 2), lambda: hs.UnNB(X, Y, 2, 3, sigma=0.0),
        lambda: hs.UnNT(X, Y, 2, 2, kernel="distance", sigma=1.0),
        lambda: hs.UnNBT(X, Y, 2, 3, 2, kernel="x"),
        # index arrays of different shapes; indices that are not all distinct (also through a
        # negative index)
        lambda: hs.UB_indices(X, Y, [0, 1], [1], [2, 2], [3, 3], **D),
        lambda: hs.UB_indices(X, Y, [0, 1], [1, 0], [2, 3], [3], **G),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 3], [2, 1], [4, 0], **D),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 2], [0, 1], [4, 0], **G),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 2], [2, 1], [0, 0], **D),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 2], [2, 2], [4, 0], **G),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 2], [2, 1], [1, 0], **D),
        lambda: hs.UB_indices(X, Y, [0, 3], [1, 2], [2, 1], [4, 1], **G),
        lambda: hs.UB_indices(X, Y, [0, -1], [1, 11], [2, 1], [3, 0], **D),
        lambda: hs.UB_indices(X, Y, [0], [1], [5], [-7], **D),
        # partitions out of scope
        lambda: hs.UnN(X, Y, 2, "SWOR", **D), lambda: hs.UnNB(X, Y, 2, 3, "prop-SWR", **G),
        lambda: hs.UnNT(X, Y, 2, 2, "SWR", **D), lambda: hs.UnNBT(X, Y, 2, 3, 2, "SWOR", **G),
        lambda: hs.UN(X, Y, 2, lambda x, y: 0.0, "SWOR"),
        # a block of fewer than 4 rows
        lambda: hs.UnN(X, Y, 4, **D), lambda: hs.UnN(X, Y, 13, **G), lambda: hs.UnNT(X, Y, 5, 2, **D),
        lambda: hs.UnNB(X, Y, 4, 3, **D), lambda: hs.UnNBT(X, Y, 7, 3, 2, **G),
        lambda: hs.UN(X, Y, 4, lambda x, y: 0.0), lambda: hs.UN(X, Y, 0, lambda x, y: 0.0),
        # UN shuffles in place: lists are refused
        lambda: hs.UN(X.tolist(), Y, 2, lambda x, y: 0.0), lambda: hs.UN(X, Y.tolist(), 2, lambda x, y: 0.0),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    with pytest.raises(ValueError, match="prop-SWOR"):
        hs.UnN(X, Y, 2, "SWOR", **D)
    with pytest.raises(ValueError, match="needs sigma"):
        hs.Un(X, Y)
    with pytest.raises(ValueError, match="four distinct rows"):
        hs.UB_indices(X, Y, [2], [3], [4], [2], **D)
    with pytest.raises(ValueError, match="paired"):
        hs.Un(X, Y[:8], **D)
    with pytest.raises(ValueError, match="at least 4 rows"):
        hs.UnN(X, Y, 4, **D)
    # a shape whose row-sum partials would pass the device work budget, alone and as one block
    big = np.zeros(300_000)
    for call in (lambda: hs.Un(big, big.copy(), **D), lambda: hs.UnN(big, big.copy(), 1, **D)):
        with pytest.raises(ValueError, match="work budget"):
            call()
        assert same_state(np.random.get_state(), state)
    # rows out of range are NumPy's IndexError, as in the sibling modules
    for call in (lambda: hs.UB_indices(X, Y, [12], [0], [1], [2], **D),
                 lambda: hs.UB_indices(X, Y, [0], [-13], [1], [2], **D),
                 lambda: hs.UB_indices(X, Y, [0], [1], [12], [2], **G),
                 lambda: hs.UB_indices(X, Y, [0], [1], [2], [-13], **G),
                 lambda: hs.UB_indices(X, Y, [0.0], [1], [2], [3], **D)):
        with pytest.raises(IndexError):
            call()
    # nothing was shuffled and nothing was drawn on the way to those errors
    assert np.array_equal(X, X0) and np.array_equal(Y, Y0)
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.hsic as hs
    X, Y = paired(6, 3, 2, 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.Un(X, Y, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.components(X, Y, kernel="distance")
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.row_sums(X, Y, sigma=(1.0, 2.0))
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.correlation(X, Y, kernel="distance")
    with pytest.raises(RuntimeError, match="no HIP device"):
        hs.UB_indices(X, Y, [0, 1], [2, 3], [4, 5], [1, 0], kernel="distance")


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    nan, inf = float("nan"), float("inf")

    def sums(dx=3, dy=2, n_blocks=1, max_n=4, kern=L.TW_HSIC_GAUSSIAN, cx=-0.5, cy=-0.25, group=0,
             ptr=p, out=p, rows=None):
        return lib.tw_hsic_sums(p, dx, ptr, dy, p, n_blocks, max_n, kern, cx, cy, group, p, rows,
                                out, None)

    def idx(dx=3, dy=2, n_shards=1, max_q=4, kern=L.TW_HSIC_DISTANCE, cx=0.0, cy=0.0, ptr=p):
        return lib.tw_hsic_idx32(p, dx, p, dy, p, p, p, ptr, p, n_shards, max_q, kern, cx, cy, p,
                                 p, None)

    for name, fn in ((b"tw_hsic_sums", sums), (b"tw_hsic_idx32", idx)):
        G = dict(kern=L.TW_HSIC_GAUSSIAN)
        for call, word in ((lambda: fn(ptr=None), b"null pointer"),
                           (lambda: fn(dx=0), b"dx 0 outside [1, 64]"),
                           (lambda: fn(dx=65), b"dx 65 outside [1, 64]"),
                           (lambda: fn(dy=0), b"dy 0 outside [1, 64]"),
                           (lambda: fn(dy=65), b"dy 65 outside [1, 64]"),
                           (lambda: fn(kern=2), b"unknown kernel"),
                           (lambda: fn(kern=-1), b"unknown kernel"),
                           (lambda: fn(cx=0.5, cy=-1.0, **G), b"Gaussian"),
                           (lambda: fn(cx=-1.0, cy=0.5, **G), b"Gaussian"),
                           (lambda: fn(cx=nan, cy=-1.0, **G), b"Gaussian"),
                           (lambda: fn(cx=-1.0, cy=nan, **G), b"Gaussian"),
                           (lambda: fn(cx=-inf, cy=-1.0, **G), b"Gaussian"),
                           (lambda: fn(cx=-1.0, cy=inf, **G), b"Gaussian")):
            assert call() == L.TW_ERR_ARG, (name, word)
            msg = lib.tw_last_error()
            assert word in msg and name in msg, msg
    for call in (lambda: sums(out=None), lambda: sums(n_blocks=-1), lambda: sums(max_n=-1),
                 lambda: idx(n_shards=-1), lambda: idx(max_q=-1)):
        assert call() == L.TW_ERR_ARG
        msg = lib.tw_last_error()
        assert b"negative size" in msg or b"null pointer" in msg, msg
    # a block of fewer than 4 rows; the plan knob; the work budget; the grid
    for call, word in ((lambda: sums(max_n=3), b"at least 4 rows"),
                       (lambda: sums(max_n=0), b"at least 4 rows"),
                       (lambda: sums(group=-1), b"group -1 outside"),
                       (lambda: sums(group=9), b"group 9 outside"),
                       (lambda: sums(max_n=10 ** 7, group=1), b"d_work past"),
                       (lambda: sums(max_n=10 ** 7), b"d_work past"),
                       (lambda: sums(n_blocks=2 ** 31 - 1, max_n=4), b"grid too large"),
                       (lambda: idx(n_shards=2 ** 31 - 1, max_q=2000), b"grid too large")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg, msg
    # nothing to do: no blocks, no shards (the distance kernel ignores c; d_rows may be NULL)
    assert sums(n_blocks=0) == L.TW_OK and idx(n_shards=0, cx=nan, cy=inf) == L.TW_OK
    with pytest.raises(ValueError, match="unknown kernel"):
        L.call("tw_hsic_sums", p, 3, p, 2, p, 1, 4, 7, -0.5, -0.5, 0, p, None, p, None)
    P = lib.tw_hsic_tile()
    assert P == lib.tw_mmd_tile()
    wb = lib.tw_hsic_work_bytes
    small, big = wb(1, 4, 0), wb(64, 1562, 0)
    assert 8 * (3 + 5 + 2) <= small <= big < 1 << 28
    # refused sizes are a work size of 0
    assert wb(0, 4, 0) == 0 and wb(-1, 4, 0) == 0 and wb(1, 3, 0) == 0 and wb(1, -1, 0) == 0
    assert wb(1, 4, -1) == 0 and wb(1, 4, 9) == 0 and wb(1, 10 ** 7, 0) == 0
    assert wb(2 ** 31 - 1, 4, 0) == 0
    # a larger group leaves fewer row-sum partials; the automatic choice is one of the explicit
    # plans, and n = 1e5 in one block fits the budget only through it
    assert wb(1, 4 * P + 5, 1) > wb(1, 4 * P + 5, 2) > wb(1, 4 * P + 5, 8) > 0
    assert wb(1, 4 * P + 5, 0) in [wb(1, 4 * P + 5, g) for g in range(1, 9)]
    assert wb(1, 10 ** 5, 1) == 0 and 0 < wb(1, 10 ** 5, 0) <= 1 << 30
    iw = lib.tw_hsic_idx_work_bytes
    small, big = iw(1, 1), iw(64, 10 ** 6)
    assert 24 <= small <= big < 1 << 26 and iw(-1, 1) == 0 and iw(1, -1) == 0
    assert iw(2 ** 31 - 1, 2000) == 0 and big % 24 == 0
