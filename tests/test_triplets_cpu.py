"""tuplewise.triplets without a GPU: the NumPy oracle the GPU tests compare against (distances in
the contract's arithmetic order, per-anchor counts by sort and search, the estimators restated
literally with the same np.random calls in the same order), the oracle against a brute-force
triple loop, every argument error before any device work or RNG draw, and the batching
arithmetic."""
import ctypes

import numpy as np
import pytest

MODES = ["gt", "half"]


# ------------------------------------------------------------------------------------ oracle
def o_rows(A):
    A = np.asarray(A)
    return A.reshape(-1, 1) if A.ndim == 1 else A


def o_dist_rows(A, B):
    """D(a, b) for every row a of A against every row b of B, (len(A), len(B)): acc = 0.0; for c:
    t = a_c - b_c; acc = acc + t * t — NumPy's elementwise multiply and add never fuse.  A NaN
    distance is np.nan itself (which NaN an operation returns is the hardware's choice)."""
    A, B = o_rows(A), o_rows(B)
    acc = np.zeros((A.shape[0], B.shape[0]))
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(A.shape[1]):
            t = A[:, None, c] - B[None, :, c]
            acc = acc + t * t
    acc[np.isnan(acc)] = np.nan
    return acc


def o_dist_pairs(A, B):
    """D(A[p], B[p]) row by row, in the same order."""
    A, B = o_rows(A), o_rows(B)
    acc = np.zeros(A.shape[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(A.shape[1]):
            t = A[:, c] - B[:, c]
            acc = acc + t * t
    return acc


def o_own_rows(X):
    """The "own" rows: D(x_i, x_j) for j != i, (n, n - 1), j > i one to the left."""
    D = o_dist_rows(X, X)
    n = D.shape[0]
    return D[~np.eye(n, dtype=bool)].reshape(n, n - 1)


def o_triplet_counts(X, Z):
    """(gt, eq) per anchor: the own row sorted without its NaN, searched with the other row's
    non-NaN entries (a NaN distance compares false both ways)."""
    other, own = o_dist_rows(X, Z), o_own_rows(X)
    gt = np.zeros(other.shape[0], dtype=np.uint64)
    eq = np.zeros(other.shape[0], dtype=np.uint64)
    for i in range(other.shape[0]):
        s = np.sort(own[i][~np.isnan(own[i])])
        q = other[i][~np.isnan(other[i])]
        left = np.searchsorted(s, q, side="left")
        gt[i] = left.sum()
        eq[i] = (np.searchsorted(s, q, side="right") - left).sum()
    return gt, eq


def o_counts(X, Z, mode):
    gt, eq = o_triplet_counts(X, Z)
    return gt if mode == "gt" else 2 * gt + eq


def o_value(count, terms, mode):
    return np.float64(int(count) / int(terms * (2 if mode == "half" else 1)))


def o_Un(X, Z, mode="gt"):
    n, m = o_rows(X).shape[0], o_rows(Z).shape[0]
    C = sum(int(c) for c in o_counts(X, Z, mode))
    return o_value(C, n * (n - 1) * m, mode)


def o_UB_indices(X, Z, i, j, k, mode):
    X, Z = o_rows(X), o_rows(Z)
    other, own = o_dist_pairs(X[i], Z[k]), o_dist_pairs(X[i], X[j])
    with np.errstate(invalid="ignore"):
        gt, eq = int(np.sum(other > own)), int(np.sum(other == own))
    if len(i) == 0:
        return np.float64("nan")
    return o_value(gt if mode == "gt" else 2 * gt + eq, len(i), mode)


def o_UB(X, Z, B, mode):
    n, m = X.shape[0], Z.shape[0]
    i = np.random.randint(0, n, B)
    j = np.random.randint(0, n - 1, B)
    j += (j >= i)
    k = np.random.randint(0, m, B)
    return o_UB_indices(X, Z, i, j, k, mode)


def o_UN(X, Z, N, f_block):
    np.random.shuffle(X)
    np.random.shuffle(Z)
    k, kz = int(X.shape[0] / N), int(Z.shape[0] / N)
    return np.mean([f_block(X[b * k:(b + 1) * k], Z[b * kz:(b + 1) * kz]) for b in range(N)])


def o_UnN(X, Z, N, mode):
    return o_UN(X, Z, N, lambda x, z: o_Un(x, z, mode))


def o_UnNB(X, Z, N, B, mode):
    return o_UN(X, Z, N, lambda x, z: o_UB(x, z, B, mode))


def o_UnNT(X, Z, N, T, mode):
    return np.mean([o_UnN(X, Z, N, mode) for _ in range(T)])


def o_UnNBT(X, Z, N, B, T, mode):
    return np.mean([o_UnNB(X, Z, N, B, mode) for _ in range(T)])


def data(kind, n, m, d, seed):
    """"ties": integer features in {0..3}; "gauss": Gaussian; "nan": Gaussian with one NaN
    coordinate in X and one row of Z copied from X."""
    rng = np.random.RandomState(seed)
    if kind == "ties":
        return (rng.randint(0, 4, size=(n, d)).astype(np.float64),
                rng.randint(0, 4, size=(m, d)).astype(np.float64))
    X, Z = rng.normal(size=(n, d)), rng.normal(0.3, 1.0, size=(m, d))
    if kind == "nan":
        X[n // 3, d // 2] = np.nan
        Z[m // 2] = X[n - 1]
    return X, Z


# ------------------------------------------------------------------- the oracle's own checks
def brute(X, Z):
    """(gt, eq) per anchor by the definition: Python floats, a triple loop."""
    n, m, d = X.shape[0], Z.shape[0], X.shape[1]

    def dist(a, b):
        acc = 0.0
        for c in range(d):
            t = float(a[c]) - float(b[c])
            acc = acc + t * t
        return acc

    other = [[dist(X[i], Z[k]) for k in range(m)] for i in range(n)]
    own = [[dist(X[i], X[j]) for j in range(n)] for i in range(n)]
    gt, eq = [0] * n, [0] * n
    for i in range(n):
        for j in range(n):
            if j == i:
                continue
            for k in range(m):
                gt[i] += other[i][k] > own[i][j]
                eq[i] += other[i][k] == own[i][j]
    return gt, eq


@pytest.mark.parametrize("kind,d", [("ties", 2), ("gauss", 17), ("nan", 17)])
def test_oracle_is_the_triple_loop(kind, d):
    n, m = 40, 23
    X, Z = data(kind, n, m, d, 1)
    gt, eq = o_triplet_counts(X, Z)
    bgt, beq = brute(X, Z)
    assert [int(v) for v in gt] == bgt and [int(v) for v in eq] == beq
    if kind == "ties":
        assert sum(beq) > 0  # ties are really exercised
    if kind == "nan":  # the NaN anchor counts nothing; the copied row ties at distance 0
        assert bgt[n // 3] == 0 and beq[n // 3] == 0 and sum(bgt) > 0
    for mode in MODES:
        C = sum(bgt) if mode == "gt" else 2 * sum(bgt) + sum(beq)
        assert o_Un(X, Z, mode) == np.float64(C / ((1 + (mode == "half")) * n * (n - 1) * m))
    # the drawn form agrees with the definition on every triplet
    i, j, k = (a.reshape(-1) for a in np.meshgrid(np.arange(n), np.arange(n), np.arange(m),
                                                   indexing="ij"))
    keep = i != j
    assert o_UB_indices(X, Z, i[keep], j[keep], k[keep], "half") == o_Un(X, Z, "half")


def test_oracle_rows_layout():
    X, Z = data("gauss", 9, 4, 3, 2)
    own = o_own_rows(X)
    full = o_dist_rows(X, X)
    assert own.shape == (9, 8) and o_dist_rows(X, Z).shape == (9, 4)
    for i in range(9):
        assert np.array_equal(own[i, :i], full[i, :i])
        assert np.array_equal(own[i, i:], full[i, i + 1:])


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.triplets as tr
    for name in ("triplet_counts", "Un", "UB_indices", "UB", "UN", "UnN", "UnNB", "UnNT", "UnNBT"):
        assert callable(getattr(tr, name)), name
    assert tr.ROWS_BYTES == 1 << 30


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_argument_errors_need_no_device(tw):
    import tuplewise.triplets as tr
    X, Z = np.arange(40.0).reshape(10, 4), np.arange(24.0).reshape(6, 4) + 0.5
    X0, Z0 = X.copy(), Z.copy()
    x1 = np.arange(10.0)
    wide = np.zeros((4, 65))
    state = np.random.get_state()
    calls = [
        # dtype, layout, rank
        lambda: tr.Un(X.astype(np.float32), Z), lambda: tr.Un(X, Z.astype(np.int64)),
        lambda: tr.Un(X[:, ::2], Z[:, ::2]), lambda: tr.triplet_counts(X.T, Z.T),
        lambda: tr.Un(X.reshape(5, 2, 4), Z), lambda: tr.UB(X, Z.reshape(3, 2, 4), 5),
        lambda: tr.Un(x1[::2], x1),
        # d: a mismatch, above 64, none
        lambda: tr.Un(X, x1), lambda: tr.Un(wide, wide), lambda: tr.UB(wide, wide, 3),
        lambda: tr.Un(np.zeros((4, 0)), np.zeros((3, 0))),
        # too few rows
        lambda: tr.Un(X[:1], Z), lambda: tr.Un(X, Z[:0]), lambda: tr.triplet_counts(X[:0], Z),
        lambda: tr.UB(X[:1], Z, 4), lambda: tr.UB_indices(X, Z[:0], [0], [1], [0]),
        # mode, algo
        lambda: tr.Un(X, Z, mode="ne"), lambda: tr.UB(X, Z, 3, mode="x"),
        lambda: tr.Un(X, Z, algo="fast"), lambda: tr.triplet_counts(X, Z, "half", "x"),
        lambda: tr.UnN(X, Z, 2, mode="subgt"), lambda: tr.UnNT(X, Z, 2, 2, algo="x"),
        lambda: tr.UnNB(X, Z, 2, 3, mode="x"), lambda: tr.UnNBT(X, Z, 2, 3, 2, mode="x"),
        # index arrays of different shapes
        lambda: tr.UB_indices(X, Z, [0, 1], [1], [0, 0]),
        # partitions out of scope
        lambda: tr.UnN(X, Z, 2, "SWOR"), lambda: tr.UnNB(X, Z, 2, 3, "prop-SWR"),
        lambda: tr.UnNT(X, Z, 2, 2, "SWR"), lambda: tr.UnNBT(X, Z, 2, 3, 2, "SWOR"),
        lambda: tr.UN(X, Z, 2, tr.Un, "SWOR"),
        # a block of fewer than 2 rows of X or none of Z
        lambda: tr.UnN(X, Z, 6), lambda: tr.UnN(X, Z[:4], 5), lambda: tr.UnNT(X, Z, 7, 2),
        lambda: tr.UnNB(X, Z, 6, 3), lambda: tr.UnNBT(X, Z, 7, 3, 2),
        lambda: tr.UN(X, Z, 7, lambda x, z: 0.0),
        # UN shuffles in place: lists are refused
        lambda: tr.UN(X.tolist(), Z, 2, tr.Un),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    with pytest.raises(ValueError, match="prop-SWOR"):
        tr.UnN(X, Z, 2, "SWOR")
    for call in (lambda: tr.UB_indices(X, Z, [10], [0], [0]),
                 lambda: tr.UB_indices(X, Z, [0], [-11], [0]),
                 lambda: tr.UB_indices(X, Z, [0], [1], [6]),
                 lambda: tr.UB_indices(X, Z, [0.0], [1], [0])):
        with pytest.raises(IndexError):
            call()
    # nothing was shuffled and nothing was drawn on the way to those errors
    assert np.array_equal(X, X0) and np.array_equal(Z, Z0)
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.triplets as tr
    X, Z = data("gauss", 6, 4, 3, 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tr.Un(X, Z)
    with pytest.raises(RuntimeError, match="no HIP device"):
        tr.UB_indices(X, Z, [0, 1], [2, 3], [0, 1])


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def rows(d=3, a_begin=0, a_end=2, max_n=2, max_m=1, ptr=p, blk_count=1):
        return lib.tw_triplet_rows(ptr, p, d, p, p, 0, blk_count, a_begin, a_end, max_n, max_m,
                                   p, p, p, p, None)

    def idx(d=3, n_shards=1, max_t=4, pred=L.TW_PRED_GT, ptr=p):
        return lib.tw_triplet_idx32(p, ptr, d, p, p, p, p, n_shards, max_t, pred, p, p, None)

    for call, word in ((lambda: rows(ptr=None), b"null pointer"),
                       (lambda: rows(d=0), b"outside [1, 64]"),
                       (lambda: rows(d=65), b"outside [1, 64]"),
                       (lambda: rows(max_n=-1), b"negative size"),
                       (lambda: rows(max_m=-2), b"negative size"),
                       (lambda: rows(a_begin=-1), b"negative size"),
                       (lambda: rows(blk_count=0), b"negative size"),
                       (lambda: rows(a_begin=2, a_end=2), b"empty anchor range"),
                       (lambda: rows(a_begin=3, a_end=1), b"empty anchor range")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_triplet_rows" in msg, msg
    for call, word in ((lambda: idx(ptr=None), b"null pointer"),
                       (lambda: idx(d=0), b"outside [1, 64]"),
                       (lambda: idx(d=65), b"outside [1, 64]"),
                       (lambda: idx(n_shards=-1), b"n_shards"),
                       (lambda: idx(max_t=-1), b"max_triplets"),
                       (lambda: idx(pred=L.TW_PRED_SUBGT), b"predicate")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_triplet_idx32" in msg, msg
    assert idx(n_shards=0) == L.TW_OK  # no shards: nothing to do
    P = lib.tw_triplet_rows_tile()
    assert 64 <= P <= 4096 and P % 64 == 0
    small, big = lib.tw_triplet_idx_work_bytes(1, 1), lib.tw_triplet_idx_work_bytes(64, 10 ** 6)
    assert 8 <= small <= big < 1 << 26 and lib.tw_triplet_idx_work_bytes(-1, 1) == 0


@pytest.mark.parametrize("cap", [1, 8, 100, 8 * 37, 8 * 38, 1000, 1 << 30])
def test_batches_cover_every_anchor_once(tw, cap):
    import tuplewise.triplets as tr
    rng = np.random.RandomState(cap % 97)
    for elems in ([37] * 11, [5, 0, 0, 9], [1000], list(rng.randint(1, 60, size=50)),
                  np.repeat([3, 70, 6, 65], [2, 67, 5, 64])):
        edges = tr.batch_edges(elems, cap)
        assert edges[0][0] == 0 and edges[-1][1] == len(elems)
        for (a0, a1), nxt in zip(edges, edges[1:] + [None]):
            assert a1 > a0  # at least one anchor
            size = 8 * int(np.sum(elems[a0:a1]))
            assert size <= cap or a1 == a0 + 1
            if nxt is not None:
                assert nxt[0] == a1  # no gap, no overlap
                assert size + 8 * int(elems[a1]) > cap  # and no batch stops early
