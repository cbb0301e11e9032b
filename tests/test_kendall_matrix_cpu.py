"""tuplewise.kendall without a GPU: the brute-force oracle the GPU tests compare against (signs
over np.triu_indices, then s^T s) checked against the (n, 2) oracle of test_onesample_cpu, every
argument error before any device work or RNG draw, the native entries' argument checks, and the
host half (tau expressions, shuffles, block means) with the device glue stubbed to the oracle."""
import ctypes

import numpy as np
import pytest

from test_onesample_cpu import o_kendall_counts, o_kendall_tau_b, o_UnN, o_UnNT


# ------------------------------------------------------------------------------------ oracle
def o_signs(S):
    """(pairs, p) int8 signs of S[i] - S[j] over i < j (int64 compared as int64)."""
    S = np.asarray(S)
    i, j = np.triu_indices(S.shape[0], 1)
    return ((S[i] > S[j]).astype(np.int8) - (S[i] < S[j]).astype(np.int8))


def o_sign_counts(S, Y=None):
    """(M, Us, Uy, pairs) as int64 arrays and a Python int."""
    # float64 products of -1, 0, 1 summed over fewer than 2^53 pairs are exact (and use BLAS)
    sa = o_signs(S).astype(np.float64)
    sb = sa if Y is None else o_signs(Y).astype(np.float64)
    n = np.asarray(S).shape[0]
    M, Us, Uy = sa.T @ sb, (sa * sa).sum(axis=0), (sb * sb).sum(axis=0)
    return M.astype(np.int64), Us.astype(np.int64), Uy.astype(np.int64), n * (n - 1) // 2


def o_tau_a(S, Y=None):
    M, _, _, P = o_sign_counts(S, Y)
    out = np.empty(M.shape, np.float64)
    for idx in np.ndindex(*M.shape):
        out[idx] = np.float64(int(M[idx]) / P)
    return out


def o_mean_blocks(vals):
    """Per entry, np.mean of the 1-D list of the blocks' values."""
    vals = [np.asarray(v) for v in vals]
    out = np.empty(vals[0].shape, np.float64)
    for idx in np.ndindex(*out.shape):
        out[idx] = np.mean([v[idx] for v in vals])
    return out


def o_UnN_matrix(S, N):
    np.random.shuffle(S)
    k = int(S.shape[0] / N)
    return o_mean_blocks([o_tau_a(S[b * k:(b + 1) * k]) for b in range(N)])


def o_UnNT_matrix(S, N, T):
    return o_mean_blocks([o_UnN_matrix(S, N) for _ in range(T)])


def table(n, p, seed, ties=False, dtype=np.float64):
    rng = np.random.RandomState(seed)
    if ties:
        return rng.randint(0, 6, size=(n, p)).astype(dtype)
    if dtype == np.int64:
        return rng.randint(-2 ** 62, 2 ** 62, size=(n, p)).astype(np.int64)
    base = rng.normal(size=(n, 1))
    return np.ascontiguousarray(0.5 * base + rng.normal(size=(n, p)))


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def stub_launch(X, Y, off):
    """kendall._launch by the oracle: one (M, Ua, Ub) per shard of `off`."""
    Ms, Ua, Ub = [], [], []
    for s in range(len(off) - 1):
        lo, hi = int(off[s]), int(off[s + 1])
        M, us, uy, _ = o_sign_counts(X[lo:hi], None if Y is None else Y[lo:hi])
        Ms.append(M)
        Ua.append(us)
        Ub.append(uy)
    return np.stack(Ms), np.stack(Ua), np.stack(Ub)


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n,p", [(2, 3), (17, 5), (389, 64)])
def test_oracle_entries_are_the_pair_oracles(n, p, ties):
    S = table(n, p, 7 * n + p + ties, ties)
    M, Us, Uy, P = o_sign_counts(S)
    assert P == n * (n - 1) // 2 and np.array_equal(M, M.T) and np.array_equal(Us, Uy)
    assert np.array_equal(np.diag(M), Us)
    for a in range(p):
        _, cnt = np.unique(S[:, a], return_counts=True)
        assert int(Us[a]) == P - int(np.sum(cnt * (cnt - 1) // 2))
    cols = [(a, b) for a in range(p) for b in range(a + 1, p)]
    if p == 64:  # every column once, and a spread of pairs
        cols = [(a, (a * 7 + 1) % p) for a in range(p) if a != (a * 7 + 1) % p]
    for a, b in cols:
        c, d, tx, ty, _ = o_kendall_counts(np.ascontiguousarray(S[:, [a, b]]))
        assert int(M[a, b]) == c - d and int(Us[a]) == P - tx and int(Us[b]) == P - ty


def test_oracle_cross_is_not_symmetric():
    S, Y = table(40, 3, 1), table(40, 5, 2)
    M, Us, Uy, _ = o_sign_counts(S, Y)
    assert M.shape == (3, 5) and Us.shape == (3,) and Uy.shape == (5,)
    for a in range(3):
        for b in range(5):
            c, d, _, _, _ = o_kendall_counts(np.ascontiguousarray(np.stack([S[:, a], Y[:, b]], 1)))
            assert int(M[a, b]) == c - d


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.kendall as K
    for name in ("sign_counts", "tau_matrix", "Un", "UnN", "UnNT"):
        assert callable(getattr(K, name)), name
    assert K.SignCounts._fields == ("M", "Us", "Uy", "pairs")


def _fail(*a, **k):
    raise AssertionError("device work before an argument error")


def test_argument_errors_need_no_device(tw, monkeypatch):
    import tuplewise.kendall as K
    L = tw._lib
    for name in ("call", "device", "to_device", "to_device_many", "empty", "stream_handle"):
        monkeypatch.setattr(L, name, _fail)
    S = np.arange(40.0).reshape(10, 4)
    nan = S.copy()
    nan[3, 1] = np.nan
    state = np.random.get_state()
    bad = [
        lambda: K.sign_counts(np.arange(10.0)),                        # shape
        lambda: K.sign_counts(np.zeros((4, 2, 2))),
        lambda: K.tau_matrix(np.zeros((4, 3), np.float32)),            # dtype
        lambda: K.sign_counts(np.zeros((4, 3), np.int32)),
        lambda: K.sign_counts(np.zeros((3, 8)).T),                     # contiguity
        lambda: K.Un(S[:, ::2]),
        lambda: K.sign_counts(S[:1]),                                  # n < 2
        lambda: K.tau_matrix(S[:0]),
        lambda: K.sign_counts(np.zeros((4, 0))),                       # p out of range
        lambda: K.sign_counts(np.zeros((2, 1025))),
        lambda: K.sign_counts(S, np.zeros((9, 2))),                    # Y mismatch
        lambda: K.sign_counts(S, np.zeros((10, 2), np.float32)),
        lambda: K.tau_matrix(S, np.arange(10.0)),
        lambda: K.sign_counts(nan),                                    # NaN
        lambda: K.tau_matrix(S, nan),
        lambda: K.Un(nan),
        lambda: K.UnN(nan, 2),
        lambda: K.UnNT(nan, 2, 2),
        lambda: K.tau_matrix(S, variant="c"),                          # variant
        lambda: K.tau_matrix(S, S, variant=None),
        lambda: K.UnN(S, 6),                                           # blocks of < 2 rows
        lambda: K.UnNT(S, 10, 2),
        lambda: K.UnN(S, 0),
        lambda: K.UnNT(S, 2, 0),
    ]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError, match="ranks are undefined.*onesample"):
        K.sign_counts(nan)
    assert np.array_equal(S.reshape(-1), np.arange(40.0))
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.kendall as K
    with pytest.raises(RuntimeError, match="no HIP device"):
        K.sign_counts(np.arange(10.0).reshape(5, 2))
    with pytest.raises(RuntimeError, match="no HIP device"):
        K.UnN(np.arange(20.0).reshape(10, 2), 2)


# ------------------------------------------------------------------------- native entries
def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()

    def ranks(n_shards=1, total=4, max_n=4, p=2, dtype=L.TW_F64, width=16):
        return lib.tw_col_ranks(None, None, n_shards, total, max_n, p, dtype, width, None, None,
                                None)

    def matrix(pa=2, pb=2, n_shards=1, max_n=4, width=16):
        return lib.tw_kendall_matrix(None, pa, None, pb, None, n_shards, max_n, width, None, None,
                                     None, None, None)

    for call, word in ((lambda: ranks(n_shards=-1), b"n_shards"),
                       (lambda: ranks(total=3), b"bad sizes"),
                       (lambda: ranks(max_n=-1), b"bad sizes"),
                       (lambda: ranks(p=0), b"columns"), (lambda: ranks(p=1025), b"columns"),
                       (lambda: ranks(dtype=2), b"dtype"), (lambda: ranks(width=8), b"width"),
                       (lambda: ranks(width=0), b"width"),
                       (lambda: ranks(total=65537, max_n=65537), b"16-bit"),
                       (lambda: ranks(), b"null")):
        assert call() == L.TW_ERR_ARG
        msg = lib.tw_last_error()
        assert word in msg and b"tw_col_ranks" in msg, msg
    assert ranks(n_shards=0, total=0, max_n=0) == L.TW_OK
    for call, word in ((lambda: matrix(n_shards=-1), b"n_shards"),
                       (lambda: matrix(max_n=-1), b"max_n"),
                       (lambda: matrix(pa=0), b"columns"), (lambda: matrix(pb=1025), b"columns"),
                       (lambda: matrix(width=24), b"width"),
                       (lambda: matrix(max_n=65537), b"16-bit"),
                       (lambda: matrix(), b"null")):
        assert call() == L.TW_ERR_ARG
        msg = lib.tw_last_error()
        assert word in msg and b"tw_kendall_matrix" in msg, msg
    assert matrix(n_shards=0) == L.TW_OK


def test_tile_width_and_work_sizes(tw):
    lib = tw._lib.lib()
    T = lib.tw_kendall_matrix_tile()
    assert T % 16 == 0 and 16 <= T <= 1024
    assert lib.tw_kendall_matrix_width(2) == 16 and lib.tw_kendall_matrix_width(65536) == 16
    assert lib.tw_kendall_matrix_width(65537) == 32
    for n in (1, 1024, 1025, 2049, 10 ** 6):
        C = lib.tw_col_ranks_chunk(n)
        assert 1024 <= C <= 16384 and C & (C - 1) == 0
    # the sorted chunks: every shard and column has room for ceil(n / C) chunks of u64 keys
    for shards, total, max_n, p in ((1, 2, 2, 1), (4, 3000, 1025, 17), (64, 99968, 1562, 64)):
        C = lib.tw_col_ranks_chunk(max_n)
        need = lib.tw_col_ranks_work_bytes(shards, total, max_n, p)
        assert need >= 8 * C * p * (total // C + shards) and need < 1 << 32
    assert lib.tw_col_ranks_work_bytes(-1, 4, 4, 2) == 0
    assert lib.tw_col_ranks_work_bytes(1, 4, 5, 2) == 0
    assert lib.tw_col_ranks_work_bytes(1, 4, 4, 0) == 0
    # 2 M and the two U vectors per shard
    assert lib.tw_kendall_matrix_work_bytes(3, 5, 7) >= 3 * (35 + 5 + 7) * 8
    assert lib.tw_kendall_matrix_work_bytes(1, 1024, 1024) >= 8 << 20
    assert lib.tw_kendall_matrix_work_bytes(1, 0, 4) == 0
    assert lib.tw_kendall_matrix_work_bytes(1, 4, 1025) == 0


def test_hook_ranges(tw):
    L = tw._lib
    for hook, good, bad in (("tw_kendall_matrix_set_width", (16, 32, 0), (8, -1, 64)),
                            ("tw_kendall_matrix_set_flush", (1, 3, 0), (-1, 1 << 24)),
                            ("tw_kendall_matrix_set_plan", (1, 3, 0), (-1,))):
        for v in bad:
            with pytest.raises(ValueError, match=hook):
                L.call(hook, v)
        for v in good:
            L.call(hook, v)
    lib = L.lib()
    L.call("tw_kendall_matrix_set_width", 32)
    try:
        assert lib.tw_kendall_matrix_width(100) == 32
    finally:
        L.call("tw_kendall_matrix_set_width", 0)
    assert lib.tw_kendall_matrix_width(100) == 16


# --------------------------------------------------- the host half on the oracle's integers
@pytest.fixture
def stubbed(tw, monkeypatch):
    import tuplewise.kendall as K
    monkeypatch.setattr(K, "_launch", stub_launch)
    return K


@pytest.mark.parametrize("ties", [False, True])
def test_sign_counts_and_tau_matrix_on_the_oracle(stubbed, ties):
    K = stubbed
    S = table(60, 5, 3 + ties, ties)
    if ties:
        S[:, 2] = 4.0  # a constant column: U = 0, tau-b NaN
    keep = S.copy()
    c = K.sign_counts(S)
    M, Us, Uy, P = o_sign_counts(S)
    assert isinstance(c, K.SignCounts) and type(c.pairs) is int and c.pairs == P
    assert c.M.dtype == np.int64 and c.Us.dtype == np.int64 and c.Uy.dtype == np.int64
    assert np.array_equal(c.M, M) and np.array_equal(c.Us, Us) and np.array_equal(c.Uy, Uy)
    assert np.array_equal(S, keep)
    tb, ta = K.tau_matrix(S), K.tau_matrix(S, variant="a")
    assert tb.dtype == np.float64 and tb.shape == (5, 5) and np.array_equal(K.Un(S), ta)
    for a in range(5):
        for b in range(5):
            pair = np.ascontiguousarray(S[:, [a, b]])
            want = o_kendall_tau_b(pair)
            cd = o_kendall_counts(pair)
            assert ta[a, b] == np.float64((cd[0] - cd[1]) / P)
            if np.isnan(want):
                assert np.isnan(tb[a, b])
            elif a == b:
                assert tb[a, b] == 1.0
            else:
                assert tb[a, b] == want, (a, b)
    Y = table(60, 3, 11, ties)
    tc = K.tau_matrix(S, Y)
    assert tc.shape == (5, 3)
    for a in range(5):
        for b in range(3):
            want = o_kendall_tau_b(np.ascontiguousarray(np.stack([S[:, a], Y[:, b]], 1)))
            assert (np.isnan(want) and np.isnan(tc[a, b])) or tc[a, b] == want


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("N", [3, 8, 64])
def test_blocks_at_two_columns_are_onesamples(stubbed, N, T):
    """UnN / UnNT at p = 2 against the (n, 2) oracle under one seed: the value, the final RNG
    state and the shuffled array.  Fails if the block mean is taken in another order."""
    K = stubbed
    n = 64 * 9 + 5
    S = table(n, 2, 100 + N)
    A, B = S.copy(), S.copy()
    np.random.seed(1234 + N + T)
    got = K.UnN(A, N) if T == 1 else K.UnNT(A, N, T)
    after = np.random.get_state()
    np.random.seed(1234 + N + T)
    want = o_UnN(B, N, "kendall") if T == 1 else o_UnNT(B, N, T, "kendall")
    assert got.shape == (2, 2) and got[0, 1] == want and got[1, 0] == want
    assert same_state(after, np.random.get_state()) and np.array_equal(A, B)


def test_blocks_at_five_columns(stubbed):
    K = stubbed
    S = table(103, 5, 9, ties=True)
    for N, T in ((4, 1), (9, 2)):
        A, B = S.copy(), S.copy()
        np.random.seed(77)
        got = K.UnN(A, N) if T == 1 else K.UnNT(A, N, T)
        after = np.random.get_state()
        np.random.seed(77)
        want = o_UnN_matrix(B, N) if T == 1 else o_UnNT_matrix(B, N, T)
        assert np.array_equal(got, want) and np.array_equal(A, B)
        assert same_state(after, np.random.get_state())
