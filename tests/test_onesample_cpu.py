"""tuplewise.onesample without a GPU: the module imports, argument errors come before any device
work, and the oracle the GPU tests compare against (a plain NumPy restatement: np.triu_indices
all-pairs with the comparison definitions, plus the same np.random calls in the same order)
agrees with scipy.stats.kendalltau and np.var."""
import math

import numpy as np
import pytest

KERNELS = ["gini", "var", "kendall"]


# ------------------------------------------------------------------------------------ oracle
def o_items(S, kernel):
    S = np.asarray(S)
    if kernel == "kendall":
        assert S.ndim == 2 and S.shape[1] == 2 and S.dtype in (np.float64, np.int64)
        return S
    return np.asarray(S, np.float64).reshape(-1)


def o_kendall_terms(si, sj):
    """(C, D, Tx, Ty, Txy) of the given point pairs, by comparisons only."""
    with np.errstate(invalid="ignore"):
        ai, bi, aj, bj = si[:, 0], si[:, 1], sj[:, 0], sj[:, 1]
        ga, la, gb, lb = ai > aj, ai < aj, bi > bj, bi < bj
        ea, eb = ai == aj, bi == bj
    return (int(np.sum((ga & gb) | (la & lb))), int(np.sum((ga & lb) | (la & gb))),
            int(np.sum(ea)), int(np.sum(eb)), int(np.sum(ea & eb)))


def o_pairs_value(S, i, j, kernel):
    """The mean of h over the index pairs (i, j)."""
    S = o_items(S, kernel)
    if kernel == "kendall":
        c, d = o_kendall_terms(S[i], S[j])[:2]
        return np.float64((c - d) / len(i))
    d = S[i] - S[j]
    return np.mean(np.abs(d)) if kernel == "gini" else np.mean(d * d / 2)


def o_Un(S, kernel="gini"):
    n = o_items(S, kernel).shape[0]
    i, j = np.triu_indices(n, 1)
    return o_pairs_value(S, i, j, kernel)


def o_kendall_counts(S):
    S = o_items(S, "kendall")
    i, j = np.triu_indices(S.shape[0], 1)
    return o_kendall_terms(S[i], S[j])


def o_kendall_tau_b(S):
    c, d, tx, ty, _ = o_kendall_counts(S)
    n = np.asarray(S).shape[0]
    p = n * (n - 1) // 2
    fx, fy = math.sqrt(float(p - tx)), math.sqrt(float(p - ty))
    return np.float64("nan") if fx == 0.0 or fy == 0.0 else np.float64((c - d) / (fx * fy))


def o_UB(S, B, kernel):
    n = np.asarray(S).shape[0]
    i = np.random.randint(0, n, B)
    j = np.random.randint(0, n - 1, B)
    j += (j >= i)
    return o_pairs_value(S, i, j, kernel)


def o_UN(S, N, f_block):
    np.random.shuffle(S)
    k = int(S.shape[0] / N)
    return np.mean([f_block(S[b * k:(b + 1) * k]) for b in range(N)])


def o_UnN(S, N, kernel):
    return o_UN(S, N, lambda s: o_Un(s, kernel))


def o_UnNB(S, N, B, kernel):
    return o_UN(S, N, lambda s: o_UB(s, B, kernel))


def o_UnNT(S, N, T, kernel):
    return np.mean([o_UnN(S, N, kernel) for _ in range(T)])


def o_UnNBT(S, N, B, T, kernel):
    return np.mean([o_UnNB(S, N, B, kernel) for _ in range(T)])


def sample(n, kernel, seed, ties=False):
    rng = np.random.RandomState(seed)
    if kernel == "kendall":
        if ties:
            return rng.randint(0, 4, size=(n, 2)).astype(np.float64)
        a = rng.normal(size=n)
        return np.ascontiguousarray(np.stack([a, 0.6 * a + rng.normal(size=n)], axis=1))
    return rng.randint(0, 4, size=n).astype(np.float64) if ties else rng.normal(1.0, 2.0, n)


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [2, 3, 255, 257, 2000])
def test_oracle_tau_b_is_scipys(n, ties):
    from scipy.stats import kendalltau
    S = sample(n, "kendall", n + ties, ties)
    want = kendalltau(S[:, 0], S[:, 1]).statistic
    got = o_kendall_tau_b(S)
    if np.isnan(want):
        assert np.isnan(got)
    else:
        assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [2, 3, 255, 257, 2000])
def test_oracle_var_is_numpys(n, ties):
    S = sample(n, "var", 3 * n + ties, ties)
    want = np.var(S, ddof=1)
    assert abs(o_Un(S, "var") - want) <= 7e-16 * abs(want)


def test_oracle_counts_partition_the_pairs():
    S = sample(257, "kendall", 5, ties=True)
    c, d, tx, ty, txy = o_kendall_counts(S)
    assert c + d + tx + ty - txy == 257 * 256 // 2 and min(c, d, txy) > 0


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.onesample as os1
    for name in ("Un", "kendall_counts", "kendall_tau_b", "UB_indices", "UB", "UN", "UnN", "UnNT",
                 "UnNB", "UnNBT"):
        assert callable(getattr(os1, name)), name
    assert "onesample" not in tw.__all__


def test_argument_errors_need_no_device(tw):
    import tuplewise.onesample as os1
    S = np.arange(10.0)
    K = np.arange(20.0).reshape(10, 2)
    state = np.random.get_state()
    for call in (lambda: os1.Un(S, "prod"), lambda: os1.UB(S, 3, "AUC"),
                 lambda: os1.UB_indices(S, [0], [1], "x"), lambda: os1.UnN(S, 2, "x"),
                 lambda: os1.UnNT(S, 2, 2, "x"), lambda: os1.UnNB(S, 2, 3, "x"),
                 lambda: os1.UnNBT(S, 2, 3, 2, "x")):
        with pytest.raises(AssertionError):
            call()
    for call in (lambda: os1.Un(S[:1]), lambda: os1.Un(S[:0], "var"),
                 lambda: os1.Un(K[:1], "kendall"), lambda: os1.kendall_counts(K[:1]),
                 lambda: os1.kendall_tau_b(K[:0]), lambda: os1.UB(S[:1], 4, "gini"),
                 # a block of fewer than 2 points
                 lambda: os1.UnN(S, 6, "gini"), lambda: os1.UnNT(S, 10, 2, "var"),
                 lambda: os1.UnNB(K, 7, 3, "kendall"), lambda: os1.UnNBT(S, 6, 3, 2, "gini"),
                 lambda: os1.UN(S, 6, lambda s: 0.0),
                 # a wrong shape, dtype or layout for "kendall"
                 lambda: os1.Un(S, "kendall"), lambda: os1.Un(np.zeros((4, 3)), "kendall"),
                 lambda: os1.kendall_counts(np.zeros((4, 2), np.float32)),
                 lambda: os1.kendall_tau_b(np.zeros((2, 4)).T),
                 lambda: os1.UnN(S, 2, "kendall"),
                 lambda: os1.UB_indices(np.zeros((4, 2, 1)), [0], [1], "kendall"),
                 lambda: os1.Un(np.zeros((4, 2)), "gini")):
        with pytest.raises(ValueError):
            call()
    # nothing was shuffled and nothing was drawn on the way to those errors
    assert np.array_equal(S, np.arange(10.0)) and np.array_equal(K.reshape(-1), np.arange(20.0))
    after = np.random.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.onesample as os1
    with pytest.raises(RuntimeError, match="no HIP device"):
        os1.Un(np.arange(5.0))
    with pytest.raises(RuntimeError, match="no HIP device"):
        os1.UB_indices(np.arange(5.0), [0, 1], [2, 3], "var")


@pytest.mark.parametrize("entry", ["tw_self_pairs", "tw_self_pairs_idx32"])
def test_native_argument_errors(tw, entry):
    L = tw._lib
    lib = L.lib()
    fn = getattr(lib, entry)

    def call(n_shards, dtype, kern):
        if entry == "tw_self_pairs":
            return fn(None, None, n_shards, 4, dtype, kern, None, None, None)
        return fn(None, None, None, None, n_shards, 4, dtype, kern, None, None, None)

    for args, word in (((-1, L.TW_F64, L.TW_SELF_GINI), b"n_shards"),
                       ((1, L.TW_F64, 3), b"kern"), ((1, L.TW_F64, -1), b"kern"),
                       ((1, 2, L.TW_SELF_KENDALL), b"dtype"),
                       ((1, L.TW_I64, L.TW_SELF_GINI), b"TW_I64"),
                       ((1, L.TW_I64, L.TW_SELF_VAR), b"TW_I64")):
        assert call(*args) == L.TW_ERR_ARG, args
        msg = lib.tw_last_error()
        assert word in msg and entry.encode() in msg, (args, msg)
    assert call(0, L.TW_I64, L.TW_SELF_KENDALL) == L.TW_OK  # no shards: nothing to do


def test_tile_and_work_sizes(tw):
    lib = tw._lib.lib()
    T = lib.tw_self_pairs_tile()
    assert 16 <= T <= 1024
    # one 8-byte slot (five for Kendall) per block: a sane, monotone size
    small, big = lib.tw_self_pairs_work_bytes(1, 2), lib.tw_self_pairs_work_bytes(64, 15625)
    assert 8 <= small <= big < 1 << 26
    assert 8 <= lib.tw_self_pairs_idx_work_bytes(1, 1) <= lib.tw_self_pairs_idx_work_bytes(64, 10 ** 6)
