"""The sorted path of tuplewise.onesample without a GPU: the O(n log n) NumPy
oracle the GPU tests compare against (lexsort, run lengths, a merge-sort inversion count; the
sorted Gini formula with math.fsum) agrees with the all-pairs oracle of test_onesample_cpu.py,
the algo= argument errors come before any device work, shuffle or RNG draw, and the choice
between the two algorithms is one pure function."""
import math

import numpy as np
import pytest

from test_gpu_onesample import edge_samples
from test_onesample_cpu import o_kendall_counts, o_Un, sample


# ------------------------------------------------------------------------------------ oracle
def _nan(x):
    return np.isnan(x) if x.dtype.kind == "f" else np.zeros(x.shape, bool)


def _tied_pairs(*cols):
    """Pairs inside the runs of equal rows of columns already sorted together."""
    n = len(cols[0])
    if n == 0:
        return 0
    change = np.zeros(n - 1, bool)
    for c in cols:
        change |= c[1:] != c[:-1]
    m = np.diff(np.flatnonzero(np.concatenate([[True], change, [True]])))
    return sum(int(k) * (int(k) - 1) // 2 for k in m)


def inversions(seq):
    """#{i < j : seq[i] > seq[j]} by a bottom-up merge sort: every element of a right run counts
    the elements of its left run above it (searchsorted)."""
    seq = np.array(seq)
    n, total, w = len(seq), 0, 1
    while w < n:
        for lo in range(0, n - w, 2 * w):
            left, right = seq[lo:lo + w], seq[lo + w:lo + 2 * w]
            total += int(np.sum(len(left) - np.searchsorted(left, right, side="right")))
            seq[lo:lo + 2 * w] = np.sort(seq[lo:lo + 2 * w], kind="stable")
        w *= 2
    return total


def s_kendall_counts(S):
    """(C, D, Tx, Ty, Txy) of the (n, 2) sample: ties from run lengths over each coordinate's
    non-NaN points; over the v points without a NaN sorted by (a, b), D = the strict inversions
    of b and C = v (v - 1) / 2 - Tx' - Ty' + Txy - D (primed: among those points)."""
    a, b = S[:, 0], S[:, 1]
    na, nb = _nan(a), _nan(b)
    tx, ty = _tied_pairs(np.sort(a[~na])), _tied_pairs(np.sort(b[~nb]))
    clean = ~na & ~nb
    a, b = a[clean], b[clean]
    order = np.lexsort((b, a))
    a, b = a[order], b[order]
    v = len(a)
    txy = _tied_pairs(a, b)
    d = inversions(b)
    c = v * (v - 1) // 2 - _tied_pairs(a) - _tied_pairs(np.sort(b)) + txy - d
    return (c, d, tx, ty, txy)


def s_gini_sum(S):
    """sum_{i<j} |s_i - s_j| = sum_i (2 i - n + 1) s_(i); NumPy's elementwise outcome for
    non-finite values."""
    s = np.sort(np.asarray(S, np.float64).reshape(-1))
    n = len(s)
    if n < 2:
        return 0.0
    if np.isnan(s).any() or np.sum(s == np.inf) >= 2 or np.sum(s == -np.inf) >= 2:
        return float("nan")
    if np.isinf(s).any():
        return float("inf")
    return math.fsum((2 * i - n + 1) * x for i, x in enumerate(s.tolist()))


def s_Un(S, kernel):
    n = np.asarray(S).shape[0]
    pairs = n * (n - 1) // 2
    if kernel == "kendall":
        c, d = s_kendall_counts(S)[:2]
        return np.float64((c - d) / pairs)
    return np.float64(s_gini_sum(S) / np.float64(pairs))


def extreme_int64(n, seed):
    """int64 points among INT64_MAX (the order key of chunk padding), INT64_MIN and neighbours."""
    hi, lo = np.iinfo(np.int64).max, np.iinfo(np.int64).min
    vals = np.array([hi, hi - 1, lo, lo + 1, 0, -1], dtype=np.int64)
    return vals[np.random.RandomState(seed).randint(0, len(vals), size=(n, 2))]


# ------------------------------------------------------------------- the oracle's own checks
def test_inversions_against_all_pairs():
    rng = np.random.RandomState(0)
    for n in (0, 1, 2, 3, 64, 65, 1000):
        for top in (4, 10 ** 6):
            x = rng.randint(0, top, n)
            i, j = np.triu_indices(n, 1)
            assert inversions(x) == int(np.sum(x[i] > x[j])), (n, top)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [2, 3, 255, 257, 2000])
def test_sorted_kendall_oracle_is_the_all_pairs_oracle(n, ties):
    S = sample(n, "kendall", n + ties, ties)
    assert s_kendall_counts(S) == o_kendall_counts(S)
    assert s_Un(S, "kendall") == o_Un(S, "kendall")


@pytest.mark.parametrize("which", ["nonfinite", "int64", "extreme"])
def test_sorted_kendall_oracle_on_edge_data(which):
    S = extreme_int64(500, 1) if which == "extreme" else edge_samples()[which]
    want = o_kendall_counts(S)
    assert s_kendall_counts(S) == want
    if which == "extreme":
        assert (S == np.iinfo(np.int64).max).any() and (S == np.iinfo(np.int64).min).any()
        assert min(want) > 0
    if which == "nonfinite":  # every kind of point: clean, one NaN on either side, two NaN
        na, nb = np.isnan(S[:, 0]), np.isnan(S[:, 1])
        assert (na & nb).any() and (na & ~nb).any() and (~na & nb).any() and (~na & ~nb).any()


def test_sorted_kendall_oracle_on_a_nan_column():
    S = sample(257, "kendall", 8, ties=True)
    S[:, 0] = np.nan
    c, d, tx, ty, txy = s_kendall_counts(S)
    assert (c, d, tx, txy) == (0, 0, 0, 0) and ty > 0
    assert (c, d, tx, ty, txy) == o_kendall_counts(S)


@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [2, 3, 255, 257, 2000])
def test_sorted_gini_oracle_is_the_all_pairs_oracle(n, ties):
    S = sample(n, "gini", 5 * n + ties, ties)
    got, want = s_Un(S, "gini"), o_Un(S, "gini")
    if ties:  # small integers: every sum is exact
        assert got == want
    assert np.isclose(got, want, rtol=1e-12, atol=1e-15), (got, want)


@pytest.mark.parametrize("extra", [[np.nan], [np.inf], [np.inf, np.inf], [np.inf, -np.inf],
                                   [-np.inf, -np.inf], [-np.inf]])
def test_sorted_gini_oracle_non_finite(extra):
    S = np.concatenate([sample(50, "gini", 3), extra])
    with np.errstate(invalid="ignore"):
        want = o_Un(S, "gini")
    got = s_Un(S, "gini")
    assert (np.isnan(got) and np.isnan(want)) or got == want, (got, want)


# ------------------------------------------------------------------------ the module, no GPU
def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_algo_argument_errors_need_no_device(tw):
    import tuplewise.onesample as os1
    S = np.arange(10.0)
    K = np.arange(20.0).reshape(10, 2)
    np.random.seed(4)
    state = np.random.get_state()
    for call in (lambda: os1.Un(S, "gini", algo="merge"), lambda: os1.Un(K, "kendall", algo=""),
                 lambda: os1.kendall_counts(K, algo="Sorted"),
                 lambda: os1.kendall_tau_b(K, algo="x"),
                 lambda: os1.UnN(S, 2, "gini", algo="x"), lambda: os1.UnN(K, 2, "kendall", algo=0),
                 lambda: os1.UnNT(S, 2, 3, "var", algo="x"),
                 # the variance has no sorted path
                 lambda: os1.Un(S, "var", algo="sorted"),
                 lambda: os1.UnN(S, 2, "var", algo="sorted"),
                 lambda: os1.UnNT(S, 2, 3, "var", algo="sorted")):
        with pytest.raises(ValueError, match="algo"):
            call()
    assert np.array_equal(S, np.arange(10.0)) and np.array_equal(K.reshape(-1), np.arange(20.0))
    assert same_state(state, np.random.get_state())
    # an unknown kernel is still the first complaint
    with pytest.raises(AssertionError):
        os1.Un(S, "prod", algo="sorted")


def test_choose_algo(tw):
    import tuplewise.onesample as os1
    m = os1.SORTED_MIN_N
    assert isinstance(m, int) and m > 5000  # every sample of the existing tests stays on "pairs"
    for max_n, auto in ((0, "pairs"), (m - 1, "pairs"), (m, "sorted"), (m + 1, "sorted")):
        assert os1._choose_algo("kendall", "auto", max_n) == auto
        assert os1._choose_algo("kendall", None, max_n) == auto  # Kendall's default is "auto"
        assert os1._choose_algo("gini", "auto", max_n) == auto
        assert os1._choose_algo("gini", None, max_n) == "pairs"  # Gini's default is "pairs"
        assert os1._choose_algo("var", "auto", max_n) == "pairs"
        assert os1._choose_algo("var", None, max_n) == "pairs"
        for kernel in ("gini", "kendall"):
            assert os1._choose_algo(kernel, "pairs", max_n) == "pairs"
            assert os1._choose_algo(kernel, "sorted", max_n) == "sorted"
    with pytest.raises(ValueError):
        os1._choose_algo("var", "sorted", m)
    with pytest.raises(ValueError):
        os1._choose_algo("kendall", "fast", m)


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()

    def call(n_shards=1, total=8, max_n=8, dtype=L.TW_F64, kern=L.TW_SELF_KENDALL, chunk=0):
        return lib.tw_self_sorted(None, None, n_shards, total, max_n, dtype, kern, chunk, None,
                                  None, None)

    for kw, word in ((dict(n_shards=-1), b"n_shards"), (dict(max_n=-1), b"max_n"),
                     (dict(total=4), b"total_n"), (dict(kern=L.TW_SELF_VAR), b"TW_SELF_VAR"),
                     (dict(kern=3), b"kern"), (dict(dtype=2), b"dtype"),
                     (dict(dtype=L.TW_I64, kern=L.TW_SELF_GINI), b"TW_I64"),
                     (dict(chunk=512), b"chunk"), (dict(chunk=3000), b"chunk"),
                     (dict(chunk=32768), b"chunk"), (dict(chunk=-1024), b"chunk"),
                     (dict(total=2 ** 31, max_n=2 ** 31), b"2^31"),
                     (dict(), b"d_work")):
        assert call(**kw) == L.TW_ERR_ARG, kw
        msg = lib.tw_last_error()
        assert word in msg and b"tw_self_sorted" in msg, (kw, msg)
    assert call(n_shards=0, total=0, max_n=0) == L.TW_OK  # no shards: nothing to do
    assert call(n_shards=0, total=2 ** 31 - 1, max_n=2 ** 31 - 1) == L.TW_OK  # the largest shard


def test_chunk_and_work_sizes(tw):
    L = tw._lib
    lib = L.lib()
    C = lib.tw_self_sorted_chunk()
    assert 1024 <= C <= 16384 and C & (C - 1) == 0
    for kern in (L.TW_SELF_GINI, L.TW_SELF_KENDALL):
        small = lib.tw_self_sorted_work_bytes(1, 2, 2, kern, 0)
        big = lib.tw_self_sorted_work_bytes(64, 10 ** 6, 15625, kern, 0)
        assert 8 <= small <= big < 1 << 28  # a few 8-byte words per item
        assert lib.tw_self_sorted_work_bytes(1, 10 ** 6, 10 ** 6, kern, 1024) > 8 * 10 ** 6
    assert lib.tw_self_sorted_work_bytes(1, 8, 8, L.TW_SELF_VAR, 0) == 0
    assert lib.tw_self_sorted_work_bytes(1, 8, 8, L.TW_SELF_GINI, 1000) == 0
