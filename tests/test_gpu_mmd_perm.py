"""tuplewise.mmd's permutation test on the device (csrc/mmd_perm.hip): every column's three sums
exactly on data whose sums are integers (constant g; |a - b| of distinct integers, which a
row / column swap of the float64 matrix fragments or the float32 accumulator row formula would
change), against the NumPy oracle of tests/test_mmd_perm_cpu.py on Gaussian data, bit for bit
across column positions and launches, permutation_test against the oracle's test (values, p-value,
RNG state), and NaN.

Tolerances: a component is a sum of non-negative g over some of the pooled pairs, Szz and Sxz as
differences of sums of the size of T = the sum over all pooled pairs, so components are compared
at atol 1e-12 * T (the oracle's), the statistic and the null values at the atol of
tests/test_gpu_mmd.py: 1e-12 * (|2 Sxx / (n (n - 1))| + |2 Szz / (m (m - 1))| + |2 Sxz / (n m)|)."""
import functools
import math

import numpy as np
import pytest

from test_gpu_mmd import GUARD, SHAPES, bits, coef, mmd_data, sigma_of
from test_mmd_cpu import KERNELS
from test_mmd_perm_cpu import o_perm_sums, o_perm_test, random_labels
from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# (n, m) as functions of the tile edge T
EXACT_SHAPES = {
    "n2-m2": (lambda T: 2, lambda T: 2),
    "n3-mT-1": (lambda T: 3, lambda T: T - 1),
    "nT-m2": (lambda T: T, lambda T: 2),
    "nT+1-mT+1": (lambda T: T + 1, lambda T: T + 1),
    "n2T+3-m5": (lambda T: 2 * T + 3, lambda T: 5),
}
# one shape of tests/test_gpu_mmd.py's SHAPES for every d
PARITY_SHAPES = ["d1-n2-m2", "d2-n3-m5", "d3-n65-mP+1", "d8-n2P+3-mP+1", "d17-nP-m2",
                 "d37-nP+1-mP+1", "d64-n65-mP+1"]


def perm_counts(C):
    return [1, 15, 16, 17, C - 1, C, C + 1, 2 * C + 1]


@pytest.fixture(scope="module")
def mm(gpu):
    import tuplewise.mmd as m
    return m


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_mmd_tile())


@pytest.fixture(scope="module")
def cols(tw, gpu):
    return int(tw._lib.lib().tw_mmd_perm_cols())


def pack(labels):
    """(P, N) bool -> (N, W) uint32: bit b of word w of row r is labels[32 w + b, r]."""
    P, N = labels.shape
    W = (P + 31) // 32
    by = np.zeros((N, 4 * W), dtype=np.uint8)
    packed = np.packbits(labels.T, axis=1, bitorder="little")
    by[:, :packed.shape[1]] = packed
    return by.view("<u4")


def raw_perm(tw, X, Z, labels, kernel, sigma=None):
    """tw_mmd_perm_sums called directly: the (P, 3) sums, read back from sentinel-filled d_out and
    d_work."""
    import torch
    L = tw._lib
    pool = np.concatenate([X.reshape(len(X), -1), Z.reshape(len(Z), -1)])
    N, d = pool.shape
    P = labels.shape[0]
    if kernel == "gaussian":
        s = sigma if sigma is not None else sigma_of(kernel, d)
        kid, c = L.TW_MMD_GAUSSIAN, -1.0 / (2.0 * s * s)
    else:
        kid, c = coef(tw, kernel, d)
    wd = L.to_device(pool.reshape(-1))
    ld = L.to_device(pack(labels).view(np.int32).reshape(-1))
    nwork = int(L.lib().tw_mmd_perm_work_bytes(N, P)) // 8
    assert nwork > 0
    work = torch.full((nwork + GUARD,), -7.0, dtype=torch.float64, device=wd.device)
    out = torch.full((3 * P + GUARD,), -7.0, dtype=torch.float64, device=wd.device)
    L.call("tw_mmd_perm_sums", wd, N, d, ld, P, kid, c, work, out, L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(-7.0)) and np.all(bits(out[3 * P:]) == bits(-7.0))
    return out[:3 * P].reshape(P, 3)


def labels_for(P, n, N, seed):
    """Row 0 the observed split, the rest random with exactly n ones."""
    labels = random_labels(np.random.RandomState(seed), P, n, N)
    labels[0] = False
    labels[0, :n] = True
    return labels


# ------------------------------------------------------------------------------ exact sums
@pytest.mark.parametrize("d", [1, 17, 64])
@pytest.mark.parametrize("shape", list(EXACT_SHAPES))
def test_constant_g_is_exact(tw, tile, cols, shape, d):
    """Every row identical: g = exp(0) = 1, so Sxx = n (n - 1) / 2, Szz = m (m - 1) / 2 and
    Sxz = n m in every column — a pair visited twice or missed at a tile edge, a diagonal, a
    k-step or a column block changes an integer."""
    fn, fm = EXACT_SHAPES[shape]
    n, m = fn(tile), fm(tile)
    row = np.random.RandomState(d).normal(size=(1, d))
    X, Z = np.repeat(row, n, axis=0), np.repeat(row, m, axis=0)
    want = np.array([n * (n - 1) / 2, m * (m - 1) / 2, n * m], dtype=np.float64)
    for P in perm_counts(cols):
        got = raw_perm(tw, X, Z, labels_for(P, n, n + m, P), "gaussian", 1.0)
        assert np.array_equal(bits(got), bits(np.tile(want, (P, 1)))), (shape, d, P, got)


def int_oracle(a, labels):
    """(P, 3) int64 sums of g = |a_i - a_j| by the definition."""
    a = a.astype(np.int64)
    G = np.abs(a[:, None] - a[None, :])
    S = labels.astype(np.int64)
    sxx = ((S @ G) * S).sum(axis=1) // 2
    szz = (((1 - S) @ G) * (1 - S)).sum(axis=1) // 2
    sxz = ((S @ G) * (1 - S)).sum(axis=1)
    return np.stack([sxx, szz, sxz], axis=1)


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("shape", list(EXACT_SHAPES))
def test_integer_distances_are_exact(tw, tile, cols, shape, d):
    """Energy kernel on distinct integers below 2^20 (d = 8: the other seven coordinates equal
    across rows): g = |a - b| exactly and every sum an integer below 2^53, weighted and
    asymmetric in (anchor, point, column) — the fragment maps' check."""
    fn, fm = EXACT_SHAPES[shape]
    n, m = fn(tile), fm(tile)
    N = n + m
    rng = np.random.RandomState(1000 * d + N)
    a = rng.choice(2 ** 20, size=N, replace=False)
    pool = np.repeat(rng.normal(size=(1, d)), N, axis=0)
    pool[:, d // 2] = a
    X, Z = pool[:n].copy(), pool[n:].copy()
    for P in perm_counts(cols):
        labels = labels_for(P, n, N, 31 * P + d)
        got = raw_perm(tw, X, Z, labels, "energy")
        want = int_oracle(a, labels)
        assert want.max() < 2 ** 53
        assert np.array_equal(got, want.astype(np.float64)), (shape, d, P)
        assert np.array_equal(got.astype(np.int64), want), (shape, d, P)


# ------------------------------------------------------------------------------ float parity
@functools.lru_cache(maxsize=None)
def parity_case(shape, T, C, kernel):
    """One data set, C + 1 label rows and the oracle's sums of every row (computed once, shared,
    never modified): the launches of fewer columns use the first rows."""
    d, fn, fm = SHAPES[shape]
    n, m = fn(T), fm(T)
    X, Z = mmd_data("gauss", n, m, d, 1000 * d + n + m)
    labels = labels_for(C + 1, n, n + m, d)
    return X, Z, labels, o_perm_sums(X, Z, labels, kernel, sigma_of(kernel, d))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_sums_match_the_oracle(tw, mm, tile, cols, shape, kernel):
    X, Z, labels, want = parity_case(shape, tile, cols, kernel)
    tol = RTOL * math.fsum(want[0])  # T: every pooled pair is in exactly one of the three sums
    for P in (1, 17, cols + 1):
        got = mm.permutation_sums(X, Z, labels[:P], kernel, sigma_of(kernel, X.shape[1]))
        assert got.shape == (P, 3) and got.dtype == np.float64
        err = np.abs(got - want[:P]).max()
        print(shape, kernel, P, "max |diff|", err, "tol", tol)
        assert err <= tol, (shape, kernel, P)
        raw = raw_perm(tw, X, Z, labels[:P], kernel)  # the sentinels; the public call's bits
        assert np.array_equal(bits(raw), bits(got))


# ----------------------------------------------------------- column independence, determinism
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_column_depends_on_its_labels_only(tw, tile, cols, kernel):
    n = m = tile + 1
    X, Z = mmd_data("gauss", n, m, 3, 41)
    N, C = n + m, cols
    one = labels_for(2, n, N, 5)[1]  # some split
    observed = labels_for(1, n, N, 0)[0]
    ref = raw_perm(tw, X, Z, one[None, :], kernel)[0]
    ref_obs = raw_perm(tw, X, Z, observed[None, :], kernel)[0]
    assert np.array_equal(bits(raw_perm(tw, X, Z, one[None, :], kernel)[0]), bits(ref))  # twice
    for P, at in ((17, 16), (2 * C + 1, C), (2 * C + 1, 16), (2 * C + 1, 2 * C)):
        for seed in (1, 2):  # other columns: two different sets
            labels = labels_for(P, n, N, 100 * P + seed)
            labels[at] = one
            got = raw_perm(tw, X, Z, labels, kernel)
            assert np.array_equal(bits(got[at]), bits(ref)), (P, at, seed)
            assert np.array_equal(bits(got[0]), bits(ref_obs)), (P, seed)
            assert np.array_equal(bits(raw_perm(tw, X, Z, labels, kernel)), bits(got))  # twice


# -------------------------------------------------------------------------- permutation_test
TESTS = [(65, 129, 3, 257, 7, 0.2), (127, 131, 8, 65, 11, 0.1), (40, 37, 2, 1000, 5, 0.0)]


@functools.lru_cache(maxsize=None)
def perm_case(n, m, d, n_perm, seed, shift, kernel):
    rng = np.random.RandomState(seed)
    X, Z = rng.normal(size=(n, d)), rng.normal(shift, 1.0, size=(m, d))
    np.random.seed(seed + 1)
    want = o_perm_test(X, Z, n_perm, kernel, sigma_of(kernel, d))
    return X, Z, want, np.random.get_state()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,m,d,n_perm,seed,shift", TESTS)
def test_permutation_test(mm, n, m, d, n_perm, seed, shift, kernel):
    X, Z, (stat, null, pvalue, scales), state = perm_case(n, m, d, n_perm, seed, shift, kernel)
    X0, Z0 = X.copy(), Z.copy()
    gap = np.abs(null - stat).min()
    print(kernel, n, m, d, n_perm, "stat", stat, "p", pvalue, "gap / scale", gap / scales.max())
    assert gap >= 1e-9 * scales.max()  # no null value close enough to the statistic to flip
    np.random.seed(seed + 1)
    res = mm.permutation_test(X, Z, n_perm, kernel, sigma_of(kernel, d))
    assert same_state(np.random.get_state(), state)
    assert np.array_equal(bits(X), bits(X0)) and np.array_equal(bits(Z), bits(Z0))
    assert isinstance(res, mm.PermutationResult) and isinstance(res.statistic, np.float64)
    assert res.null.shape == (n_perm,) and res.null.dtype == np.float64
    assert abs(res.statistic - stat) <= RTOL * scales[0]
    assert np.all(np.abs(res.null - null) <= RTOL * scales[1:])
    assert res.pvalue == pvalue
    assert abs(res.statistic - mm.Un(X, Z, kernel, sigma_of(kernel, d))) <= 2 * RTOL * scales[0]


@pytest.mark.parametrize("kernel", KERNELS)
def test_same_sample_twice(mm, kernel):
    X = mmd_data("gauss", 70, 2, 4, 9)[0]
    np.random.seed(2)
    res = mm.permutation_test(X, X.copy(), 99, kernel, sigma_of(kernel, 4))
    assert 1 / 100 <= res.pvalue <= 1.0 and np.isfinite(res.null).all()


# -------------------------------------------------------------------------------------- NaN
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,m,where", [(5, 4, 0), (5, 4, 7), (130, 131, 3), (130, 131, 200)])
def test_nan_fills_every_column(tw, mm, n, m, where, kernel):
    X, Z = mmd_data("gauss", n, m, 5, 3)
    pool = np.concatenate([X, Z])
    pool[where, 2] = np.nan
    labels = labels_for(17, n, n + m, 8)
    got = raw_perm(tw, pool[:n], pool[n:], labels, kernel)
    assert np.isnan(got).all(), got
    np.random.seed(4)
    res = mm.permutation_test(pool[:n], pool[n:], 20, kernel, sigma_of(kernel, 5))
    assert np.isnan(res.statistic) and np.isnan(res.null).all() and res.pvalue == 1 / 21
