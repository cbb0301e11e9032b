"""The launch plans of tw_mmd_perm_sums and tw_mmd_sums that tests/test_gpu_mmd_perm.py and
tests/test_gpu_mmd.py do not reach: more than one tile pair per workgroup of k_mmd_perm (the item
loop's second and third iterations, its barrier before the label words are overwritten, the
accumulators carried across items, a last workgroup with fewer items), more than 256 workgroups a
pass (the stride of k_mmd_perm_reduce) and more than 256 workgroups a block of k_mmd_sums (the
stride of k_self_reduce).

Sums are exact: the energy kernel at d = 1 on N distinct integers below 2^20 gives g = |a - b|
exactly, and with at most 16.6e6 pairs every sum and every partial sum is an integer below 2^45 in
any order of summation, so the device must return the integers of int_oracle_chunked
(tests/test_kernel_range_cpu.py) bit for bit.  The one float case is compared at atol 1e-12 * T
(tests/test_gpu_mmd_perm.py's tolerance) with sums formed in np.longdouble.

Every case first derives (items, ipw, wgs) from tw_mmd_tile(), tw_mmd_perm_cols() and
tw_mmd_perm_work_bytes and asserts the plan it was written for, so a change of the tile or of the
workgroup cap fails here instead of silently testing one item per workgroup again."""
import functools

import numpy as np
import pytest

from test_gpu_mmd import raw_sums
from test_gpu_mmd_perm import bits, labels_for, raw_perm
from test_kernel_range_cpu import int_oracle_chunked
from test_mmd_cpu import o_g
from test_triplets_cpu import o_dist_rows

pytestmark = pytest.mark.gpu

REDUCE_THREADS = 256  # threads of k_mmd_perm_reduce / k_self_reduce: more partials than this stride
# N -> (n, tiles, items, ipw, wgs, items of the last workgroup)
PLANS = {
    2817: (1400, 23, 276, 1, 276, 1),   # the reduce stride only
    3969: (2000, 32, 528, 2, 264, 2),   # two items per workgroup, every workgroup full, the stride
    4100: (7, 33, 561, 2, 281, 1),      # the last workgroup holds one item; Sxx tiny beside T
    5765: (2882, 46, 1081, 3, 361, 1),  # three items per workgroup, the last workgroup one
}


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_mmd_tile())


@pytest.fixture(scope="module")
def cols(tw, gpu):
    return int(tw._lib.lib().tw_mmd_perm_cols())


def check_plan(tw, tile, cols, N):
    """The plan of N pooled rows, derived from the library, against the table."""
    n, tiles, items, ipw, wgs, last = PLANS[N]
    got_tiles = -(-N // tile)
    got_items = got_tiles * (got_tiles + 1) // 2
    wb = int(tw._lib.lib().tw_mmd_perm_work_bytes(N, 1))
    assert wb % (8 * (2 * cols + 16)) == 0
    got_wgs = wb // (8 * (2 * cols + 16))
    got_ipw = -(-got_items // got_wgs)
    got_last = got_items - (got_wgs - 1) * got_ipw
    print("N", N, "tiles", got_tiles, "items", got_items, "ipw", got_ipw, "wgs", got_wgs, "last", got_last)
    assert (got_tiles, got_items, got_ipw, got_wgs, got_last) == (tiles, items, ipw, wgs, last)
    assert got_wgs > REDUCE_THREADS and -(-got_items // got_ipw) == got_wgs
    return n


@functools.lru_cache(maxsize=None)
def int_case(N, n, P):
    """N distinct integers below 2^20, P label rows (row 0 the observed split) and the integer
    sums of every row (computed once, shared, never modified): launches of fewer columns use the
    first rows."""
    rng = np.random.RandomState(N)
    a = rng.choice(2 ** 20, size=N, replace=False)
    labels = labels_for(P, n, N, N + 1)
    want = int_oracle_chunked(a, labels)
    assert want.max() < 2 ** 45 and want.min() > 0
    return a, labels, want


@pytest.mark.parametrize("N", list(PLANS))
def test_integer_distances_are_exact(tw, tile, cols, N):
    n = check_plan(tw, tile, cols, N)
    a, labels, want = int_case(N, n, cols + 1)
    pool = a.astype(np.float64).reshape(N, 1)
    for P in (1, 17, cols + 1):
        got = raw_perm(tw, pool[:n], pool[n:], labels[:P], "energy")
        assert np.array_equal(got, want[:P].astype(np.float64)), (N, P)
        assert np.array_equal(got.astype(np.int64), want[:P]), (N, P)


@pytest.mark.parametrize("N", [3969, 5765])
def test_constant_g_is_exact(tw, tile, cols, N):
    """Every row identical under the Gaussian kernel: g = 1, so the sums are n (n - 1) / 2,
    m (m - 1) / 2 and n m in every column."""
    n = check_plan(tw, tile, cols, N)
    m = N - n
    pool = np.full((N, 1), 0.75)
    want = np.array([n * (n - 1) / 2, m * (m - 1) / 2, n * m], dtype=np.float64)
    labels = int_case(N, n, cols + 1)[1]
    for P in (1, 17, cols + 1):
        got = raw_perm(tw, pool[:n], pool[n:], labels[:P], "gaussian", 1.0)
        assert np.array_equal(bits(got), bits(np.tile(want, (P, 1)))), (N, P, got)


def test_float_sums_two_items_per_workgroup(tw, tile, cols):
    """N = 3969, d = 3, Gaussian, three columns against sums formed in np.longdouble from the
    oracle's g (row chunks of 512, so no N x N array is held); the same launch twice gives the
    same bits, and column 0 has the bits of that column run alone."""
    N, d, P = 3969, 3, 3
    n = check_plan(tw, tile, cols, N)
    rng = np.random.RandomState(7)
    W = np.concatenate([rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(N - n, d))])
    labels = labels_for(P, n, N, 3)
    sigma = float(np.sqrt(d))
    S = labels.astype(np.longdouble)
    two_sxx = np.zeros(P, dtype=np.longdouble)
    two_szz, sxz = two_sxx.copy(), two_sxx.copy()
    for r0 in range(0, N, 512):
        r1 = min(N, r0 + 512)
        G = o_g(o_dist_rows(W[r0:r1], W), "gaussian", sigma)
        G[np.arange(r1 - r0), np.arange(r0, r1)] = 0.0  # no pair (i, i)
        R = G.astype(np.longdouble)
        for p in range(P):
            row1 = (R * S[p, r0:r1, None]).sum(axis=0)        # over the chunk's first-sample rows
            row0 = (R * (1 - S[p, r0:r1, None])).sum(axis=0)
            two_sxx[p] += (row1 * S[p]).sum()
            two_szz[p] += (row0 * (1 - S[p])).sum()
            sxz[p] += (row1 * (1 - S[p])).sum()
    want = np.stack([two_sxx / 2, two_szz / 2, sxz], axis=1)
    T = float(want[0].sum())
    got = raw_perm(tw, W[:n], W[n:], labels, "gaussian")
    err = np.abs(got.astype(np.longdouble) - want).max()
    print("max |diff|", float(err), "tol", 1e-12 * T, "T", T)
    assert err <= 1e-12 * T
    assert np.array_equal(bits(raw_perm(tw, W[:n], W[n:], labels, "gaussian")), bits(got))
    alone = raw_perm(tw, W[:n], W[n:], labels[:1], "gaussian")
    assert np.array_equal(bits(alone[0]), bits(got[0]))


def test_mmd_sums_reduce_stride(tw, tile):
    """tw_mmd_sums on one block of n = m = 16 T + 1 integers (energy, d = 1): more than 256
    workgroups' partials for k_self_reduce to stride over, the three sums exact; beside a second
    block of n = m = 2 the big block's bits are unchanged."""
    n = m = 16 * tile + 1
    tx = -(-n // tile)
    items = tx * (tx + 1) + tx * tx  # two triangles and the rectangle
    wb = int(tw._lib.lib().tw_mmd_work_bytes(1, n, m))
    assert wb % 24 == 0
    per = wb // 24
    print("n = m", n, "tiles", tx, "items", items, "workgroups", per)
    assert per > REDUCE_THREADS and per * 2 >= items > (per - 1) * 2  # 2 items per workgroup
    rng = np.random.RandomState(16)
    a = rng.choice(2 ** 20, size=n + m + 4, replace=False)
    labels = np.zeros((1, n + m), dtype=bool)
    labels[0, :n] = True
    want = int_oracle_chunked(a[:n + m], labels)[0]
    X, Z = a[:n].astype(np.float64).reshape(n, 1), a[n:n + m].astype(np.float64).reshape(m, 1)
    got = raw_sums(tw, X, Z, [0, n], [0, m], "energy")
    assert np.array_equal(got[0], want.astype(np.float64)) and np.array_equal(got[0].astype(np.int64), want)
    tail = a[n + m:].astype(np.float64).reshape(4, 1)
    X2, Z2 = np.concatenate([X, tail[:2]]), np.concatenate([Z, tail[2:]])
    both = raw_sums(tw, X2, Z2, [0, n, n + 2], [0, m, m + 2], "energy")
    assert np.array_equal(bits(both[0]), bits(got[0]))
    assert np.array_equal(both[1], [abs(tail[0, 0] - tail[1, 0]), abs(tail[2, 0] - tail[3, 0]),
                                    np.abs(tail[:2] - tail[2:].T).sum()])
