"""tuplewise.bandwidth on the device: exact order statistics of pairwise squared distances, the
median distance and sigma="median" in the kernel modules.

The oracle is NumPy, here: D by the fixed-order loop (acc = acc + t * t over the coordinates,
vectorised over the pairs), then np.sort.  Every comparison is EXACT, on the uint64 views of the
doubles: a radix select over integer histograms has no rounding, and D has the same bits in NumPy
and on the device (one arithmetic order, never fused).  There is no tolerance in this file."""
import ctypes

import numpy as np
import pytest

from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def bw(gpu):
    import tuplewise.bandwidth as b
    return b


def rows(kind, n, d, seed):
    rng = np.random.RandomState(seed)
    if kind == "ints":  # most pairs tie
        return rng.randint(0, 3, size=(n, d)).astype(np.float64)
    if kind == "equal":  # every D = 0
        return np.tile(rng.normal(size=(1, d)), (n, 1))
    A = rng.normal(size=(n, d))
    if kind == "huge":  # D of distinct rows overflows to +inf
        return A * 1e200
    if kind == "tiny":  # every square underflows: D = 0
        return A * 1e-170
    if kind == "subnormal":  # squares around 1e-320: D is subnormal (or 0)
        return A * 1e-160
    if kind == "sorted":
        return A[np.lexsort(A.T[::-1])]
    assert kind == "gauss"
    return A


def dist_pairs(A, B):
    acc = np.zeros(A.shape[0])
    with np.errstate(over="ignore", under="ignore"):
        for c in range(A.shape[1]):
            t = A[:, c] - B[:, c]
            acc = acc + t * t
    return acc


def o_dist(X, Z, pairs):
    """The M squared distances of the pair set, unsorted."""
    if pairs == "pooled":
        X, Z, pairs = np.concatenate([X, Z]), None, "within"
    if pairs == "within":
        i, j = np.triu_indices(X.shape[0], 1)
        return dist_pairs(X[i], X[j])
    i, k = np.divmod(np.arange(X.shape[0] * Z.shape[0]), Z.shape[0])
    return dist_pairs(X[i], Z[k])


def u64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def ranks_for(M, seed):
    r = [0, M - 1, (M - 1) // 2, M // 2]
    return np.array(r + list(np.random.RandomState(seed).randint(0, M, 20)), dtype=np.int64)


# (n, d, data): one pair, three pairs, a full tile, a one-row tail tile, items split across
# workgroups, several tile rows; d = 1, 8, 9, 63, 64; every kind of data
WITHIN = [(2, 1, "gauss"), (2, 8, "huge"), (3, 8, "ints"), (128, 9, "gauss"), (129, 63, "gauss"),
          (257, 64, "sorted"), (600, 8, "gauss"), (129, 8, "equal"), (129, 9, "huge"),
          (257, 1, "tiny"), (257, 8, "subnormal"), (600, 1, "ints"), (257, 8, "ints"),
          (128, 64, "ints"), (600, 63, "sorted"), (129, 1, "gauss")]
CROSS = [(1, 1, 1, "gauss"), (1, 1, 64, "equal"), (130, 5, 8, "gauss"), (257, 129, 9, "ints"),
         (130, 5, 64, "huge"), (257, 129, 63, "tiny"), (130, 5, 1, "equal"),
         (257, 129, 8, "sorted"), (257, 129, 1, "subnormal"), (130, 5, 63, "gauss")]


def check_select(bw, X, Z, pairs):
    want = np.sort(o_dist(X, Z, pairs))
    M = len(want)
    ranks = ranks_for(M, M)
    results = []
    for cap in (0, None, M, max(1, M // 8)):  # never gather, the default, at once, after a pass
        got = bw.order_statistics(X, Z, ranks, pairs, _gather_cap=cap)
        assert got.dtype == np.float64 and got.shape == ranks.shape
        results.append(u64(got))
    for r in results:
        assert np.array_equal(r, u64(want[ranks]))
    return want


@pytest.mark.parametrize("n,d,kind", WITHIN, ids=lambda v: str(v))
def test_within_order_statistics_are_exact(bw, n, d, kind):
    X = rows(kind, n, d, 100 * n + d)
    want = check_select(bw, X, None, "within")
    if kind == "equal" or kind == "tiny":
        assert not want.any()
    if kind == "huge":
        assert np.isinf(want).all()
    if kind == "subnormal":
        assert (want[want > 0] < np.finfo(np.float64).tiny).any()


@pytest.mark.parametrize("n,m,d,kind", CROSS, ids=lambda v: str(v))
def test_cross_order_statistics_are_exact(bw, n, m, d, kind):
    A = rows(kind, n + m, d, 100 * n + d)
    check_select(bw, A[:n].copy(), A[n:].copy(), "cross")


def test_pooled_is_within_on_the_concatenation(bw):
    X, Z = rows("gauss", 70, 8, 1), rows("gauss", 61, 8, 2) + 0.5
    want = check_select(bw, X, Z, "pooled")
    assert len(want) == 131 * 130 // 2
    assert np.array_equal(u64(bw.order_statistics(np.concatenate([X, Z]), ranks=[5, 77])),
                          u64(want[[5, 77]]))
    # a 1-D sample is d = 1; scalar ranks give a 0-d array; duplicated ranks are allowed
    x = rows("gauss", 50, 1, 3)
    w1 = np.sort(o_dist(x, None, "within"))
    assert u64(bw.order_statistics(x[:, 0].copy(), ranks=7)).item() == u64(w1[7]).item()
    got = bw.order_statistics(x, ranks=np.array([[3, 3], [0, 1224]]))
    assert np.array_equal(u64(got), u64(w1[[[3, 3], [0, 1224]]]))


@pytest.mark.parametrize("pairs,n,m", [("within", 3, 0), ("within", 129, 0), ("within", 130, 0),
                                       ("pooled", 64, 66), ("pooled", 64, 65), ("cross", 9, 7),
                                       ("cross", 10, 7)])
def test_median_distance_is_numpys(bw, pairs, n, m):
    """np.median(np.sqrt(D)) bit for bit, for odd and even M."""
    A = rows("gauss", n + m, 8, n)
    X, Z = (A, None) if pairs == "within" else (A[:n].copy(), A[n:].copy())
    D = o_dist(X, Z, pairs)
    got = bw.median_distance(X, Z, pairs)
    assert isinstance(got, np.float64)
    assert u64(got).item() == u64(np.median(np.sqrt(D))).item(), (len(D), got)
    ties = rows("ints", n + m, 2, n)
    Xt, Zt = (ties, None) if pairs == "within" else (ties[:n].copy(), ties[n:].copy())
    assert u64(bw.median_distance(Xt, Zt, pairs)).item() == \
        u64(np.median(np.sqrt(o_dist(Xt, Zt, pairs)))).item()


def test_quantile_distances(bw):
    X = rows("gauss", 200, 9, 5)
    want = np.sqrt(np.sort(o_dist(X, None, "within")))
    M = len(want)
    q = np.array([0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 1.0])
    lo = bw.quantile_distances(X, q=q, method="lower")
    hi = bw.quantile_distances(X, q=q, method="higher")
    assert np.array_equal(u64(lo), u64(want[np.floor(q * (M - 1)).astype(np.int64)]))
    assert np.array_equal(u64(hi), u64(want[np.ceil(q * (M - 1)).astype(np.int64)]))
    assert np.array_equal(u64(lo), u64(np.quantile(want, q, method="lower")))
    assert np.array_equal(u64(hi), u64(np.quantile(want, q, method="higher")))
    assert bw.quantile_distances(X, q=0.5).shape == ()


# ------------------------------------------------------------------------- the raw entry points
def host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def raw_setup(tw, pairs, n, m, d, kind="gauss"):
    L = tw._lib
    A = rows(kind, n + m, d, 9)
    X, Z = A[:n].copy(), (A[n:].copy() if m else None)
    keys = u64(o_dist(X, Z, pairs))
    xd = L.to_device(X.reshape(-1))
    zd = L.to_device(Z.reshape(-1)) if m else None
    pid = L.TW_DIST_WITHIN if pairs == "within" else L.TW_DIST_CROSS
    return L, keys, xd, zd, pid


def o_hist(keys, prefixes, bits, shift, width, bins):
    out = np.zeros((len(prefixes), bins), dtype=np.uint64)
    for g, (p, b) in enumerate(zip(prefixes, bits)):
        sel = keys[(keys >> np.uint64(63 - b)) == np.uint64(p)]
        digits = ((sel >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64)
        out[g, :1 << width] = np.bincount(digits, minlength=1 << width)
    return out


@pytest.mark.parametrize("pairs,n,m", [("within", 129, 0), ("cross", 130, 5)])
def test_raw_histogram_is_bincount(tw, gpu, pairs, n, m):
    import torch
    L, keys, xd, zd, pid = raw_setup(tw, pairs, n, m, 8)
    bins = 1 << int(L.lib().tw_dist_select_digit_bits())
    assert bins == 2048 and int(L.lib().tw_dist_select_max_groups()) == 8
    assert int(L.lib().tw_dist_hist_bytes(3)) == 3 * bins * 8
    assert int(L.lib().tw_dist_hist_bytes(0)) == 0 == int(L.lib().tw_dist_hist_bytes(9))
    expo = int(np.bincount((keys >> np.uint64(52)).astype(np.int64)).argmax())
    absent = 5  # D around 1e-307: no pair has this exponent
    assert not ((keys >> np.uint64(52)) == np.uint64(absent)).any()
    passes = [  # (prefixes, prefix bits, digit shift, digit width)
        ([0], [0], 52, 11),  # pass 1: the exponents of all pairs
        ([expo, absent, expo + 1], [11, 11, 11], 41, 11),  # pass 2, one prefix matching nothing
        ([expo, (expo << 11) | 1000, 0], [11, 22, 0], 30, 11),  # groups of unequal prefix length
        ([expo] * 8, [11] * 8, 0, 8),  # eight groups (the largest LDS plan), the last digit
    ]
    for prefixes, pbits, shift, width in passes:
        ng = len(prefixes)
        hist = torch.full((ng * bins + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        pre, pb = np.array(prefixes, dtype=np.uint64), np.array(pbits, dtype=np.int32)
        L.call("tw_dist_hist", xd, n, zd, m, 8, pid, host_ptr(pre), host_ptr(pb), ng, shift,
               width, hist, L.stream_handle())
        got = hist.cpu().numpy().view(np.uint64)
        assert (got[ng * bins:] == SENTINEL).all()  # nothing behind the histogram
        want = o_hist(keys, prefixes, pbits, shift, width, bins)
        assert np.array_equal(got[:ng * bins].reshape(ng, bins), want), (prefixes, shift)
        if absent in prefixes:
            assert not want[prefixes.index(absent)].any()
        # the same histogram from a key buffer
        kd = L.to_device(keys.view(np.int64))
        hist2 = torch.full((ng * bins + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        L.call("tw_keys_hist", kd, len(keys), host_ptr(pre), host_ptr(pb), ng, shift, width,
               hist2, L.stream_handle())
        assert np.array_equal(hist2.cpu().numpy().view(np.uint64), got)
    assert want.sum() == 8 * (keys >> np.uint64(52) == np.uint64(expo)).sum()


def test_raw_key_buffer_histogram_spans_workgroups(tw, gpu):
    """tw_keys_hist on a buffer of several workgroups with a ragged end."""
    import torch
    L = tw._lib
    rng = np.random.RandomState(3)
    keys = (np.abs(rng.normal(size=40_001)) * 10.0 ** rng.randint(-2, 3, 40_001)).view(np.uint64)
    kd = L.to_device(keys.view(np.int64))
    pre, pb = np.array([0], dtype=np.uint64), np.array([0], dtype=np.int32)
    hist = torch.zeros((2048,), dtype=torch.int64, device=gpu)
    L.call("tw_keys_hist", kd, len(keys), host_ptr(pre), host_ptr(pb), 1, 52, 11, hist,
           L.stream_handle())
    assert np.array_equal(hist.cpu().numpy().view(np.uint64),
                          o_hist(keys, [0], [0], 52, 11, 2048)[0])


@pytest.mark.parametrize("pairs,n,m", [("within", 129, 0), ("cross", 130, 5)])
def test_raw_gather_and_its_overflow(tw, gpu, pairs, n, m):
    import torch
    L, keys, xd, zd, pid = raw_setup(tw, pairs, n, m, 8)
    M = len(keys)
    expo = int(np.bincount((keys >> np.uint64(52)).astype(np.int64)).argmax())
    under = np.sort(keys[(keys >> np.uint64(52)) == np.uint64(expo)])

    def gather(prefixes, pbits, cap):
        buf = torch.full((cap + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        count = torch.full((2 + GUARD,), SENTINEL, dtype=torch.int64, device=gpu)
        pre, pb = np.array(prefixes, dtype=np.uint64), np.array(pbits, dtype=np.int32)
        L.call("tw_dist_gather", xd, n, zd, m, 8, pid, host_ptr(pre), host_ptr(pb), len(pre),
               buf, cap, count, L.stream_handle())
        b, c = buf.cpu().numpy().view(np.uint64), count.cpu().numpy().view(np.uint64)
        assert (b[cap:] == SENTINEL).all() and (c[2:] == SENTINEL).all()  # the guard regions
        return b[:cap], int(c[0]), int(c[1])

    b, cnt, over = gather([0], [0], M)  # everything fits: the keys, in some order
    assert (cnt, over) == (M, 0) and np.array_equal(np.sort(b), np.sort(keys))
    b, cnt, over = gather([expo, 5], [11, 11], len(under) + 7)  # one exponent; one empty group
    assert (cnt, over) == (len(under), 0) and np.array_equal(np.sort(b[:cnt]), under)
    assert (b[cnt:] == SENTINEL).all()
    b, cnt, over = gather([expo, expo], [11, 11], len(under))  # a key of two groups: once
    assert (cnt, over) == (len(under), 0) and np.array_equal(np.sort(b), under)
    cap = len(under) // 3  # too small: the count is the true one, the flag is set, and what was
    b, cnt, over = gather([expo], [11], cap)  # written is cap keys of the candidates
    assert (cnt, over) == (len(under), 1)
    vals, num = np.unique(b, return_counts=True)
    uvals, unum = np.unique(under, return_counts=True)
    assert np.isin(vals, uvals).all() and (num <= unum[np.searchsorted(uvals, vals)]).all()
    b, cnt, over = gather([0], [0], 0)  # capacity 0: only the count
    assert (cnt, over) == (M, 1)


# --------------------------------------------------------------- sigma="median" in the modules
@pytest.fixture(scope="module")
def sample():
    rng = np.random.RandomState(12)
    X, Z = rng.normal(size=(150, 5)), rng.normal(0.3, 1.2, size=(131, 5))
    Y = X[:, :2] ** 2 + 0.5 * rng.normal(size=(150, 2))
    return X, Z, Y


def same_bits(a, b):
    return np.array_equal(u64(np.asarray(a, dtype=np.float64).reshape(-1)),
                          u64(np.asarray(b, dtype=np.float64).reshape(-1)))


def test_mmd_median_is_the_pooled_median(bw, sample):
    import tuplewise.mmd as mm
    X, Z, _ = sample
    s = bw.median_distance(X, Z, "pooled")
    assert u64(s).item() == u64(np.median(np.sqrt(o_dist(X, Z, "pooled")))).item()
    assert same_bits(mm.Un(X, Z, sigma="median"), mm.Un(X, Z, sigma=s))
    assert same_bits(mm.components(X, Z, sigma="median"), mm.components(X, Z, sigma=s))
    res = []
    for sg in ("median", s):
        np.random.seed(8)
        r = mm.permutation_test(X, Z, 30, sigma=sg)
        res.append((r, np.random.get_state()))
    (a, sa), (b, sb) = res
    assert same_bits(a.statistic, b.statistic) and same_bits(a.null, b.null)
    assert a.pvalue == b.pvalue and same_state(sa, sb)
    for fn in (lambda x, z, sg: mm.UnNT(x, z, 4, 3, sigma=sg),
               lambda x, z, sg: mm.UnNBT(x, z, 4, 50, 2, sigma=sg),
               lambda x, z, sg: mm.UB(x, z, 200, sigma=sg)):
        out = []
        for sg in ("median", s):
            np.random.seed(9)
            x, z = X.copy(), Z.copy()
            out.append((fn(x, z, sg), x, z, np.random.get_state()))
        assert same_bits(out[0][0], out[1][0]) and same_state(out[0][3], out[1][3])
        assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_hsic_median_is_each_sides_median(bw, sample):
    import tuplewise.hsic as hh
    import tuplewise.hsic_perm as hp
    X, _, Y = sample
    sx, sy = bw.median_distance(X), bw.median_distance(Y)
    assert u64(sy).item() == u64(np.median(np.sqrt(o_dist(Y, None, "within")))).item()
    assert same_bits(hh.Un(X, Y, sigma="median"), hh.Un(X, Y, sigma=(sx, sy)))
    assert same_bits(hh.Un(X, Y, sigma=("median", 2.0)), hh.Un(X, Y, sigma=(sx, 2.0)))
    assert same_bits(hh.Un(X, Y, sigma=(0.7, "median")), hh.Un(X, Y, sigma=(0.7, sy)))
    assert same_bits(hh.correlation(X, Y, sigma="median"), hh.correlation(X, Y, sigma=(sx, sy)))
    res = []
    for sg in ("median", (sx, sy)):
        np.random.seed(8)
        r = hp.permutation_test(X, Y, 30, sigma=sg)
        res.append((r, np.random.get_state()))
    (a, sa), (b, sb) = res
    assert same_bits(a.statistic, b.statistic) and same_bits(a.null, b.null)
    assert a.pvalue == b.pvalue and same_state(sa, sb)
    out = []
    for sg in ("median", (sx, sy)):
        np.random.seed(9)
        x, y = X.copy(), Y.copy()
        out.append((hh.UnNT(x, y, 4, 3, sigma=sg), x, y, np.random.get_state()))
    assert same_bits(out[0][0], out[1][0]) and same_state(out[0][3], out[1][3])
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])


def test_a_median_of_zero_is_refused(bw):
    import tuplewise.hsic as hh
    import tuplewise.mmd as mm
    X = rows("equal", 40, 3, 1)
    Y = rows("gauss", 40, 2, 2)
    assert bw.median_distance(X) == 0.0
    state = np.random.get_state()
    with pytest.raises(ValueError, match="median distance of the pooled sample is 0"):
        mm.UnNT(X, X.copy(), 2, 2, sigma="median")
    with pytest.raises(ValueError, match="median distance of X is 0"):
        hh.Un(X, Y, sigma="median")
    with pytest.raises(ValueError, match="median distance of Y is 0"):
        hh.UnN(Y, X, 2, sigma=(1.0, "median"))
    assert same_state(state, np.random.get_state())
