"""tuplewise.bandwidth without a GPU: the host side of the radix select (narrowing ranks to
digits, grouping prefixes, the decision to gather) against np.sort on random uint64 keys with
histograms made by NumPy, every ValueError of the module and of sigma="median" in tuplewise.mmd /
hsic / hsic_perm (raised before any device call, the global RNG untouched), and how "median" is
parsed and resolved once per call.  Everything here is exact: integers and bit patterns."""
import numpy as np
import pytest

from test_triplets_cpu import same_state


@pytest.fixture(scope="module")
def bw(tw):
    import tuplewise.bandwidth as b
    return b


@pytest.fixture(scope="module")
def mods(tw):
    import tuplewise.hsic as hh
    import tuplewise.hsic_perm as hp
    import tuplewise.mmd as mm
    return mm, hh, hp


class NpSource:
    """The select's passes on a NumPy array of keys (bit 63 clear): what the device source does,
    with the calls recorded."""

    def __init__(self, keys, bins_bits):
        self.keys = np.asarray(keys, dtype=np.uint64)
        self.bins = 1 << bins_bits
        self.calls = []  # ("hist" | "buf" | "gather", number of groups, prefix bits)

    @staticmethod
    def _top(keys, bits):
        return keys >> np.uint64(63 - bits)

    def hist(self, groups, bits, shift, width, buffer):
        src = self.keys if buffer is None else buffer
        self.calls.append(("hist" if buffer is None else "buf", len(groups), bits))
        assert len(groups) <= 8 and len(np.unique(groups)) == len(groups)
        out = np.zeros((len(groups), self.bins), dtype=np.uint64)
        top = self._top(src, bits)
        for g, p in enumerate(groups):
            sel = src[top == p]
            digits = (sel >> np.uint64(shift)) & np.uint64((1 << width) - 1)
            out[g, :1 << width] = np.bincount(digits.astype(np.int64), minlength=1 << width)
        return out

    def gather(self, groups, bits, count):
        self.calls.append(("gather", len(groups), bits))
        sel = self.keys[np.isin(self._top(self.keys, bits), groups)]
        assert len(sel) == count  # the host's candidate count is the gather's
        return sel[np.random.RandomState(len(sel)).permutation(len(sel))]  # order is unspecified


def ranks_for(M, seed, extra=20):
    r = [0, M - 1, (M - 1) // 2, M // 2]
    return np.array(r + list(np.random.RandomState(seed).randint(0, M, extra)), dtype=np.int64)


def keys_of(kind, M, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":  # all 63 bits in use
        return (rng.randint(0, 2 ** 31, M).astype(np.uint64) << np.uint64(32)
                | rng.randint(0, 2 ** 32, M, dtype=np.int64).astype(np.uint64))
    if kind == "ties":  # three values
        return np.array([5, 2 ** 62 + 1, 2 ** 40], dtype=np.uint64)[rng.randint(0, 3, M)]
    if kind == "low":  # one long shared prefix: targets split only in the last digits
        return np.uint64(0x3FF0_0000_0000_0000) | rng.randint(0, 4096, M).astype(np.uint64)
    if kind == "doubles":  # what the device sees: patterns of non-negative doubles, +inf and 0
        v = np.abs(rng.normal(size=M)) * 10.0 ** rng.randint(-3, 4, M)
        v[:3], v[3:6] = np.inf, 0.0
        return v.view(np.uint64)
    raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["random", "ties", "low", "doubles"])
@pytest.mark.parametrize("digit_bits", [11, 4, 13])
def test_select_matches_sort_on_every_path(bw, kind, digit_bits):
    M = 5000
    keys = keys_of(kind, M, 7)
    want = np.sort(keys)
    ranks = ranks_for(M, 11)
    passes = -(-63 // digit_bits)
    for cap in (0, bw.GATHER_CAP, M, M // 16, 1):
        src = NpSource(keys, max(digit_bits, 11))
        got = bw._select(ranks, M, src, cap, digit_bits)
        assert got.dtype == np.uint64 and np.array_equal(got, want[ranks]), (kind, cap)
        chunks = -(-len(np.unique(ranks)) // bw.MAX_GROUPS)
        kinds = [c[0] for c in src.calls]
        assert len(kinds) - kinds.count("gather") == chunks * passes  # all 63 bits, every chunk
        if cap == 0:
            assert set(kinds) == {"hist"}
        if cap >= M:  # gathers at once: the rows are never histogrammed
            assert kinds.count("gather") == chunks and "hist" not in kinds


def test_digits_cover_the_63_bits(bw):
    for digit_bits in (11, 12, 13, 4, 1):
        bits, seen = 0, []
        while bits < 63:
            shift, width = bw._digit_at(bits, digit_bits)
            assert 1 <= width <= digit_bits and shift == 63 - bits - width
            seen.append((shift, width))
            bits += width
        assert bits == 63 and seen[-1][0] == 0
    assert bw._digit_at(0) == (52, 11)  # the first digit of a double's pattern: its exponent
    assert bw._digit_at(55) == (0, 8)


def test_targets_share_and_split_groups(bw):
    """Ranks under one prefix ride in one group; they split when their digits differ."""
    keys = keys_of("low", 4000, 3)  # 52 shared bits, then 12 random ones
    src = NpSource(keys, 11)
    ranks = np.array([0, 1000, 2000, 3999], dtype=np.int64)
    got = bw._select(ranks, len(keys), src, 0)
    assert np.array_equal(got, np.sort(keys)[ranks])
    groups = [c[1] for c in src.calls]
    assert groups[:5] == [1, 1, 1, 1, 1]  # exponent and 40 mantissa bits: one prefix
    assert groups[5] > 1  # the last digit: the targets have split
    # equal ranks and ranks of equal keys stay one group to the end
    src = NpSource(keys_of("ties", 999, 1), 11)
    bw._select(np.array([0, 1, 2, 2], dtype=np.int64), 999, src, 0)
    assert {c[1] for c in src.calls} == {1}


def test_narrow_one_pass(bw):
    hist = np.zeros((2, 2048), dtype=np.uint64)
    hist[0, [3, 7, 9]] = [4, 1, 5]
    hist[1, 2047] = 6
    p, r, c = bw._narrow(hist, np.array([0, 0, 0, 1]), np.array([1, 1, 1, 2], dtype=np.uint64),
                         np.array([3, 4, 9, 5]), 11)
    assert list(p) == [(1 << 11) | 3, (1 << 11) | 7, (1 << 11) | 9, (2 << 11) | 2047]
    assert list(r) == [3, 0, 4, 5] and list(c) == [4, 1, 5, 6]
    assert bw._candidates(p, c) == 16 and bw._candidates(p[[0, 0]], c[[0, 0]]) == 4
    with pytest.raises(RuntimeError, match="outside"):
        bw._narrow(hist, np.array([1]), np.array([2], dtype=np.uint64), np.array([6]), 11)
    assert not bw._gather_now(10, 0) and bw._gather_now(10, 10) and not bw._gather_now(11, 10)
    assert not bw._gather_now(0, 10)


@pytest.fixture
def no_device(monkeypatch, tw):
    """Any device or native call fails the test (on a GPU machine too)."""
    def boom(*a, **k):
        raise AssertionError("the device was touched")
    for name in ("device", "call", "to_device", "to_device_many", "empty"):
        monkeypatch.setattr(tw._lib, name, boom)


def raises_clean(fn, match=None):
    state = np.random.get_state()
    with pytest.raises(ValueError, match=match):
        fn()
    assert same_state(state, np.random.get_state())


def test_bandwidth_argument_errors(bw, no_device):
    X, Z = np.arange(12.0).reshape(6, 2), np.arange(8.0).reshape(4, 2) + 0.5
    bad = X.copy()
    bad[2, 1] = np.nan
    inf = Z.copy()
    inf[0, 0] = -np.inf
    for fn in (lambda **k: bw.order_statistics(ranks=[0], **k), bw.median_distance,
               lambda **k: bw.quantile_distances(q=0.5, **k)):
        raises_clean(lambda: fn(X=X, pairs="all"), "pairs")
        raises_clean(lambda: fn(X=X, Z=Z, pairs="within"), "Z must be None")
        raises_clean(lambda: fn(X=X, pairs="cross"), "needs Z")
        raises_clean(lambda: fn(X=X, pairs="pooled"), "needs Z")
        raises_clean(lambda: fn(X=X.astype(np.float32)), "float64")
        raises_clean(lambda: fn(X=np.arange(24.0).reshape(6, 4)[:, ::2]), "C-contiguous")
        raises_clean(lambda: fn(X=np.zeros((2, 2, 2))), "shape")
        raises_clean(lambda: fn(X=np.zeros((3, 65))), "outside")
        raises_clean(lambda: fn(X=X, Z=np.zeros((4, 3)), pairs="cross"), "coordinates")
        raises_clean(lambda: fn(X=X[:1]), "no pair")
        raises_clean(lambda: fn(X=X[:1], Z=Z[:0], pairs="pooled"), "no pair")
        raises_clean(lambda: fn(X=X, Z=Z[:0], pairs="cross"), "no pair")
        raises_clean(lambda: fn(X=bad), "non-finite")
        raises_clean(lambda: fn(X=X, Z=inf, pairs="pooled"), "non-finite")
        raises_clean(lambda: fn(X=X, Z=inf, pairs="cross"), "non-finite")
        raises_clean(lambda: fn(X=X, _gather_cap=-1), "_gather_cap")
    M = 15
    for r in (None, [0.5], [True], [-1], [M], np.array([0, M])):
        raises_clean(lambda: bw.order_statistics(X, ranks=r))
    for q in (None, -0.1, [0.5, 1.5], np.nan, "x"):
        raises_clean(lambda: bw.quantile_distances(X, q=q))
    raises_clean(lambda: bw.quantile_distances(X, q=0.5, method="linear"), "method")
    # a 1-D sample is d = 1; no ranks is no work
    assert bw.order_statistics(np.arange(4.0), ranks=[]).shape == (0,)


def test_median_sigma_argument_errors(mods, no_device):
    mm, hh, hp = mods
    rng = np.random.RandomState(0)
    X, Z, Y = rng.normal(size=(12, 3)), rng.normal(size=(9, 3)), rng.normal(size=(12, 2))
    Xn, Yn = X.copy(), Y.copy()
    Xn[5, 0], Yn[0, 1] = np.nan, np.inf
    labels = np.zeros((1, 21), dtype=bool)
    labels[0, :12] = True
    perms = np.arange(12)[None, :]
    i = np.array([0])
    # "median" with the kernels that take no sigma
    raises_clean(lambda: mm.Un(X, Z, "energy", "median"), "no sigma")
    raises_clean(lambda: mm.permutation_test(X, Z, 5, "energy", "median"), "no sigma")
    raises_clean(lambda: mm.UnNT(X, Z, 2, 2, kernel="energy", sigma="median"), "no sigma")
    raises_clean(lambda: hh.Un(X, Y, "distance", "median"), "no sigma")
    raises_clean(lambda: hh.Un(X, Y, "distance", ("median", 2.0)), "no sigma")
    raises_clean(lambda: hp.permutation_test(X, Y, 5, "distance", "median"), "no sigma")
    # other strings and a bad number beside "median" stay errors
    raises_clean(lambda: mm.Un(X, Z, "gaussian", "wide"), "not a number")
    raises_clean(lambda: mm.Un(X, Z, "gaussian", "Median"), "not a number")
    raises_clean(lambda: hh.Un(X, Y, "gaussian", ("median", -1.0)), "positive")
    raises_clean(lambda: hh.Un(X, Y, "gaussian", ("median", "wide")), "not a number")
    raises_clean(lambda: hh.Un(X, Y, "gaussian", ("median", 1.0, 2.0)), "pair")
    # non-finite rows: a ValueError with "median" (a NaN propagates with a number)
    calls = [
        lambda: mm.components(Xn, Z, sigma="median"), lambda: mm.Un(Xn, Z, sigma="median"),
        lambda: mm.Un(Z, Xn, sigma="median"),
        lambda: mm.UB_indices(Xn, Z, i, i + 1, i, i + 1, sigma="median"),
        lambda: mm.UB(Xn, Z, 5, sigma="median"), lambda: mm.UnN(Xn, Z, 2, sigma="median"),
        lambda: mm.UnNB(Xn, Z, 2, 5, sigma="median"), lambda: mm.UnNT(Xn, Z, 2, 3, sigma="median"),
        lambda: mm.UnNBT(Xn, Z, 2, 5, 3, sigma="median"),
        lambda: mm.permutation_sums(Xn, Z, labels, sigma="median"),
        lambda: mm.permutation_test(Xn, Z, 5, sigma="median"),
        lambda: hh.components(Xn, Y, sigma="median"), lambda: hh.row_sums(X, Yn, sigma="median"),
        lambda: hh.Un(Xn, Y, sigma="median"), lambda: hh.correlation(X, Yn, sigma="median"),
        lambda: hh.Un(Xn, Y, sigma=("median", 2.0)), lambda: hh.Un(X, Yn, sigma=(2.0, "median")),
        lambda: hh.UB_indices(Xn, Y, i, i + 1, i + 2, i + 3, sigma="median"),
        lambda: hh.UB(Xn, Y, 5, sigma="median"), lambda: hh.UnN(Xn, Y, 2, sigma="median"),
        lambda: hh.UnNB(Xn, Y, 2, 5, sigma="median"), lambda: hh.UnNT(Xn, Y, 2, 3, sigma="median"),
        lambda: hh.UnNBT(X, Yn, 2, 5, 3, sigma="median"),
        lambda: hp.permutation_sums(Xn, Y, perms, sigma="median"),
        lambda: hp.permutation_test(X, Yn, 5, sigma="median"),
    ]
    for k, fn in enumerate(calls):
        state = np.random.get_state()
        with pytest.raises(ValueError, match="non-finite"):
            fn()
        assert same_state(state, np.random.get_state()), k
    # the call's other checks come first: nothing is resolved for a call that is refused anyway
    raises_clean(lambda: mm.UnN(X, Z, 7, sigma="median"), "blocks")
    raises_clean(lambda: mm.UnNT(X, Z, 2, 3, "SWOR", sigma="median"), "prop-SWOR")
    raises_clean(lambda: hh.UnN(X, Y, 4, sigma="median"), "blocks")
    raises_clean(lambda: mm.permutation_test(X, Z, 0, sigma="median"), "n_perm")
    raises_clean(lambda: mm.permutation_sums(X, Z, labels[:, :5], sigma="median"), "labels")
    raises_clean(lambda: hp.permutation_sums(X, Y, perms[:, :5], sigma="median"), "perms")
    raises_clean(lambda: mm.UB_indices(X, Z, i, i, i, i + 1, sigma="median"), "i != j")
    assert not hasattr(hh, "permutation_test")


def test_median_is_parsed(mods, tw):
    mm, hh, _ = mods
    L = tw._lib
    assert mm._coef("gaussian", "median") == (L.TW_MMD_GAUSSIAN, None)
    assert mm._coef("gaussian", 2.0) == (L.TW_MMD_GAUSSIAN, -0.125)
    assert hh._coef("gaussian", "median") == (L.TW_HSIC_GAUSSIAN, None, None)
    assert hh._coef("gaussian", ("median", 2.0)) == (L.TW_HSIC_GAUSSIAN, None, -0.125)
    assert hh._coef("gaussian", [2.0, "median"]) == (L.TW_HSIC_GAUSSIAN, -0.125, None)
    assert hh._coef("gaussian", (1.0, 2.0)) == (L.TW_HSIC_GAUSSIAN, -0.5, -0.125)
    assert mm._is_median("median") and not mm._is_median("Median") and not mm._is_median(1.0)
    assert not mm._is_median(np.array(["median"]))


def test_median_is_resolved_once_and_only_where_asked(mods, bw, monkeypatch, no_device):
    """The resolution (stubbed: no device here) is called once per public call, for the sides that
    ask, with the right pair set, before the first draw; the reshuffled estimators do not repeat
    it; and a numeric sigma never reaches it."""
    mm, hh, hp = mods
    seen = []

    def fake(A, B, pairs, what):
        seen.append((A.shape, None if B is None else B.shape, pairs,
                     np.random.get_state()[1].copy()))
        return 3.0 if what != "Y" else 5.0

    monkeypatch.setattr(bw, "_median_sigma", fake)
    monkeypatch.setattr(mm, "_sums_blocks", lambda Xf, Zf, bxo, bzo, kid, c:
                        np.full((len(bxo) - 1, 3), c))
    monkeypatch.setattr(hh, "_sums_blocks", lambda Xf, Yf, off, kid, cx, cy, **k:
                        (np.tile(np.array([cx, cy] * 4), (len(off) - 1, 1)), None))
    monkeypatch.setattr(hh, "_work_bytes", lambda *a, **k: 8)
    rng = np.random.RandomState(1)
    X, Z, Y = rng.normal(size=(40, 3)), rng.normal(size=(30, 3)), rng.normal(size=(40, 2))

    def both(fn, a, b, sig, num):
        seen.clear()
        np.random.seed(4)
        start = np.random.get_state()[1].copy()
        a1, b1 = a.copy(), b.copy()
        got = fn(a1, b1, sig)
        end = np.random.get_state()
        n_seen = list(seen)
        np.random.seed(4)
        a2, b2 = a.copy(), b.copy()
        want = fn(a2, b2, num)
        assert len(seen) == len(n_seen), "a numeric sigma resolves nothing"
        assert got == want and same_state(end, np.random.get_state())
        assert np.array_equal(a1, a2) and np.array_equal(b1, b2)
        for s in n_seen:
            assert np.array_equal(s[3], start), "resolved before the first draw"
        return n_seen

    s = both(lambda a, b, sg: mm.Un(a, b, sigma=sg), X, Z, "median", 3.0)
    assert [(x[0], x[1], x[2]) for x in s] == [((40, 3), (30, 3), "pooled")]
    for fn in (lambda a, b, sg: mm.UnN(a, b, 3, sigma=sg),
               lambda a, b, sg: mm.UnNT(a, b, 3, 4, sigma=sg)):
        assert len(both(fn, X, Z, "median", 3.0)) == 1
    s = both(lambda a, b, sg: hh.Un(a, b, sigma=sg), X, Y, "median", (3.0, 5.0))
    assert [(x[0], x[1], x[2]) for x in s] == [((40, 3), None, "within"), ((40, 2), None, "within")]
    s = both(lambda a, b, sg: hh.Un(a, b, sigma=sg), X, Y, (2.0, "median"), (2.0, 5.0))
    assert [(x[0], x[2]) for x in s] == [((40, 2), "within")]
    for fn in (lambda a, b, sg: hh.UnN(a, b, 3, sigma=sg),
               lambda a, b, sg: hh.UnNT(a, b, 3, 4, sigma=sg)):
        assert len(both(fn, X, Y, ("median", 7.0), (3.0, 7.0))) == 1
        assert len(both(fn, X, Y, "median", (3.0, 5.0))) == 2
