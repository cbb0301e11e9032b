"""tuplewise.hsic_perm (the permutation test of tuplewise.hsic's statistic) on the device (csrc/hsic_perm.hip): both sums of every
column exactly on data whose sums are integers (|a - b| of distinct integers below 2^10 at d = 1:
every K, L, product, row sum and total is an integer below 2^53 in any order of summation),
across tile edges, column chunks, both moved sides and every launch plan; against the NumPy oracle
of tests/test_hsic_perm_cpu.py on float data; bit for bit across column positions, launches and
runs; permutation_test against the oracle's test (values, p-value, RNG state, the caller's
arrays); NaN and D = +inf.

Tolerances: the distances and c * D are bit-identical on both sides, exp is within an ulp or so of
NumPy's, sqrt is exact and every term is non-negative, so S_p and Rab_p agree with the oracle to
the package's rtol 1e-12 for float sums whatever the order of summation (tests/test_gpu_hsic.py).
The statistic cancels, so values are compared at that file's propagated atol,
1e-12 * (|2 S_p| + |R_K R_L| / ((n - 1)(n - 2)) + |2 Rab_p| / (n - 2)) / (n (n - 3)), from the
oracle."""
import functools

import numpy as np
import pytest

from test_gpu_hsic import GUARD, SENT, bits, coef, raw_sums
from test_hsic_cpu import KERNELS, paired, sig
from test_hsic_perm_cpu import inverse, o_perm_sums, o_perm_test, o_perm_values, some_perms
from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# n as a function of the tile edge T
EXACT_N = {"4": lambda T: 4, "5": lambda T: 5, "T-1": lambda T: T - 1, "T": lambda T: T,
           "T+1": lambda T: T + 1, "2T+3": lambda T: 2 * T + 3, "4T+5": lambda T: 4 * T + 5}
FLOAT_N = {"5": lambda T: 5, "T+1": lambda T: T + 1, "2T+3": lambda T: 2 * T + 3}
FLOAT_D = [(1, 1), (2, 3), (8, 8), (17, 5), (5, 17), (64, 64), (64, 2), (2, 64)]
# wgs -> (tile pairs per workgroup, workgroups, tile pairs of the last one) at n = 4 T + 5
PLANS = {0: (1, 15, 1), 1: (15, 1, 15), 2: (8, 2, 7), 4: (4, 4, 3), 15: (1, 15, 1)}


@pytest.fixture(scope="module")
def hs(gpu):
    import tuplewise.hsic as h
    return h


@pytest.fixture(scope="module")
def hp(gpu):
    import tuplewise.hsic_perm as h
    return h


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_hsic_tile())


@pytest.fixture(scope="module")
def cols(tw, gpu):
    return int(tw._lib.lib().tw_hsic_perm_cols())


def col_counts(C):
    return sorted({c for c in (1, 2, C - 1, C, C + 1, 2 * C + 1) if c >= 1})


def raw_perm(tw, X, Y, perms, kernel, wgs=0, move=None, coefs=None):
    """tw_hsic_sums for the row sums, then tw_hsic_perm_sums called directly: the (P, 2) sums,
    read back from sentinel-filled d_out and d_work, and the eight sums of the unpermuted sample.
    move: "y" (rows of perms), "x" (their inverses, Y held), None: the host's rule."""
    import torch
    L = tw._lib
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    n, P = len(X), len(perms)
    kid, cx, cy = coefs if coefs is not None else coef(tw, kernel, X.shape[1], Y.shape[1])
    comp, rows = raw_sums(tw, X, Y, [0, n], kernel, coefs=(kid, cx, cy))
    if move is None:
        move = "y" if Y.shape[1] <= X.shape[1] else "x"
    if move == "y":
        held, moved, idx, rh, rm, ch, cm = X, Y, perms, rows[:, 0], rows[:, 1], cx, cy
    else:
        held, moved, idx, rh, rm, ch, cm = Y, X, inverse(perms), rows[:, 1], rows[:, 0], cy, cx
    hd, md, rhd, rmd = (L.to_device(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))
                        for a in (held, moved, rh, rm))
    idd = L.to_device(np.ascontiguousarray(idx, dtype=np.int32).reshape(-1))
    nwork = int(L.lib().tw_hsic_perm_work_bytes(n, P, wgs)) // 8
    assert nwork > 0
    work = torch.full((nwork + GUARD,), SENT, dtype=torch.float64, device=hd.device)
    out = torch.full((2 * P + GUARD,), SENT, dtype=torch.float64, device=hd.device)
    L.call("tw_hsic_perm_sums", hd, held.shape[1], md, moved.shape[1], n, idd, P, rhd, rmd, kid,
           ch, cm, wgs, work, out, L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(SENT)) and np.all(bits(out[2 * P:]) == bits(SENT))
    assert not np.any(bits(work[:nwork]) == bits(SENT)), "a slot of d_work was not written"
    return out[:2 * P].reshape(P, 2), comp[0]


def close(got, want, what=None):
    """rtol 1e-12, NaN exactly where the oracle has NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "got", got.reshape(-1).tolist()[:6], "want", want.reshape(-1).tolist()[:6])
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), (what, got, want)


# ------------------------------------------------------------------------------ exact sums
@functools.lru_cache(maxsize=None)
def int_case(n, P):
    """n distinct integers below 2^10 on each side, P index rows (identity, reversal, rotation by
    one, seeded random ones) and the integer sums of every row (computed once, shared, never
    modified): launches of fewer columns use the first rows."""
    rng = np.random.RandomState(n)
    x, y = rng.choice(2 ** 10, size=n, replace=False), rng.choice(2 ** 10, size=n, replace=False)
    perms = some_perms(n, P, n + 1)
    K, L = np.abs(x[:, None] - x[None, :]), np.abs(y[:, None] - y[None, :])
    k, l = K.sum(axis=1), L.sum(axis=1)  # noqa: E741
    iu = np.triu_indices(n, 1)
    want = np.array([[(K[iu] * L[pi][:, pi][iu]).sum(), (k * l[pi]).sum()] for pi in perms],
                    dtype=np.int64)
    assert 0 <= want.min() and want.max() < 2 ** 53 and (k.max() * l.max()) * n < 2 ** 53
    return x.astype(np.float64).reshape(n, 1), y.astype(np.float64).reshape(n, 1), perms, want


def exact(got, want, what):
    assert np.array_equal(got, want.astype(np.float64)), (what, got[:4], want[:4])
    assert np.array_equal(got.astype(np.int64), want), what


@pytest.mark.parametrize("shape", list(EXACT_N))
def test_integer_sums_are_exact(tw, tile, cols, shape):
    n = EXACT_N[shape](tile)
    X, Y, perms, want = int_case(n, 2 * cols + 1)
    for P in col_counts(cols):
        got, comp = raw_perm(tw, X, Y, perms[:P], "distance")
        exact(got, want[:P], (shape, P))
        # column 0 is the identity: tw_hsic_sums' own S_KL and R_KL
        assert comp[0] == want[0, 0] and comp[5] == want[0, 1]
    got, _ = raw_perm(tw, X, Y, perms[:cols + 1], "distance", move="x")
    exact(got, want[:cols + 1], (shape, "moved x"))


@pytest.mark.parametrize("wgs", list(PLANS))
def test_integer_sums_are_exact_in_every_plan(tw, tile, cols, wgs):
    """n = 4 T + 5: 15 tile pairs at 15, 8, 4 and 1 per workgroup and the automatic plan, so the
    item loop's later iterations, the running slots carried across items and a short last
    workgroup.  The plan is derived from the library first, so a change of it fails here."""
    n = 4 * tile + 5
    tiles = -(-n // tile)
    items = tiles * (tiles + 1) // 2
    wb = int(tw._lib.lib().tw_hsic_perm_work_bytes(n, 1, wgs))
    assert wb % (8 * cols) == 0
    got_wgs = wb // (8 * cols)
    ipw = -(-items // got_wgs)
    last = items - (got_wgs - 1) * ipw
    print("wgs", wgs, "tiles", tiles, "items", items, "ipw", ipw, "workgroups", got_wgs, "last", last)
    assert (tiles, items) == (5, 15) and (ipw, got_wgs, last) == PLANS[wgs]
    assert -(-items // ipw) == got_wgs and (wgs == 0 or got_wgs <= wgs)
    X, Y, perms, want = int_case(n, 2 * cols + 1)
    for P in (1, cols + 1):
        got, _ = raw_perm(tw, X, Y, perms[:P], "distance", wgs=wgs)
        exact(got, want[:P], (wgs, P))
    got, _ = raw_perm(tw, X, Y, perms[:2], "distance", wgs=wgs, move="x")
    exact(got, want[:2], (wgs, "moved x"))


# ------------------------------------------------------------------------------ float sums
@functools.lru_cache(maxsize=None)
def float_case(dx, dy, n, kernel, P):
    """One data set, P index rows and the oracle's (P, 2) sums (computed once, shared, never
    modified)."""
    X, Y = paired(n, dx, dy, 1000 * dx + 10 * dy + n)
    perms = some_perms(n, P, n + dx)
    s = sig(kernel, dx, dy)
    return X, Y, perms, o_perm_sums(X, Y, perms, kernel, s)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", list(FLOAT_N))
@pytest.mark.parametrize("dx,dy", FLOAT_D)
def test_float_sums(tw, hp, tile, cols, dx, dy, shape, kernel):
    n = FLOAT_N[shape](tile)
    X, Y, perms, want = float_case(dx, dy, n, kernel, cols + 1)
    for P in (1, cols + 1):
        got, comp = raw_perm(tw, X, Y, perms[:P], kernel)
        close(got, want[:P], (dx, dy, n, P))
        close(got[0], [comp[0], comp[5]], "column 0 against tw_hsic_sums")
    # the public call is the same launch under the host's rule for the moved side
    pub = hp.permutation_sums(X, Y, perms, kernel, sig(kernel, dx, dy))
    assert pub.shape == (cols + 1, 2) and pub.dtype == np.float64
    assert np.array_equal(bits(pub), bits(got))
    # and the other moved side gives the same sums
    other, _ = raw_perm(tw, X, Y, perms[:2], kernel, move="x" if dy <= dx else "y")
    close(other, want[:2], (dx, dy, n, "the other side moved"))


# ------------------------------------------------------------- bit for bit across positions
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dx,dy", [(3, 3), (2, 9)])
def test_a_column_depends_on_its_own_index_row_only(tw, tile, cols, dx, dy, kernel):
    n, C = 2 * tile + 3, cols
    X, Y = paired(n, dx, dy, 41)
    rng = np.random.RandomState(5)
    star = rng.permutation(n)
    seen = []
    for P in (1, C + 1, 2 * C + 1):
        for pos in sorted({0, 1, C - 1, C, 2 * C}):
            if not 0 <= pos < P:
                continue
            perms = np.stack([rng.permutation(n) for _ in range(P)])
            perms[pos] = star
            got, _ = raw_perm(tw, X, Y, perms, kernel)
            again, _ = raw_perm(tw, X, Y, perms, kernel)
            assert np.array_equal(bits(again), bits(got)), (P, pos)  # the same launch twice
            seen.append(bits(got[pos]))
    assert len(seen) >= 3 and all(np.array_equal(s, seen[0]) for s in seen), seen
    # a permutation equal to the identity ties with column 0
    perms = some_perms(n, C + 2, 3)
    perms[C + 1] = perms[0]
    got, _ = raw_perm(tw, X, Y, perms, kernel)
    assert np.array_equal(bits(got[C + 1]), bits(got[0]))


@pytest.mark.parametrize("dx,dy", [(3, 2), (2, 3)])
def test_a_constant_moved_side_gives_every_column_the_same_bits(tw, tile, cols, dx, dy):
    """The moved side's rows all equal under the Gaussian kernel: M = exp(0) = 1 exactly, so every
    column is the same sum of H in the same order."""
    n = 2 * tile + 3
    X, Y = paired(n, dx, dy, 6)
    if dy <= dx:
        Y = np.repeat(Y[:1], n, axis=0)
    else:
        X = np.repeat(X[:1], n, axis=0)
    perms = some_perms(n, 2 * cols + 1, 9)
    got, comp = raw_perm(tw, X, Y, perms, "gaussian")
    assert np.isfinite(got).all() and got[0, 0] > 0.0
    assert np.array_equal(bits(got), bits(np.tile(got[0], (len(perms), 1)))), got[:4]
    r_held = comp[3] if dy <= dx else comp[4]  # S = sum_{i<j} H_ij, Rab = (n - 1) sum_i h_i
    close(got[0], [r_held / 2.0, (n - 1) * r_held], "S = R_held / 2, Rab = (n - 1) R_held")


# ------------------------------------------------------------------------- permutation_test
# seeds for which the oracle's statistic is further than the atol from every null value
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dx,dy", [(5, 3), (3, 5)])
def test_permutation_test(hs, hp, dx, dy, kernel):
    n, n_perm = 103, 40
    X, Y = paired(n, dx, dy, 21)
    Y = 0.05 * Y + np.random.RandomState(22).normal(size=Y.shape)  # weak: a p-value inside (0, 1)
    X0, Y0 = X.copy(), Y.copy()
    s = sig(kernel, dx, dy)
    np.random.seed(77)
    stat, null, pvalue, perms = o_perm_test(X, Y, n_perm, kernel, s)
    state = np.random.get_state()
    atol = RTOL * o_perm_values(X, Y, perms, kernel, s)[1]
    gap = np.abs(null - stat).min()
    print(kernel, "oracle stat", stat, "pvalue", pvalue, "gap", gap, "atol", atol.max())
    assert gap > 2.0 * atol.max() and 1 / (n_perm + 1) < pvalue < 1.0
    np.random.seed(77)
    got = hp.permutation_test(X, Y, n_perm, kernel, s)
    assert same_state(state, np.random.get_state())
    assert np.array_equal(bits(X), bits(X0)) and np.array_equal(bits(Y), bits(Y0))
    assert isinstance(got, hp.PermutationResult) and isinstance(got.statistic, np.float64)
    assert got.null.shape == (n_perm,) and got.null.dtype == np.float64
    assert abs(got.statistic - stat) <= atol[0]
    assert np.all(np.abs(got.null - null) <= atol[1:])
    assert got.pvalue == pvalue
    assert got.pvalue == (1 + int(np.count_nonzero(got.null >= got.statistic))) / (1 + n_perm)
    # against the complete statistic of the permuted sample
    for p in range(n_perm + 1):
        un = hs.Un(X, Y[perms[p]], kernel, s)
        val = got.statistic if p == 0 else got.null[p - 1]
        assert abs(val - un) <= atol[p], (p, val, un)


@pytest.mark.parametrize("kernel", KERNELS)
def test_permutation_test_separates_dependent_from_independent(hp, kernel):
    """Seeds checked on the CPU oracle: the dependent pair's statistic is above all 99 null values
    by far more than the tolerance, the independent pair's p-value is far above 0.05."""
    n, n_perm = 200, 99
    X, Y = paired(n, 3, 2, 31)  # Y = X A + 0.5 noise
    s = sig(kernel, 3, 2)
    np.random.seed(3)
    dep = hp.permutation_test(X, Y, n_perm, kernel, s)
    assert dep.pvalue == 0.01 and dep.statistic > dep.null.max() > 0.0 > dep.null.min()
    Z = np.random.RandomState(32).normal(size=Y.shape)
    np.random.seed(3)
    ind = hp.permutation_test(X, Z, n_perm, kernel, s)
    print(kernel, "dependent", dep.statistic, dep.null.max(), "independent", ind.statistic, ind.pvalue)
    assert ind.pvalue > 0.05


# ---------------------------------------------------------------------------- NaN and range
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("side", ["x", "y"])
def test_nan_reaches_every_column(tw, hp, tile, cols, side, kernel):
    n = 2 * tile + 3
    for pos in (0, tile + 1):
        X, Y = paired(n, 3, 3, 8)
        (X if side == "x" else Y)[pos, 1] = np.nan
        perms = some_perms(n, cols + 1, pos)
        for move in ("y", "x"):
            got, _ = raw_perm(tw, X, Y, perms, kernel, move=move)
            assert np.isnan(got[:, 0]).all(), (side, pos, move, got[:, 0])
    np.random.seed(2)
    res = hp.permutation_test(X, Y, 9, kernel, sig(kernel, 3, 3))
    assert np.isnan(res.statistic) and np.isnan(res.null).all() and res.pvalue == 1 / 10


@pytest.mark.parametrize("side", ["x", "y"])
def test_gaussian_infinite_distance_is_a_zero_term(tw, tile, cols, side):
    """One row 1e200 away: D = +inf, g = exp(-inf) = 0 exactly; every column finite."""
    n = tile + 1
    X, Y = paired(n, 3, 2, 9)
    X, Y = X.copy(), Y.copy()
    (X if side == "x" else Y)[tile - 1] = 1e200
    perms = some_perms(n, cols + 1, 4)
    s = sig("gaussian", 3, 2)
    want = o_perm_sums(X, Y, perms, "gaussian", s)
    assert np.isfinite(want).all()
    for move in ("y", "x"):
        got, _ = raw_perm(tw, X, Y, perms, "gaussian", move=move)
        assert np.isfinite(got).all()
        close(got, want, (side, move))
