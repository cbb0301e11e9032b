"""tuplewise.hsic on the device against the NumPy oracle of tests/test_hsic_cpu.py: the eight sums
and both row-sum vectors of tw_hsic_sums at rtol 1e-12 (one block, the plan knob, mixed block
sizes in one launch, a partition behind a leading gap, sentinels behind d_out, d_work and d_rows),
the exact properties (run-to-run bits, a block alone and beside others, X against its copy,
duplicated rows, NaN placement), the indexed kernel on hand-made 4-tuples, and the estimators'
values, in-place paired shuffles and RNG consumption.

Tolerances: the distances and c * D are bit-identical on both sides, exp is within an ulp or so of
NumPy's, sqrt is exact and every term is non-negative, so the eight sums and the row sums agree to
the package's rtol 1e-12 for float sums whatever the order of summation (at n <= 4 P + 5 a row
sum's worst-case rounding, n ulps, is below 1e-13).  The statistic cancels, so values are compared
at atol = 1e-12 * (|2 S_KL| + |R_K R_L| / ((n - 1)(n - 2)) + |2 R_KL| / (n - 2)) / (n (n - 3)),
the indexed ones at 1e-12 * (A + B + 2 C) / B_n, both from the oracle; the correlation's tolerance
is propagated from the three statistics' atols."""
import functools
import math

import numpy as np
import pytest

from test_hsic_cpu import (KERNELS, NAMES, o_components, o_correlation, o_draw, o_idx_sums,
                           o_row_sums, o_three, o_UB_indices, o_UB_scale, o_Un, o_Un_scale, o_UN,
                           paired, sig)
from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# (dx, dy, n) with n a function of the tile edge P
SHAPES = {
    "1-1-4": (1, 1, lambda P: 4),
    "2-3-5": (2, 3, lambda P: 5),
    "3-1-65": (3, 1, lambda P: 65),
    "8-8-P-1": (8, 8, lambda P: P - 1),
    "17-2-P": (17, 2, lambda P: P),
    "37-37-P+1": (37, 37, lambda P: P + 1),
    "64-8-2P+3": (64, 8, lambda P: 2 * P + 3),
    "8-64-65": (8, 64, lambda P: 65),
    "64-64-P+1": (64, 64, lambda P: P + 1),
}
GUARD = 64  # sentinel entries behind d_out, d_work and d_rows: nothing may be written there
SENT = -7.0


@pytest.fixture(scope="module")
def hs(gpu):
    import tuplewise.hsic as h
    return h


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_hsic_tile())


def coef(tw, kernel, dx, dy):
    if kernel == "gaussian":
        sx, sy = sig(kernel, dx, dy)
        return tw._lib.TW_HSIC_GAUSSIAN, -1.0 / (2.0 * sx * sx), -1.0 / (2.0 * sy * sy)
    return tw._lib.TW_HSIC_DISTANCE, 0.0, 0.0


@functools.lru_cache(maxsize=None)
def case(dx, dy, n, kind, kernel):
    """One data set and its reference (computed once, shared, never modified): X, Y, the eight
    sums, the row sums k and l."""
    X, Y = paired(n, dx, dy, 1000 * dx + 10 * dy + n, kind)
    s = sig(kernel, dx, dy)
    return X, Y, o_components(X, Y, kernel, s), o_row_sums(X, Y, kernel, s)


def shape_case(shape, P, kind, kernel):
    dx, dy, fn = SHAPES[shape]
    return case(dx, dy, fn(P), kind, kernel)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def raw_sums(tw, X, Y, off, kernel, group=0, coefs=None):
    """tw_hsic_sums called directly on the blocks `off`: the (n_blocks, 8) sums and the (rows, 2)
    row sums, read back from sentinel-filled d_out, d_work and d_rows; rows outside every block
    must still hold the sentinel."""
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    nb = len(off) - 1
    max_n = int(np.diff(off).max())
    kid, cx, cy = coefs if coefs is not None else coef(tw, kernel, X.shape[1], Y.shape[1])
    xd, yd, od = (L.to_device(np.ascontiguousarray(a).reshape(-1)) for a in (X, Y, off))
    nwork = int(L.lib().tw_hsic_work_bytes(nb, max_n, group)) // 8
    assert nwork > 0
    work = torch.full((nwork + GUARD,), SENT, dtype=torch.float64, device=xd.device)
    out = torch.full((8 * nb + GUARD,), SENT, dtype=torch.float64, device=xd.device)
    rows = torch.full((2 * X.shape[0] + GUARD,), SENT, dtype=torch.float64, device=xd.device)
    L.call("tw_hsic_sums", xd, X.shape[1], yd, Y.shape[1], od, nb, max_n, kid, cx, cy, group,
           work, rows, out, L.stream_handle())
    work, out, rows = work.cpu().numpy(), out.cpu().numpy(), rows.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(SENT)) and np.all(bits(out[8 * nb:]) == bits(SENT))
    assert np.all(bits(rows[2 * X.shape[0]:]) == bits(SENT))
    rows = rows[:2 * X.shape[0]].reshape(-1, 2)
    inside = np.zeros(X.shape[0], dtype=bool)
    for a, b in zip(off, off[1:]):
        inside[a:b] = True
    assert np.all(bits(rows[~inside]) == bits(SENT)), "a row outside every block was written"
    return out[:8 * nb].reshape(nb, 8), rows


def close(got, want, what=None):
    """rtol 1e-12, NaN exactly where the oracle has NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "got", got.tolist()[:8], "want", want.tolist()[:8])
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), (what, got, want)


def close_all(got, rows, want, want_rows, what):
    close(got, want, what)
    close(rows[:, 0], want_rows[0], (what, "k"))
    close(rows[:, 1], want_rows[1], (what, "l"))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_sums_one_block(tw, hs, tile, shape, kernel):
    X, Y, want, want_rows = shape_case(shape, tile, "gauss", kernel)
    n = X.shape[0]
    got, rows = raw_sums(tw, X, Y, [0, n], kernel)
    close_all(got[0], rows, want, want_rows, shape)
    again, rows2 = raw_sums(tw, X, Y, [0, n], kernel)
    assert np.array_equal(bits(again), bits(got)) and np.array_equal(bits(rows2), bits(rows))
    s = sig(kernel, X.shape[1], Y.shape[1])
    pub = hs.components(X, Y, kernel, s)
    assert pub._fields == NAMES and all(isinstance(v, np.float64) for v in pub)
    assert np.array_equal(bits(pub), bits(got))
    k, l = hs.row_sums(X, Y, kernel, s)  # noqa: E741
    assert k.shape == l.shape == (n,) and k.dtype == l.dtype == np.float64
    assert np.array_equal(bits(k), bits(rows[:, 0])) and np.array_equal(bits(l), bits(rows[:, 1]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("mult", [2, 4])
def test_plan_knob(tw, tile, mult, kernel):
    n = mult * tile + mult + 1  # 2 P + 3, 4 P + 5
    X, Y, want, want_rows = case(8, 8, n, "gauss", kernel)
    wb = tw._lib.lib().tw_hsic_work_bytes
    by_group = {}
    for g in (0, 1, 2, 3):
        got, rows = raw_sums(tw, X, Y, [0, n], kernel, group=g)
        close_all(got[0], rows, want, want_rows, (n, g))
        by_group[g] = np.concatenate([bits(got), bits(rows)])
    # group = 0 is one of the explicit plans: the one with its d_work, bit for bit
    same = [g for g in range(1, 9) if wb(1, n, g) == wb(1, n, 0)]
    assert same and all(g in by_group for g in same), same
    assert any(np.array_equal(by_group[0], by_group[g]) for g in same)


def test_plan_knob_largest_groups(tw, tile):
    """Groups past the block's tiles (one super-tile holds everything) and the largest one."""
    n = 4 * tile + 5
    X, Y, want, want_rows = case(8, 8, n, "gauss", "gaussian")
    for g in (4, 5, 8):
        got, rows = raw_sums(tw, X, Y, [0, n], "gaussian", group=g)
        close_all(got[0], rows, want, want_rows, (n, g))


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_blocks_in_one_launch(tw, tile, kernel):
    P, dx, dy = tile, 5, 3
    sizes = [4, P + 1, 65, 2 * P + 3]
    s = sig(kernel, dx, dy)
    want = first = None
    for gap in (0, 7):  # the partition at 0, then behind a leading gap of rows
        off = gap + np.concatenate([[0], np.cumsum(sizes)])
        X, Y = paired(int(off[-1]) - gap, dx, dy, 77)
        if want is None:
            want = [(o_components(X[a:b], Y[a:b], kernel, s), o_row_sums(X[a:b], Y[a:b], kernel, s))
                    for a, b in zip(off, off[1:])]
        # rows no block owns: far away, so a block-relative offset shows in the sums
        X = np.concatenate([np.full((gap, dx), 1e3), X])
        Y = np.concatenate([np.full((gap, dy), -1e3), Y])
        got, rows = raw_sums(tw, X, Y, off, kernel)
        for b, (a, e) in enumerate(zip(off, off[1:])):
            close_all(got[b], rows[a:e], want[b][0], want[b][1], (gap, b))
        again, rows2 = raw_sums(tw, X, Y, off, kernel)
        assert np.array_equal(bits(again), bits(got)) and np.array_equal(bits(rows2), bits(rows))
        for b, (a, e) in enumerate(zip(off, off[1:])):  # a block alone: the bits it has beside others
            alone, arows = raw_sums(tw, X, Y, off[b:b + 2], kernel)
            assert np.array_equal(bits(alone[0]), bits(got[b])), (gap, b)
            assert np.array_equal(bits(arows[a:e]), bits(rows[a:e])), (gap, b)
        if gap == 0:
            first = got, rows
        else:  # and the same bits wherever the partition starts
            assert np.array_equal(bits(got), bits(first[0]))
            assert np.array_equal(bits(rows[gap:]), bits(first[1]))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", ["2-3-5", "3-1-65", "37-37-P+1", "64-8-2P+3"])
def test_same_sample_on_both_sides(tw, tile, shape, kernel):
    """Y = X.copy() with equal coefficients: K and L are the same bits, so are their sums."""
    X = shape_case(shape, tile, "gauss", kernel)[0]
    n, d = X.shape
    kid, cx, _ = coef(tw, kernel, d, d)
    got, rows = raw_sums(tw, X, X.copy(), [0, n], kernel, coefs=(kid, cx, cx))
    b = bits(got[0])
    assert b[0] == b[1] == b[2] and b[3] == b[4] and b[5] == b[6] == b[7], got
    assert np.array_equal(bits(rows[:, 0]), bits(rows[:, 1]))
    s = math.sqrt(d) if kernel == "gaussian" else None
    close(got[0], o_components(X, X, kernel, s), shape)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dx,dy", [(1, 1), (8, 17), (64, 3)])
def test_duplicated_rows_are_exact(tw, dx, dy, kernel):
    """Five equal rows: D = 0 exactly, so every K and L is exactly 1 (Gaussian) or 0 (distance)
    and the sums are small integers."""
    rng = np.random.RandomState(dx)
    X, Y = np.repeat(rng.normal(size=(1, dx)), 5, axis=0), np.repeat(rng.normal(size=(1, dy)), 5, axis=0)
    got, rows = raw_sums(tw, X, Y, [0, 5], kernel)
    if kernel == "gaussian":
        want, row = [10.0, 10.0, 10.0, 20.0, 20.0, 80.0, 80.0, 80.0], 4.0
    else:
        want, row = [0.0] * 8, 0.0
    assert np.array_equal(bits(got[0]), bits(want)), got
    assert np.array_equal(bits(rows), bits(np.full((5, 2), row)))
    assert tuple(want) == o_components(X, Y, kernel, sig(kernel, dx, dy))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", ["2-3-5", "37-37-P+1", "64-8-2P+3"])
def test_ties_and_nan(tw, tile, shape, kernel):
    X, Y, want, want_rows = shape_case(shape, tile, "ties", kernel)
    got, rows = raw_sums(tw, X, Y, [0, X.shape[0]], kernel)
    close_all(got[0], rows, want, want_rows, (shape, "ties"))
    # a NaN in X: every K-derived output is NaN, the L-only ones are finite and the oracle's
    X, Y, want, want_rows = shape_case(shape, tile, "nan", kernel)
    assert [np.isnan(v) for v in want] == [True, True, False, True, False, True, True, False]
    assert np.isnan(want_rows[0]).all() and not np.isnan(want_rows[1]).any()
    got, rows = raw_sums(tw, X, Y, [0, X.shape[0]], kernel)
    close_all(got[0], rows, want, want_rows, (shape, "nan"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_nan_in_another_block_changes_nothing(tw, tile, kernel):
    P, dx, dy = tile, 8, 3
    off = np.array([0, P + 1, 2 * P + 6, 2 * P + 10])
    X, Y = paired(int(off[-1]), dx, dy, 5)
    clean, crows = raw_sums(tw, X, Y, off, kernel)
    Xn, Yn = X.copy(), Y.copy()
    Xn[off[1] + 3, 2] = np.nan  # the middle block: a NaN on each side
    Yn[off[2] - 1, 0] = np.nan
    got, rows = raw_sums(tw, Xn, Yn, off, kernel)
    for b in (0, 2):
        assert np.array_equal(bits(got[b]), bits(clean[b])), b
        assert np.array_equal(bits(rows[off[b]:off[b + 1]]), bits(crows[off[b]:off[b + 1]])), b
    assert np.isnan(got[1]).all() and np.isnan(rows[off[1]:off[2]]).all()


def raw_idx(tw, X, Y, i, j, q, r, off, kernel):
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns = len(off) - 1
    max_q = int(np.diff(off).max())
    kid, cx, cy = coef(tw, kernel, X.shape[1], Y.shape[1])
    xd, yd = L.to_device(X.reshape(-1)), L.to_device(Y.reshape(-1))
    id_, jd, qd, rd = (L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, q, r))
    od = L.to_device(off)
    nwork = int(L.lib().tw_hsic_idx_work_bytes(ns, max_q)) // 8
    work = torch.full((nwork + GUARD,), SENT, dtype=torch.float64, device=xd.device)
    out = torch.full((3 * ns + GUARD,), SENT, dtype=torch.float64, device=xd.device)
    L.call("tw_hsic_idx32", xd, X.shape[1], yd, Y.shape[1], id_, jd, qd, rd, od, ns, max_q, kid,
           cx, cy, work, out, L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(SENT)) and np.all(bits(out[3 * ns:]) == bits(SENT))
    return out[:3 * ns].reshape(ns, 3)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind,dx,dy", [("ties", 2, 1), ("gauss", 37, 8), ("nan", 8, 64)])
def test_indexed(tw, hs, kind, dx, dy, kernel):
    n = 40
    X, Y = paired(n, dx, dy, 1, kind)
    s = sig(kernel, dx, dy)
    # hand-made: neighbours, repeated tuples, the last rows, the tied rows 0, 20, 39, negative
    # indices as NumPy reads them
    i = np.array([0, 1, 5, 5, 5, 39, 38, 13, 0, -1, 0])
    j = np.array([1, 0, 4, 6, 6, 38, 39, 12, 20, 0, -1])
    q = np.array([2, 3, 3, 7, 7, 0, 1, 11, 39, -2, -40 + 5])
    r = np.array([3, 2, 6, 4, 4, 1, 0, 14, 1, 1, 2])
    if kind != "nan":
        got = hs.UB_indices(X, Y, i, j, q, r, kernel, s)
        want = o_UB_indices(X, Y, i, j, q, r, kernel, s)
        tol = RTOL * o_UB_scale(X, Y, i, j, q, r, kernel, s)
        print(kind, kernel, got, want, tol)
        assert isinstance(got, np.float64) and abs(got - want) <= tol
        col = [a.reshape(-1, 1) for a in (i, j, q, r)]
        assert hs.UB_indices(X, Y, *col, kernel, s) == got
    none = np.zeros(0, dtype=np.int64)
    assert np.isnan(hs.UB_indices(X, Y, none, none, none, none, kernel, s))
    # raw, shards of mixed sizes: none, one, a few, one past a wave's tuples, one past two
    # workgroups' worth (4 tuples per lane, 256 lanes)
    sizes = [0, 1, 3, 257, 2049, 0, 11]
    off = np.concatenate([[0], np.cumsum(sizes)])
    T = int(off[-1])
    np.random.seed(4)
    ri, rj, rq, rr = o_draw(n, T)
    ri[-11:], rj[-11:], rq[-11:], rr[-11:] = i % n, j % n, q % n, r % n
    got = raw_idx(tw, X, Y, ri, rj, rq, rr, off, kernel)
    for sh, (a, b) in enumerate(zip(off, off[1:])):
        if a == b:
            assert np.array_equal(bits(got[sh]), bits(np.zeros(3))), sh  # an empty shard: zeros
        else:
            close(got[sh], o_idx_sums(X, Y, ri[a:b], rj[a:b], rq[a:b], rr[a:b], kernel, s), sh)
    assert np.array_equal(bits(raw_idx(tw, X, Y, ri, rj, rq, rr, off, kernel)), bits(got))
    for sh in (1, 3, 4):  # a shard's sums are the same bits alone as beside others
        a, b = off[sh], off[sh + 1]
        alone = raw_idx(tw, X, Y, ri[a:b], rj[a:b], rq[a:b], rr[a:b], [0, b - a], kernel)
        assert np.array_equal(bits(alone[0]), bits(got[sh])), sh


# ---- the estimators: the oracle's value with the magnitude its tolerance is taken from
def ref_Un(X, Y, kernel, s):
    return o_Un(X, Y, kernel, s), o_Un_scale(X, Y, kernel, s)


def ref_UB(X, Y, B, kernel, s):
    t = o_draw(X.shape[0], B)
    return o_UB_indices(X, Y, *t, kernel, s), o_UB_scale(X, Y, *t, kernel, s)


def ref_blocks(X, Y, N, T, block):
    """T rounds of o_UN over `block` (value, scale): the value and the mean scale."""
    scales = []

    def f(x, y):
        v, sc = block(x, y)
        scales.append(sc)
        return v

    value = np.mean([o_UN(X, Y, N, f) for _ in range(T)])
    return value, float(np.mean(scales))


@pytest.mark.parametrize("kernel", KERNELS)
def test_estimators(hs, kernel):
    n, dx, dy, N, B, T = 103, 5, 3, 4, 500, 3
    X0, Y0 = paired(n, dx, dy, 21)
    s = sig(kernel, dx, dy)
    kw = dict(kernel=kernel, sigma=s)

    def un(x, y):
        return ref_Un(x, y, kernel, s)

    def ub(b):
        return lambda x, y: ref_UB(x, y, b, kernel, s)

    runs = [("Un", lambda X, Y: hs.Un(X, Y, **kw), un),
            ("UB", lambda X, Y: hs.UB(X, Y, 1000, **kw), ub(1000)),
            ("UnN", lambda X, Y: hs.UnN(X, Y, N, **kw), lambda X, Y: ref_blocks(X, Y, N, 1, un)),
            ("UnNB", lambda X, Y: hs.UnNB(X, Y, N, B, **kw),
             lambda X, Y: ref_blocks(X, Y, N, 1, ub(B))),
            ("UnNT", lambda X, Y: hs.UnNT(X, Y, N, T, **kw),
             lambda X, Y: ref_blocks(X, Y, N, T, un)),
            ("UnNBT", lambda X, Y: hs.UnNBT(X, Y, N, B, T, **kw),
             lambda X, Y: ref_blocks(X, Y, N, T, ub(B))),
            # UN with Un itself (its arguments bound) and with a callable of the caller's own go
            # block by block, the same partition
            ("UN(Un)", lambda X, Y: hs.UN(X, Y, N, functools.partial(hs.Un, **kw)),
             lambda X, Y: ref_blocks(X, Y, N, 1, un)),
            ("UN(callable)", lambda X, Y: hs.UN(X, Y, N, lambda x, y: float(x[0, 0] - y[-1, 1])),
             lambda X, Y: (o_UN(X, Y, N, lambda x, y: float(x[0, 0] - y[-1, 1])), 0.0))]
    for seed, (name, f, o) in enumerate(runs):
        X, Y, Xo, Yo = X0.copy(), Y0.copy(), X0.copy(), Y0.copy()
        np.random.seed(100 + seed)
        got = f(X, Y)
        state = np.random.get_state()
        np.random.seed(100 + seed)
        want, scale = o(Xo, Yo)
        print(name, kernel, got, want, RTOL * scale)
        assert isinstance(got, np.float64) and abs(got - want) <= RTOL * scale, (name, got, want)
        assert np.array_equal(bits(X), bits(Xo)) and np.array_equal(bits(Y), bits(Yo)), name
        assert same_state(state, np.random.get_state()), name
    # no sign flip: both statistics are positive for a dependent pair
    assert hs.Un(X0, Y0, **kw) > 0.0


@pytest.mark.parametrize("kernel", KERNELS)
def test_correlation(hs, kernel):
    X, Y = paired(150, 4, 3, 31)  # Y = X A + 0.5 noise: both denominators are far from 0
    s = sig(kernel, 4, 3)
    (vxy, sxy), (vxx, sxx), (vyy, syy) = o_three(X, Y, kernel, s)
    want = o_correlation(X, Y, kernel, s)
    assert vxx > 0.0 and vyy > 0.0 and 0.1 < want < 1.0
    tol = abs(want) * RTOL * (sxy / abs(vxy) + sxx / (2.0 * abs(vxx)) + syy / (2.0 * abs(vyy)))
    got = hs.correlation(X, Y, kernel, s)
    print(kernel, got, want, tol)
    assert isinstance(got, np.float64) and abs(got - want) <= tol
    # X against its copy: the three statistics are the same bits, so v / sqrt(v * v) is 1 up to
    # the roundings of one product, one root and one quotient
    one = hs.correlation(X, X.copy(), kernel, s[0] if s else None)
    assert abs(one - 1.0) <= 1e-15
    # a constant side has no variance to normalise by
    assert np.isnan(hs.correlation(X, np.ones_like(Y), "distance"))


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_dimensional_samples(hs, kernel):
    rng = np.random.RandomState(8)
    X = rng.normal(size=300)
    Y = X * X + 0.3 * rng.normal(size=300)
    s = sig(kernel, 1, 1)
    got = hs.Un(X, Y, kernel, s)
    want, scale = ref_Un(X, Y, kernel, s)
    assert abs(got - want) <= RTOL * scale and got > 0.0
    Xo, Yo = X.copy(), Y.copy()
    np.random.seed(1)
    got = hs.UnNB(X, Y, 4, 50, kernel=kernel, sigma=s)
    np.random.seed(1)
    want, scale = ref_blocks(Xo, Yo, 4, 1, lambda x, y: ref_UB(x, y, 50, kernel, s))
    assert abs(got - want) <= RTOL * scale and np.array_equal(X, Xo) and np.array_equal(Y, Yo)
