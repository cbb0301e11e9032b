"""tuplewise.hsic_var on the device: tw_hsic_rows against the fsum oracle of
tests/test_hsic_var_cpu.py over tile edges and dimensions, without weights and with the oracle's
row sums as weights, mixed blocks in one launch with sentinels, the bit contracts (run to run,
alone / beside other blocks / at another start, a pair alone / inside a grid, the first sum with
and without weights), the identities against tw_hsic_sums, exact cases, and the public functions."""
import math

import numpy as np
import pytest

from test_hsic_cpu import KERNELS, o_fsum, o_KL, o_Un_scale, paired, sig
from test_hsic_var_cpu import o_h_scale, o_rows, o_rows_of, o_select, o_Un_var
from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 64


def coefs(sigma):
    """The coefficient pair of one sigma of hsic (None: the distance kernel's unused zeros)."""
    if sigma is None:
        return (0.0, 0.0)
    sx, sy = sigma if isinstance(sigma, tuple) else (sigma, sigma)
    return (-1.0 / (2.0 * sx * sx), -1.0 / (2.0 * sy * sy))


def native_rows(tw, X, Y, off, kernel, cs, w=None):
    """tw_hsic_rows called directly: d_rows as (S, rows, 3).  The output and the work buffer are
    followed by PAD sentinels, which must survive, and are pre-filled with the sentinel, so that
    rows that are not written show it.  w: (S, rows, 3) weights (a previous launch's rows)."""
    import torch
    L = tw._lib
    X, Y = X.reshape(len(X), -1), Y.reshape(len(Y), -1)
    off = np.asarray(off, dtype=np.int64)
    nb, S, rows, max_n = len(off) - 1, len(cs), int(off[-1]), int(np.diff(off).max())
    dev = L.device()
    xd, yd = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Y.copy()).to(dev)
    od = torch.from_numpy(off).to(dev)
    cd = torch.from_numpy(np.asarray(cs, dtype=np.float64).reshape(-1)).to(dev)
    wd = None
    if w is not None:
        assert w.shape == (S, rows, 3)
        wd = torch.from_numpy(np.ascontiguousarray(w)).to(dev)
    nbytes = L.lib().tw_hsic_rows_work_bytes(nb, max_n, S)
    assert nbytes > 0 and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    out = torch.full((S * rows * 3 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    L.call("tw_hsic_rows", xd, X.shape[1], yd, Y.shape[1], od, nb, max_n, KERNELS.index(kernel), cd,
           S, wd, work, out, L.stream_handle())
    torch.cuda.synchronize()
    out, tail = out.cpu().numpy(), work[nbytes // 8:].cpu().numpy()
    assert np.all(out[S * rows * 3:] == SENTINEL) and np.all(tail == SENTINEL), \
        "a sentinel behind a buffer was overwritten"
    return out[:S * rows * 3].reshape(S, rows, 3)


def weights_of(k, l, rows=None, at=0):  # noqa: E741
    """(rows, 3) weights as a first launch leaves them: [:, 1] = k, [:, 2] = l; NaN in the column
    the kernel must not read and in every row outside [at, at + len(k))."""
    w = np.full((len(k) if rows is None else rows, 3), np.nan)
    w[at:at + len(k), 1], w[at:at + len(k), 2] = k, l
    return w


def close_rows(got, want, what):
    """rtol 1e-12 of the row's sum of |terms| (every term is >= 0: the oracle's sum itself); NaN
    exactly where the oracle has it."""
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs(got[~nan] - want[~nan])
    assert np.all(err <= 1e-12 * want[~nan]), (what, err.max())


def check_block(first, second, want, what):
    """first = (p, k, l) and second = (p, u, v) of one block against the oracle's five rows."""
    for got, w, name in ((first[:, 0], want[0], "p"), (first[:, 1], want[1], "k"),
                         (first[:, 2], want[2], "l"), (second[:, 1], want[3], "u"),
                         (second[:, 2], want[4], "v")):
        close_rows(got, w, f"{what} {name}")
    assert np.array_equal(first[:, 0], second[:, 0], equal_nan=True), what + ": p with weights"


def grid_of(kernel, dx, dy):
    if kernel == "distance":
        return [None]
    return [sig(kernel, dx, dy), (0.6 * math.sqrt(dx), 2.5 * math.sqrt(dy))]


# ------------------------------------------------------------------------- rows vs the oracle
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("dx,dy", [(1, 1), (8, 9), (63, 64), (64, 2)])
def test_rows_match_the_oracle(tw, gpu, kernel, dx, dy):
    P = tw._lib.lib().tw_hsic_tile()
    grid = grid_of(kernel, dx, dy)
    cs = [coefs(s) for s in grid]
    for n in (4, 5, P - 1, P, P + 1, 2 * P + 3, 4 * P + 5):
        X, Y = paired(n, dx, dy, 10 + dx)
        want = [o_rows(X, Y, kernel, s) for s in grid]
        first = native_rows(tw, X, Y, [0, n], kernel, cs)
        w = np.stack([weights_of(t[1], t[2]) for t in want])  # the oracle's k, l as weights
        second = native_rows(tw, X, Y, [0, n], kernel, cs, w)
        assert first.shape == second.shape == (len(grid), n, 3)
        for s in range(len(grid)):
            check_block(first[s], second[s], want[s], f"n={n} dx={dx} dy={dy} s={s}")


def mixed_partition(P, dx, dy, seed):
    sizes = [4, P + 1, 5, 2 * P, P - 1]
    off = np.cumsum([7] + sizes)
    X, Y = paired(int(off[-1]), dx, dy, seed)
    return X, Y, off


def oracle_weights(X, Y, off, kernel, grid):
    """(want[s][b], w (S, rows, 3)) of a partition: the blocks' oracle rows and their k, l as the
    weights of a second launch (NaN outside every block)."""
    want = [[o_rows(X[off[b]:off[b + 1]], Y[off[b]:off[b + 1]], kernel, s)
             for b in range(len(off) - 1)] for s in grid]
    w = np.full((len(grid), int(off[-1]), 3), np.nan)
    for s in range(len(grid)):
        for b in range(len(off) - 1):
            w[s, off[b]:off[b + 1], 1], w[s, off[b]:off[b + 1], 2] = want[s][b][1], want[s][b][2]
    return want, w


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_blocks_in_one_launch(tw, gpu, kernel):
    P, dx, dy = tw._lib.lib().tw_hsic_tile(), 5, 3
    X, Y, off = mixed_partition(P, dx, dy, 3)
    grid = grid_of(kernel, dx, dy)
    cs = [coefs(s) for s in grid]
    want, w = oracle_weights(X, Y, off, kernel, grid)
    first = native_rows(tw, X, Y, off, kernel, cs)
    second = native_rows(tw, X, Y, off, kernel, cs, w)
    # the rows of the leading gap belong to no block: not written
    assert np.all(first[:, :7] == SENTINEL) and np.all(second[:, :7] == SENTINEL)
    for s in range(len(grid)):
        for b in range(len(off) - 1):
            blk = slice(off[b], off[b + 1])
            check_block(first[s, blk], second[s, blk], want[s][b], f"block {b} s={s}")


# ------------------------------------------------------------------------------ bit contracts
@pytest.mark.parametrize("kernel", KERNELS)
def test_block_rows_are_the_same_bits_wherever_the_block_stands(tw, gpu, kernel):
    P, dx, dy = tw._lib.lib().tw_hsic_tile(), 9, 4
    X, Y, off = mixed_partition(P, dx, dy, 4)
    cs = [coefs(s) for s in grid_of(kernel, dx, dy)]
    first = native_rows(tw, X, Y, off, kernel, cs)
    second = native_rows(tw, X, Y, off, kernel, cs, first)  # the first launch's rows as weights
    assert np.array_equal(first, native_rows(tw, X, Y, off, kernel, cs))  # run to run
    assert np.array_equal(second, native_rows(tw, X, Y, off, kernel, cs, first))
    assert np.array_equal(first[:, 7:, 0], second[:, 7:, 0])  # p with and without weights
    nb = len(off) - 1
    for b in range(nb):
        blk = slice(off[b], off[b + 1])
        # alone in a launch, at its own place (everything before it is a leading gap)
        a1 = native_rows(tw, X[:off[b + 1]], Y[:off[b + 1]], off[b:b + 2], kernel, cs)
        a2 = native_rows(tw, X[:off[b + 1]], Y[:off[b + 1]], off[b:b + 2], kernel, cs,
                         first[:, :off[b + 1]])
        assert np.array_equal(a1[:, blk], first[:, blk]) and np.array_equal(a2[:, blk], second[:, blk]), b
        assert np.all(a1[:, :off[b]] == SENTINEL) and np.all(a2[:, :off[b]] == SENTINEL)
        # at another partition start: the block's rows moved to row 0
        m1 = native_rows(tw, X[blk], Y[blk], [0, off[b + 1] - off[b]], kernel, cs)
        m2 = native_rows(tw, X[blk], Y[blk], [0, off[b + 1] - off[b]], kernel, cs,
                         np.ascontiguousarray(first[:, blk]))
        assert np.array_equal(m1, first[:, blk]) and np.array_equal(m2, second[:, blk]), b
    # beside other blocks of another size (max_n and the launch plan change)
    t1 = native_rows(tw, X[:off[2]], Y[:off[2]], off[:3], kernel, cs)
    t2 = native_rows(tw, X[:off[2]], Y[:off[2]], off[:3], kernel, cs, first[:, :off[2]])
    assert np.array_equal(t1[:, 7:], first[:, 7:off[2]]) and np.array_equal(t2[:, 7:], second[:, 7:off[2]])


def test_pair_rows_do_not_depend_on_the_grid(tw, gpu):
    import tuplewise.hsic_var as hv
    lib = tw._lib.lib()
    P, smax, dx, dy = lib.tw_hsic_tile(), lib.tw_hsic_rows_max_sigma(), 6, 3
    n = 2 * P + 37
    X, Y = paired(n, dx, dy, 21)
    pairs = [(float(a), float(b)) for a, b in zip(np.geomspace(0.5, 9.0, smax + 1),
                                                  np.geomspace(7.0, 0.4, smax + 1))]
    cs = [coefs(s) for s in pairs]
    g1 = native_rows(tw, X, Y, [0, n], "gaussian", cs[:smax])
    g2 = native_rows(tw, X, Y, [0, n], "gaussian", cs[:smax], g1)
    ones = []
    for s, c in enumerate(cs):
        o1 = native_rows(tw, X, Y, [0, n], "gaussian", [c])
        o2 = native_rows(tw, X, Y, [0, n], "gaussian", [c], o1)
        ones.append((o1[0], o2[0]))
        if s < smax:
            assert np.array_equal(o1[0], g1[s]) and np.array_equal(o2[0], g2[s]), s
    # another position, other neighbours, another length
    perm = [smax - 1, 0][:smax]
    p1 = native_rows(tw, X, Y, [0, n], "gaussian", [cs[i] for i in perm])
    p2 = native_rows(tw, X, Y, [0, n], "gaussian", [cs[i] for i in perm], p1)
    for s, i in enumerate(perm):
        assert np.array_equal(p1[s], g1[i]) and np.array_equal(p2[s], g2[i]), i
    # a grid of max_sigma + 1 pairs splits into two launches without changing a number
    rows = hv.row_sums(X, Y, sigma=pairs)
    assert rows.p.shape == (smax + 1, n)
    for s, (o1, o2) in enumerate(ones):
        got = np.stack([r[s] for r in rows], axis=1)
        assert np.array_equal(got, np.stack([o1[:, 0], o1[:, 1], o1[:, 2], o2[:, 1], o2[:, 2]], axis=1)), s


# -------------------------------------------------------- identities against the existing kernel
@pytest.mark.parametrize("kernel", KERNELS)
def test_rows_against_tw_hsic_sums(tw, gpu, kernel):
    import tuplewise.hsic as hs
    import tuplewise.hsic_var as hv
    P = tw._lib.lib().tw_hsic_tile()
    X, Y = paired(2 * P + 9, 8, 5, 31)
    sigma = sig(kernel, 8, 5)
    rows = hv.row_sums(X, Y, kernel, sigma)
    k, l = hs.row_sums(X, Y, kernel, sigma)  # noqa: E741
    assert np.all(np.abs(rows.k - k) <= 1e-12 * k) and np.all(np.abs(rows.l - l) <= 1e-12 * l)
    c = hs.components(X, Y, kernel, sigma)
    assert abs(o_fsum(rows.p) / 2.0 - c.S_KL) <= 1e-12 * c.S_KL
    # sum(u) = sum(v) = R_KL, every term >= 0
    assert abs(o_fsum(rows.u) - c.R_KL) <= 2e-12 * c.R_KL
    assert abs(o_fsum(rows.v) - c.R_KL) <= 2e-12 * c.R_KL


# --------------------------------------------------------------------------------- exact cases
def test_duplicates_under_a_huge_coefficient_count_exactly(tw, gpu):
    P = tw._lib.lib().tw_hsic_tile()
    n, d = 2 * P + 5, 3
    gx, gy = np.arange(n) % 5, np.arange(n) % 3
    X = np.repeat(gx[:, None], d, 1).astype(np.float64)
    Y = np.repeat(gy[:, None], 2, 1).astype(np.float64)
    first = native_rows(tw, X, Y, [0, n], "gaussian", [(-1e300, -1e300)])
    second = native_rows(tw, X, Y, [0, n], "gaussian", [(-1e300, -1e300)], first)
    K = (gx[:, None] == gx[None, :]).astype(np.float64)
    L = (gy[:, None] == gy[None, :]).astype(np.float64)
    np.fill_diagonal(K, 0.0)
    np.fill_diagonal(L, 0.0)
    k, l = K.sum(1), L.sum(1)  # noqa: E741  (small integers: every sum below is exact)
    assert np.array_equal(first[0], np.stack([(K * L).sum(1), k, l], axis=1))
    assert np.array_equal(second[0], np.stack([(K * L).sum(1), K @ l, L @ k], axis=1))
    # the distance kernel on equal rows: exact zeros
    Z = np.zeros((5, d))
    assert np.all(native_rows(tw, Z, Z[:, :2], [0, 5], "distance", [(0.0, 0.0)]) == 0.0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_nan_of_another_block_changes_nothing(tw, gpu, kernel):
    P, dx, dy = tw._lib.lib().tw_hsic_tile(), 4, 3
    X, Y, off = mixed_partition(P, dx, dy, 8)
    cs = [coefs(s) for s in grid_of(kernel, dx, dy)]
    first = native_rows(tw, X, Y, off, kernel, cs)
    second = native_rows(tw, X, Y, off, kernel, cs, first)
    Xn, Yn = X.copy(), Y.copy()
    Xn[off[2] + 1, 2] = np.nan  # block 2 of 5 rows
    Yn[off[4] - 1, 0] = np.nan  # the last row of block 3: beside block 4's first row
    f = native_rows(tw, Xn, Yn, off, kernel, cs)
    s = native_rows(tw, Xn, Yn, off, kernel, cs, f)
    for b in (0, 1, 4):
        blk = slice(off[b], off[b + 1])
        assert np.array_equal(f[:, blk], first[:, blk]) and np.array_equal(s[:, blk], second[:, blk]), b
    b2, b3 = slice(off[2], off[3]), slice(off[3], off[4])
    # x of block 2: p and k are NaN, l is as it was; y of block 3: p and l are NaN, k as it was
    assert np.isnan(f[:, b2, :2]).all() and np.array_equal(f[:, b2, 2], first[:, b2, 2])
    assert np.isnan(f[:, b3, 0]).all() and np.isnan(f[:, b3, 2]).all()
    assert np.array_equal(f[:, b3, 1], first[:, b3, 1])
    assert np.isnan(s[:, b2]).all() and np.isnan(s[:, b3]).all()  # K l and L k read both sides


@pytest.mark.parametrize("kernel", KERNELS)
def test_nan_rows_are_the_oracles(tw, gpu, kernel):
    P, dx, dy = tw._lib.lib().tw_hsic_tile(), 4, 3
    n = P + 9
    X, Y = paired(n, dx, dy, 8, "nan")
    sigma = sig(kernel, dx, dy)
    K, L = o_KL(X, Y, kernel, sigma)
    want = o_rows_of(K, L)
    assert np.isnan(want[0]).all() and np.isnan(want[1]).all() and not np.isnan(want[2]).any()
    assert np.isnan(want[3]).all() and np.isnan(want[4]).all()
    first = native_rows(tw, X, Y, [0, n], kernel, [coefs(sigma)])
    second = native_rows(tw, X, Y, [0, n], kernel, [coefs(sigma)], first)
    check_block(first[0], second[0], want, "nan")
    # finite weights: the sum over L's factors is untouched by the NaN in x
    rng = np.random.RandomState(3)
    wk, wl = rng.uniform(0.5, 2.0, n), rng.uniform(0.5, 2.0, n)
    got = native_rows(tw, X, Y, [0, n], kernel, [coefs(sigma)], weights_of(wl, wk)[None])
    with np.errstate(invalid="ignore"):
        close_rows(got[0, :, 1], np.array([o_fsum(a * wk) for a in K]), "K wk")
    close_rows(got[0, :, 2], np.array([o_fsum(b * wl) for b in L]), "L wl")
    assert not np.isnan(got[0, :, 2]).any()


# ------------------------------------------------------------------------- public functions
@pytest.mark.parametrize("kernel", KERNELS)
def test_Un_var_matches_the_oracle(tw, gpu, kernel):
    """h at atol = 4e-12 x the sum of the absolute values of the terms of h_i's formula (each a
    product of two sums good to 1e-12, or a sum over weights good to 1e-12, doubled)."""
    import tuplewise.hsic as hs
    import tuplewise.hsic_var as hv
    P = tw._lib.lib().tw_hsic_tile()
    n = 2 * P + 44
    X, Y = paired(n, 8, 5, 41)
    sigma = sig(kernel, 8, 5)
    rows = o_rows(X, Y, kernel, sigma)
    v, want = hv.Un_var(X, Y, kernel, sigma), o_Un_var(X, Y, kernel, sigma)
    atol = 4e-12 * o_h_scale(*rows)
    err = np.abs(v.h - want[3])
    print(f"{kernel}: value {v.value!r} (oracle {want[0]!r}), var {v.var!r} (oracle {want[1]!r}), "
          f"max err / atol {np.max(err / atol):.3g}")
    assert v.h.shape == (n,) and np.all(err <= atol)
    scale = o_Un_scale(X, Y, kernel, sigma)
    assert abs(v.value - hs.Un(X, Y, kernel, sigma)) <= 1e-12 * scale
    assert abs(v.value - want[0]) <= atol.mean()
    assert v.var > 0 and v.se == math.sqrt(v.var) and v.var == 16.0 * v.zeta / n
    value, lo, hi = hv.Un_ci(X, Y, 0.95, kernel, sigma)
    assert value == v.value and lo < value < hi and abs((hi - lo) / (2 * 1.959963984540054) - v.se) <= 1e-12 * v.se


@pytest.mark.parametrize("kernel", KERNELS)
def test_UnN_var_matches_UnN(tw, gpu, kernel):
    import tuplewise.hsic as hs
    import tuplewise.hsic_var as hv
    X, Y = paired(530, 5, 3, 43)
    sigma = sig(kernel, 5, 3)
    copies = [(X.copy(), Y.copy()) for _ in range(2)]
    np.random.seed(9)
    value, var = hv.UnN_var(*copies[0], 4, kernel=kernel, sigma=sigma)
    s0 = np.random.get_state()
    np.random.seed(9)
    un = hs.UnN(*copies[1], 4, kernel=kernel, sigma=sigma)
    s1 = np.random.get_state()
    k = 530 // 4
    A, B = copies[0]
    blocks = [o_Un_var(A[b * k:(b + 1) * k], B[b * k:(b + 1) * k], kernel, sigma) for b in range(4)]
    scale = np.mean([o_Un_scale(A[b * k:(b + 1) * k], B[b * k:(b + 1) * k], kernel, sigma)
                     for b in range(4)])
    assert abs(value - un) <= 1e-12 * scale
    assert abs(value - np.mean([t[0] for t in blocks])) <= 4e-12 * scale
    # a block's rows are the same bits alone: var is the mean of the blocks' own var over N
    own = [hv.Un_var(A[b * k:(b + 1) * k], B[b * k:(b + 1) * k], kernel, sigma).var for b in range(4)]
    assert abs(var - np.mean(own) / 4) <= 1e-12 * var and var > 0
    print(f"{kernel}: var {var!r}, oracle {np.mean([t[1] for t in blocks]) / 4!r}")
    assert same_state(s0, s1)
    for C, D in zip(copies[0], copies[1]):
        assert np.array_equal(C, D)
    assert not np.array_equal(A, X)


def test_select_sigma_matches_the_oracle(tw, gpu):
    import tuplewise.hsic_var as hv
    rng = np.random.RandomState(5)
    X = rng.normal(size=(150, 2))
    Y = X[:, :1] + 0.7 * rng.normal(size=(150, 1))
    side = np.geomspace(0.1, 30.0, 6)
    grid = [(float(a), float(b)) for a in side[::2] for b in side[1::2]]  # 9 pairs: 3 launches
    sel = hv.select_sigma(X, Y, grid)
    index, crit, value, var = o_select(X, Y, grid)
    print("criterion", sel.criterion, "oracle", crit)
    top = np.sort(crit)[::-1]
    assert top[0] - top[1] > 1e-6 * top[0]  # the oracle's best is clear of the second
    assert sel.index == index and sel.sigma == grid[index]
    assert np.all(np.abs(sel.value - value) <= 4e-12 * np.array(
        [o_h_scale(*o_rows(X, Y, "gaussian", s)).mean() for s in grid]))
    one = hv.Un_var(X, Y, sigma=grid[:2])
    assert np.array_equal(one.value, sel.value[:2]) and np.array_equal(one.var, sel.var[:2])


def test_median_inside_a_grid_is_its_number(tw, gpu):
    import tuplewise.bandwidth as bw
    import tuplewise.hsic_var as hv
    X, Y = paired(90, 4, 3, 17)
    mx, my = float(bw.median_distance(X)), float(bw.median_distance(Y))
    a = hv.Un_var(X, Y, sigma=[(0.5, 1.0), ("median", "median"), ("median", 2.0), (4.0, "median")])
    b = hv.Un_var(X, Y, sigma=[(0.5, 1.0), (mx, my), (mx, 2.0), (4.0, my)])
    one = hv.Un_var(X, Y, sigma="median")
    for f in hv.HSICVariance._fields:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(getattr(a, f)[1], getattr(one, f)), f
    ra, rb = hv.row_sums(X, Y, sigma=("median", 2.0)), hv.row_sums(X, Y, sigma=(mx, 2.0))
    assert all(np.array_equal(p, q) for p, q in zip(ra, rb))
    sel = hv.select_sigma(X, Y, [("median", "median")])
    assert sel.sigma == (mx, my) and sel.index == 0
