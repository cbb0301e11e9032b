"""tuplewise.mmd_var on the device: tw_mmd_rows against the fsum oracle of tests/test_mmd_var_cpu.py
over tile edges, dimensions and grid lengths, mixed blocks in one launch with sentinels, the bit
contracts (run to run, alone / beside other blocks / at another start, a sigma alone / inside a
grid), the identities against tw_mmd_sums, exact cases, and the public functions."""
import math

import numpy as np
import pytest

from test_mmd_cpu import KERNELS, o_Un_scale, o_g
from test_mmd_var_cpu import o_Un_var, o_UnN_var, o_fsum, o_row_sums, o_select
from test_triplets_cpu import data, o_dist_rows, same_state

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
PAD = 64


def coef(sigma):
    return -1.0 / (2.0 * sigma * sigma)


def native_rows(tw, X, Z, bxo, bzo, kernel, cs):
    """tw_mmd_rows called directly: (rows_x (S, nx, 2), rows_z (S, nz, 2)); every output and the
    work buffer are followed by PAD sentinels, which must survive, and are pre-filled with the
    sentinel, so that rows that are not written show it."""
    import torch
    L = tw._lib
    X, Z = X.reshape(len(X), -1), Z.reshape(len(Z), -1)
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb, S = len(bxo) - 1, len(cs)
    nx, nz = int(bxo[-1]), int(bzo[-1])
    max_n, max_m = int(np.diff(bxo).max()), int(np.diff(bzo).max())
    dev = L.device()
    xd, zd = torch.from_numpy(X.copy()).to(dev), torch.from_numpy(Z.copy()).to(dev)
    bx, bz = torch.from_numpy(bxo).to(dev), torch.from_numpy(bzo).to(dev)
    cd = torch.from_numpy(np.asarray(cs, dtype=np.float64)).to(dev)
    nbytes = L.lib().tw_mmd_rows_work_bytes(nb, max_n, max_m, S)
    assert nbytes > 0 and nbytes % 8 == 0
    work = torch.full((nbytes // 8 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    rx = torch.full((S * nx * 2 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    rz = torch.full((S * nz * 2 + PAD,), SENTINEL, dtype=torch.float64, device=dev)
    L.call("tw_mmd_rows", xd, zd, X.shape[1], bx, bz, nb, max_n, max_m, KERNELS.index(kernel), cd, S,
           work, rx, rz, L.stream_handle())
    torch.cuda.synchronize()
    rx, rz, tail = rx.cpu().numpy(), rz.cpu().numpy(), work[nbytes // 8:].cpu().numpy()
    for t in (rx[S * nx * 2:], rz[S * nz * 2:], tail):
        assert np.all(t == SENTINEL), "a sentinel behind a buffer was overwritten"
    return rx[:S * nx * 2].reshape(S, nx, 2), rz[:S * nz * 2].reshape(S, nz, 2)


def o_rows_of_terms(D3, kernel, sigma):
    """(a, r, q, b) by fsum from the three distance matrices (Dxx, Dxz, Dzz)."""
    gxx, gxz, gzz = (o_g(D, kernel, sigma) for D in D3)
    n, m = gxz.shape
    gxx, gzz = gxx[~np.eye(n, dtype=bool)].reshape(n, n - 1), gzz[~np.eye(m, dtype=bool)].reshape(m, m - 1)
    return (np.array([o_fsum(t) for t in gxx]), np.array([o_fsum(t) for t in gxz]),
            np.array([o_fsum(t) for t in gxz.T]), np.array([o_fsum(t) for t in gzz]))


def close_rows(got, want, what):
    """rtol 1e-12 of the row's sum of |terms| (g >= 0: the oracle's sum itself); NaN exactly where
    the oracle has it."""
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    err = np.abs(got[~nan] - want[~nan])
    assert np.all(err <= 1e-12 * want[~nan]), (what, err.max())


def check_block(rx, rz, want, what):
    close_rows(rx[:, 0], want[0], what + " a")
    close_rows(rx[:, 1], want[1], what + " r")
    close_rows(rz[:, 0], want[2], what + " q")
    close_rows(rz[:, 1], want[3], what + " b")


def shapes(P):
    return [(2, 2), (P - 1, P + 1), (P, 2 * P + 3), (2 * P + 1, 5), (3, 2 * P)]


# ------------------------------------------------------------------------- rows vs the oracle
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [1, 2, 3, 8, 17, 37, 64])
def test_rows_match_the_oracle(tw, gpu, kernel, d):
    lib = tw._lib.lib()
    P, smax = lib.tw_mmd_tile(), lib.tw_mmd_rows_max_sigma()
    base = math.sqrt(d)
    for n, m in shapes(P):
        X, Z = data("gauss", n, m, d, 10 + d)
        D3 = (o_dist_rows(X, X), o_dist_rows(X, Z), o_dist_rows(Z, Z))
        grids = [[None]] if kernel == "energy" else [
            [base], [0.4 * base, base, 3.0 * base], list(base * np.geomspace(0.2, 6.0, smax))]
        oracle = {}
        for grid in grids:
            cs = [0.0 if s is None else coef(s) for s in grid]
            rx, rz = native_rows(tw, X, Z, [0, n], [0, m], kernel, cs)
            assert rx.shape == (len(grid), n, 2) and rz.shape == (len(grid), m, 2)
            for s, sigma in enumerate(grid):
                if sigma not in oracle:
                    oracle[sigma] = o_rows_of_terms(D3, kernel, sigma)
                check_block(rx[s], rz[s], oracle[sigma], f"n={n} m={m} d={d} S={len(grid)} s={s}")


def mixed_partition(P, d, seed):
    sizes = [(2, 2), (P + 1, 5), (65, P + 1), (2 * P + 3, 3)]
    bxo = np.cumsum([7] + [s[0] for s in sizes])
    bzo = np.cumsum([3] + [s[1] for s in sizes])
    rng = np.random.RandomState(seed)
    return rng.normal(size=(bxo[-1], d)), rng.normal(0.3, 1.0, size=(bzo[-1], d)), bxo, bzo


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_blocks_in_one_launch(tw, gpu, kernel):
    P, d = tw._lib.lib().tw_mmd_tile(), 5
    X, Z, bxo, bzo = mixed_partition(P, d, 3)
    sigmas = [None] if kernel == "energy" else [1.0, 2.5, 6.0]
    cs = [0.0 if s is None else coef(s) for s in sigmas]
    rx, rz = native_rows(tw, X, Z, bxo, bzo, kernel, cs)
    # the rows of the leading gaps belong to no block: not written
    assert np.all(rx[:, :7] == SENTINEL) and np.all(rz[:, :3] == SENTINEL)
    for s, sigma in enumerate(sigmas):
        for b in range(4):
            x, z = X[bxo[b]:bxo[b + 1]], Z[bzo[b]:bzo[b + 1]]
            check_block(rx[s, bxo[b]:bxo[b + 1]], rz[s, bzo[b]:bzo[b + 1]],
                        o_row_sums(x, z, kernel, sigma), f"block {b} s={s}")


# ------------------------------------------------------------------------------ bit contracts
@pytest.mark.parametrize("kernel", KERNELS)
def test_block_rows_are_the_same_bits_wherever_the_block_stands(tw, gpu, kernel):
    P, d = tw._lib.lib().tw_mmd_tile(), 9
    X, Z, bxo, bzo = mixed_partition(P, d, 4)
    cs = [0.0] if kernel == "energy" else [coef(2.0), coef(5.0)]
    rx, rz = native_rows(tw, X, Z, bxo, bzo, kernel, cs)
    again = native_rows(tw, X, Z, bxo, bzo, kernel, cs)
    assert np.array_equal(rx, again[0]) and np.array_equal(rz, again[1])  # run to run
    for b in range(4):
        bx, bz = slice(bxo[b], bxo[b + 1]), slice(bzo[b], bzo[b + 1])
        # alone in a launch, at its own place (everything before it is a leading gap)
        ax, az = native_rows(tw, X[:bxo[b + 1]], Z[:bzo[b + 1]], bxo[b:b + 2], bzo[b:b + 2], kernel, cs)
        assert np.array_equal(ax[:, bx], rx[:, bx]) and np.array_equal(az[:, bz], rz[:, bz]), b
        assert np.all(ax[:, :bxo[b]] == SENTINEL) and np.all(az[:, :bzo[b]] == SENTINEL)
        # at another partition start: the block's rows moved to row 0
        mx, mz = native_rows(tw, X[bx], Z[bz], [0, bxo[b + 1] - bxo[b]], [0, bzo[b + 1] - bzo[b]],
                             kernel, cs)
        assert np.array_equal(mx, rx[:, bx]) and np.array_equal(mz, rz[:, bz]), b
    # beside other blocks of another size (max_n, max_m and the launch plan change)
    tx, tz = native_rows(tw, X, Z, bxo[:3], bzo[:3], kernel, cs)
    assert np.array_equal(tx[:, 7:], rx[:, 7:bxo[2]]) and np.array_equal(tz[:, 3:], rz[:, 3:bzo[2]])


def test_sigma_rows_do_not_depend_on_the_grid(tw, gpu):
    lib = tw._lib.lib()
    P, smax, d = lib.tw_mmd_tile(), lib.tw_mmd_rows_max_sigma(), 6
    n, m = P + 37, 2 * P + 1
    X, Z = data("gauss", n, m, d, 21)
    cs = [coef(s) for s in np.geomspace(0.3, 12.0, smax)]
    gx, gz = native_rows(tw, X, Z, [0, n], [0, m], "gaussian", cs)
    for s, c in enumerate(cs):
        ox, oz = native_rows(tw, X, Z, [0, n], [0, m], "gaussian", [c])
        assert np.array_equal(ox[0], gx[s]) and np.array_equal(oz[0], gz[s]), s
    # another position, other neighbours, another length
    perm = [5, 0, 3]
    px, pz = native_rows(tw, X, Z, [0, n], [0, m], "gaussian", [cs[i] for i in perm])
    for s, i in enumerate(perm):
        assert np.array_equal(px[s], gx[i]) and np.array_equal(pz[s], gz[i]), i


# -------------------------------------------------------- identities against the existing kernel
@pytest.mark.parametrize("kernel", KERNELS)
def test_sums_of_rows_are_the_components(tw, gpu, kernel):
    import tuplewise.mmd as mm
    import tuplewise.mmd_var as mv
    P = tw._lib.lib().tw_mmd_tile()
    X, Z = data("gauss", 2 * P + 9, P + 70, 8, 31)
    sigma = 2.5 if kernel == "gaussian" else None
    rows = mv.row_sums(X, Z, kernel, sigma)
    sxx, szz, sxz = mm.components(X, Z, kernel, sigma)
    for got, want in ((o_fsum(rows.a) / 2.0, sxx), (o_fsum(rows.b) / 2.0, szz),
                      (o_fsum(rows.r), sxz), (o_fsum(rows.q), sxz)):
        assert abs(got - want) <= 1e-12 * want, (got, want)


# --------------------------------------------------------------------------------- exact cases
def test_duplicates_under_a_huge_coefficient_count_exactly(tw, gpu):
    P = tw._lib.lib().tw_mmd_tile()
    n, m, d = 2 * P + 5, P + 3, 3
    gx, gz = np.arange(n) % 5, np.arange(m) % 3
    X, Z = np.repeat(gx[:, None], d, 1).astype(np.float64), np.repeat(gz[:, None], d, 1).astype(np.float64)
    rx, rz = native_rows(tw, X, Z, [0, n], [0, m], "gaussian", [-1e300])
    cx, cz = np.bincount(gx, minlength=5), np.bincount(gz, minlength=5)
    assert np.array_equal(rx[0, :, 0], cx[gx] - 1.0) and np.array_equal(rx[0, :, 1], cz[gx] * 1.0)
    assert np.array_equal(rz[0, :, 0], cx[gz] * 1.0) and np.array_equal(rz[0, :, 1], cz[gz] - 1.0)
    # the energy kernel on the same rows: integers times sqrt(3), and exact zeros among duplicates
    X2 = np.zeros((4, d))
    ex, ez = native_rows(tw, X2, X2[:3], [0, 4], [0, 3], "energy", [0.0])
    assert np.all(ex == 0.0) and np.all(ez == 0.0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_nan_rows_are_the_oracles(tw, gpu, kernel):
    P = tw._lib.lib().tw_mmd_tile()
    n, m, d = P + 9, 2 * P - 1, 4
    X, Z = data("nan", n, m, d, 8)
    sigma = 1.7 if kernel == "gaussian" else None
    rx, rz = native_rows(tw, X, Z, [0, n], [0, m], kernel, [0.0 if sigma is None else coef(sigma)])
    want = o_row_sums(X, Z, kernel, sigma)
    assert np.isnan(want[0]).all() and np.isnan(want[2]).all() and not np.isnan(want[3]).any()
    assert np.isnan(want[1]).sum() == 1
    check_block(rx[0], rz[0], want, "nan")


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_sample_against_its_copy(tw, gpu, kernel):
    import tuplewise.mmd_var as mv
    P = tw._lib.lib().tw_mmd_tile()
    X, _ = data("gauss", 2 * P + 1, 2, 7, 12)
    sigma = 2.0 if kernel == "gaussian" else None
    rows = mv.row_sums(X, X.copy(), kernel, sigma)
    diag = 1.0 if kernel == "gaussian" else 0.0  # g(x, x): the cross sums hold the diagonal term
    for own, cross in ((rows.a, rows.q), (rows.b, rows.r), (rows.a, rows.r), (rows.b, rows.q)):
        assert np.all(np.abs(cross - (own + diag)) <= 1e-12 * (own + diag))
    assert np.all(np.abs(rows.a - rows.b) <= 1e-12 * rows.a)
    assert np.all(np.abs(rows.r - rows.q) <= 1e-12 * rows.r)


# ------------------------------------------------------------------------- public functions
@pytest.mark.parametrize("kernel", KERNELS)
def test_Un_var_matches_the_oracle(tw, gpu, kernel):
    import tuplewise.mmd as mm
    import tuplewise.mmd_var as mv
    X, Z = data("gauss", 300, 200, 8, 41)
    sigma = 3.0 if kernel == "gaussian" else None
    v, want = mv.Un_var(X, Z, kernel, sigma), o_Un_var(X, Z, kernel, sigma)
    scale = o_Un_scale(X, Z, kernel, sigma)
    print(f"{kernel}: value {v.value!r} (oracle {want[0]!r}), var {v.var!r} (oracle {want[1]!r})")
    assert abs(v.value - want[0]) <= 1e-12 * scale
    assert abs(v.var - want[1]) <= 1e-9 * want[1]
    assert np.all(np.abs(v.phi_x - want[2]) <= 1e-12 * scale) and v.phi_x.shape == (300,)
    assert np.all(np.abs(v.phi_z - want[3]) <= 1e-12 * scale) and v.phi_z.shape == (200,)
    assert abs(v.zeta_x - want[4]) <= 1e-9 * want[4] and abs(v.zeta_z - want[5]) <= 1e-9 * want[5]
    assert abs(v.value - mm.Un(X, Z, kernel, sigma)) <= 1e-12 * scale


@pytest.mark.parametrize("kernel", KERNELS)
def test_UnN_var_matches_the_oracle_and_UnN(tw, gpu, kernel):
    import tuplewise.mmd as mm
    import tuplewise.mmd_var as mv
    X, Z = data("gauss", 530, 270, 5, 43)
    sigma = 2.0 if kernel == "gaussian" else None
    copies = [(X.copy(), Z.copy()) for _ in range(3)]
    np.random.seed(9)
    value, var = mv.UnN_var(*copies[0], 4, kernel=kernel, sigma=sigma)
    s0 = np.random.get_state()
    np.random.seed(9)
    o_value, o_var = o_UnN_var(*copies[1], 4, kernel, sigma)
    s1 = np.random.get_state()
    np.random.seed(9)
    un = mm.UnN(*copies[2], 4, kernel=kernel, sigma=sigma)
    scale = o_Un_scale(X, Z, kernel, sigma)
    assert abs(value - o_value) <= 1e-12 * scale and abs(value - un) <= 1e-12 * scale
    assert abs(var - o_var) <= 1e-9 * o_var
    assert same_state(s0, s1) and same_state(s0, np.random.get_state())
    for A, B in zip(copies[0], copies[1]):
        assert np.array_equal(A, B)
    for A, B in zip(copies[0], copies[2]):
        assert np.array_equal(A, B)


def test_select_sigma_matches_the_oracle(tw, gpu):
    import tuplewise.mmd_var as mv
    rng = np.random.RandomState(5)
    X, Z = rng.normal(size=(150, 3)), rng.normal(size=(140, 3))
    Z[:, 0] += 0.8  # the planted shift
    grid = list(np.geomspace(0.1, 30.0, 11))
    sel = mv.select_sigma(X, Z, grid)
    index, crit, value, var = o_select(X, Z, grid)
    print("criterion", sel.criterion, "oracle", crit)
    assert sel.index == index and sel.sigma == grid[index] and 0 < index < 10
    assert np.all(np.abs(sel.criterion - crit) <= 1e-9 * np.abs(crit))
    assert np.all(np.abs(sel.var - var) <= 1e-9 * var)
    # a grid longer than one launch splits without changing a number
    one = mv.Un_var(X, Z, sigma=grid[:8])
    assert np.array_equal(one.value, sel.value[:8]) and np.array_equal(one.var, sel.var[:8])


def test_median_inside_a_grid_is_its_number(tw, gpu):
    import tuplewise.bandwidth as bw
    import tuplewise.mmd_var as mv
    X, Z = data("gauss", 90, 70, 4, 17)
    med = float(bw.median_distance(X, Z, pairs="pooled"))
    a = mv.Un_var(X, Z, sigma=[0.5, "median", 4.0])
    b = mv.Un_var(X, Z, sigma=[0.5, med, 4.0])
    one = mv.Un_var(X, Z, sigma="median")
    for f in ("value", "var", "phi_x", "phi_z", "zeta_x", "zeta_z"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
        assert np.array_equal(getattr(a, f)[1], getattr(one, f)), f
    ra, rb = mv.row_sums(X, Z, sigma=("median", 2.0)), mv.row_sums(X, Z, sigma=(med, 2.0))
    assert all(np.array_equal(p, q) for p, q in zip(ra, rb))
    sel = mv.select_sigma(X, Z, ["median"])
    assert sel.sigma == med and sel.index == 0
