"""The pair function g of tuplewise.mmd, its permutation test and tuplewise.hsic on the device at
the edges of its range (tests/test_gpu_mmd.py, test_gpu_mmd_perm.py and test_gpu_hsic.py only
visit c * D in about [-4, 0] and D in about [0.01, 300]).

Single terms.  A block of n = 2, m = 2 makes Sxx and Szz of tw_mmd_sums one term each, a shard of
one quadruple makes the four outputs of tw_mmd_idx32 one term each, and tw_hsic_idx32 on one
4-tuple gives K_ij (the other side's factors exactly 1) or L_ij, L_qr, L_iq (K_ij exactly 1); sums
of one term and zeros, and products with 1.0, are exact.  The grids and the exact references are
those of tests/test_kernel_range_cpu.py:
  * Gaussian: every term within 4 ulp of the exact exp(fl(c * D)) — the bar DESIGN.md §4.3 grants
    the device exp — with the ulp of a subnormal or zero result 2^-1074, so a result flushed to
    zero in the subnormal range fails; exactly 1.0 where |c * D| < 2^-54; exactly 0.0 where the
    exact value rounds to 0 and at D = +inf; never NaN or negative.
  * energy: the bits of np.sqrt(D), which the CPU file shows to be the correctly rounded root, for
    D subnormal, near 2^-1022, ordinary, near 2^1023 and +inf.
  * one bit pattern per grid point from tw_mmd_sums, tw_mmd_idx32, tw_hsic_idx32 and (on a subset:
    one launch a point) column 0 of tw_mmd_perm_sums — csrc/mmdtile.h's "the same bits".

Sums.  All five entry points at data scales 1e-150, 1, 1e120 and mixed (1 and 1e3) with Gaussian
coefficients that put the median c * D at -1e-12, -1, -720 and -1e8, and the energy / distance
kernel, against the existing oracles at the existing tolerances (rtol 1e-12 for sums of
non-negative terms, atol 1e-12 * T for the permutation components).  This follows from the single
terms: a normal term is within 4 ulp, a subnormal one within 4 * 2^-1074, and every oracle sum
here is either exactly 0.0 (then the device's must be exactly 0.0) or above 1e-300, where some
1e4 subnormal terms' errors are below 1e-13 of it — the test asserts that premise.

Non-finite values: +inf coordinates, inf - inf = NaN differences and finite rows whose distance
overflows, at n = 5, m = 4 and n = 130, m = 131: NaN and +inf exactly where the NumPy oracles have
them; for the permutation kernel the contract of DESIGN.md §4.13 (a NaN or an overflowing distance
anywhere under the energy kernel makes every column NaN).

The public API at sigma = 0.02 and 1e6."""
import functools
import math

import numpy as np
import pytest

import test_gpu_hsic as TH
import test_hsic_cpu as HC
import test_mmd_cpu as MC
from test_gpu_mmd import GUARD, bits, mmd_data, raw_idx, raw_sums, sigma_of
from test_gpu_mmd_perm import labels_for, pack, raw_perm
from test_kernel_range_cpu import (E_REGIMES, G_REGIMES, arg_grid, energy_grid, gauss_arg,
                                   gauss_refs, rounded, subset, ulps)
from test_mmd_perm_cpu import o_perm_sums
from test_triplets_cpu import o_dist_rows

pytestmark = pytest.mark.gpu

RTOL = 1e-12
EXP_ULPS = 4.0  # the bar the project grants the device exp
FILL = np.array([0.5, -1.25, 3.0, 0.125, -7.0, 2.5, 1e-3, -40.0, 0.0])  # the d - 1 equal coordinates


@pytest.fixture(scope="module")
def mm(gpu):
    import tuplewise.mmd as m
    return m


@pytest.fixture(scope="module")
def hs(gpu):
    import tuplewise.hsic as h
    return h


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_mmd_tile())


# ------------------------------------------------- raw calls with the coefficient given directly
def _launch(tw, entry, args_before, args_after, nwork, nout):
    """One entry point on sentinel-filled d_work and d_out: the first nout doubles of d_out."""
    import torch
    L = tw._lib
    dev = args_before[0].device
    work = torch.full((nwork + GUARD,), -7.0, dtype=torch.float64, device=dev)
    out = torch.full((nout + GUARD,), -7.0, dtype=torch.float64, device=dev)
    L.call(entry, *args_before, *args_after, work, out, L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(-7.0)) and np.all(bits(out[nout:]) == bits(-7.0))
    return out[:nout]


def sums_c(tw, X, Z, bxo, bzo, kid, c):
    """tw_mmd_sums as tests/test_gpu_mmd.py's raw_sums calls it, with (kernel id, c) given."""
    L = tw._lib
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb, max_n, max_m = len(bxo) - 1, int(np.diff(bxo).max()), int(np.diff(bzo).max())
    dev = [L.to_device(np.ascontiguousarray(a).reshape(-1)) for a in (X, Z, bxo, bzo)]
    nwork = int(L.lib().tw_mmd_work_bytes(nb, max_n, max_m)) // 8
    return _launch(tw, "tw_mmd_sums", (dev[0], dev[1], X.shape[1], dev[2], dev[3]),
                   (nb, max_n, max_m, kid, c), nwork, 3 * nb).reshape(nb, 3)


def idx_c(tw, X, Z, i, j, k, l, off, kid, c):  # noqa: E741
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns, max_q = len(off) - 1, int(np.diff(off).max())
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    ix = [L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, k, l)]
    od = L.to_device(off)
    nwork = int(L.lib().tw_mmd_idx_work_bytes(ns, max_q)) // 8
    return _launch(tw, "tw_mmd_idx32", (xd, zd, X.shape[1], *ix, od), (ns, max_q, kid, c), nwork,
                   4 * ns).reshape(ns, 4)


def perm_c(tw, pool, labels, kid, c):
    L = tw._lib
    N, d = pool.shape
    P = labels.shape[0]
    wd = L.to_device(pool.reshape(-1))
    ld = L.to_device(pack(labels).view(np.int32).reshape(-1))
    nwork = int(L.lib().tw_mmd_perm_work_bytes(N, P)) // 8
    assert nwork > 0
    return _launch(tw, "tw_mmd_perm_sums", (wd, N, d, ld), (P, kid, c), nwork, 3 * P).reshape(P, 3)


def hsic_idx_c(tw, X, Y, i, j, q, r, off, kid, cx, cy):
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns, max_q = len(off) - 1, int(np.diff(off).max())
    xd, yd = L.to_device(X.reshape(-1)), L.to_device(Y.reshape(-1))
    ix = [L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, q, r)]
    od = L.to_device(off)
    nwork = int(L.lib().tw_hsic_idx_work_bytes(ns, max_q)) // 8
    return _launch(tw, "tw_hsic_idx32", (xd, X.shape[1], yd, Y.shape[1], *ix, od),
                   (ns, max_q, kid, cx, cy), nwork, 3 * ns).reshape(ns, 3)


def kid_of(tw, kernel):
    return tw._lib.TW_MMD_GAUSSIAN if kernel == "gaussian" else tw._lib.TW_MMD_ENERGY


def close_nf(got, want, what=None):
    """rtol 1e-12; NaN and +inf exactly where the oracle has them, and no -inf."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "got", got.reshape(-1).tolist()[:8], "want", want.reshape(-1).tolist()[:8])
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (what, got, want)
    assert not np.isneginf(got).any() and not np.isneginf(want).any(), (what, got, want)
    ok = np.isfinite(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), (what, got, want)


# --------------------------------------------------------------------------- single terms
def rows_of(v, d):
    """(len(v), d) rows: v in the last coordinate (the tail chunk at d = 9), the others equal
    across rows, so a pair's D is that of its last coordinates alone."""
    rows = np.tile(FILL[:d], (len(v), 1))
    rows[:, d - 1] = v
    return rows


@functools.lru_cache(maxsize=None)
def single_terms(tw, kernel, d):
    """Every grid point's single terms out of the reducing kernels, computed once: (G, 2) from
    tw_mmd_sums (Sxx, Szz), (G, 4) from tw_mmd_idx32, (G, 6) from tw_hsic_idx32 (A, B, C with the
    grid pair on the x side, then on the y side).  One launch per entry point and coefficient."""
    grid = arg_grid() if kernel == "gaussian" else energy_grid()
    G = len(grid["a"])
    kid = kid_of(tw, kernel)
    sums, idx, hsic = np.full((G, 2), -7.0), np.full((G, 4), -7.0), np.full((G, 6), -7.0)
    for c in np.unique(grid["c"]):
        at = np.flatnonzero(grid["c"] == c)
        g, c = len(at), float(c)
        a, b = grid["a"][at], grid["b"][at]
        pair = rows_of(np.stack([a, b], axis=1).reshape(-1), d)  # rows 2 p, 2 p + 1: point p
        two = 2 * np.arange(g + 1)
        s = sums_c(tw, pair, pair.copy(), two, two, kid, c)
        sums[at] = s[:, :2]
        p2 = 2 * np.arange(g)
        idx[at] = idx_c(tw, pair, pair.copy(), p2, p2 + 1, p2, p2 + 1, np.arange(g + 1), kid, c)
        # tw_hsic_idx32 on rows (4 p .. 4 p + 3), tuple (i, j, q, r) = (4 p, 4 p + 1, 4 p + 2, 4 p + 3).
        # The grid pair on one side, as (a, b, b, a): g_ij = g_qr = g_iq = g(a, b).  The other side
        # has factors of exactly 1: equal rows (Gaussian: exp(c * 0)) or the coordinates 0, 1, 1, 2
        # (distance: |0 - 1| = |1 - 2| = |0 - 1| = 1).
        quad = rows_of(np.stack([a, b, b, a], axis=1).reshape(-1), d)
        unit = rows_of(np.tile([0.0, 0.0, 0.0, 0.0] if kernel == "gaussian" else [0.0, 1.0, 1.0, 2.0], g), d)
        p4 = 4 * np.arange(g)
        off = np.arange(g + 1)
        hsic[at, :3] = hsic_idx_c(tw, quad, unit, p4, p4 + 1, p4 + 2, p4 + 3, off, kid, c, c)
        hsic[at, 3:] = hsic_idx_c(tw, unit, quad, p4, p4 + 1, p4 + 2, p4 + 3, off, kid, c, c)
    return sums, idx, hsic


def report(name, err, regime, regimes):
    worst = {r: float(np.max(err[regime == r])) for r in regimes}
    print(name, "max ulps per regime:", worst)
    return worst


@pytest.mark.parametrize("d", [1, 9])
def test_gaussian_single_terms(tw, d):
    grid, p, refs = arg_grid(), gauss_arg(arg_grid()), gauss_refs()
    want = np.array([rounded(e) for e in refs])
    sums, idx, hsic = single_terms(tw, "gaussian", d)
    for name, terms in (("tw_mmd_sums", sums), ("tw_mmd_idx32", idx), ("tw_hsic_idx32", hsic)):
        err = np.array([[ulps(v, e) for v in row] for row, e in zip(terms, refs)])
        report(f"exp d={d} {name}", err.max(axis=1), grid["regime"], G_REGIMES)
        assert not np.isnan(terms).any() and not np.signbit(terms).any(), name
        assert np.all(err <= EXP_ULPS), (name, np.argwhere(~(err <= EXP_ULPS))[:8])
        one, zero = np.abs(p) < 2.0 ** -54, (want == 0.0) | np.isinf(grid["D"])
        assert np.all(bits(terms[one]) == bits(1.0)), name
        assert np.all(bits(terms[zero]) == bits(0.0)), name


@pytest.mark.parametrize("d", [1, 9])
def test_energy_single_terms(tw, d):
    grid = energy_grid()
    want = np.sqrt(grid["D"])
    sums, idx, hsic = single_terms(tw, "energy", d)
    for name, terms in (("tw_mmd_sums", sums), ("tw_mmd_idx32", idx), ("tw_hsic_idx32", hsic)):
        away = np.abs(terms.view(np.int64) - want.view(np.int64)[:, None])  # ulps between the bit patterns
        report(f"sqrt d={d} {name}", away.max(axis=1), grid["regime"], E_REGIMES)
        assert np.array_equal(bits(terms), bits(np.repeat(want[:, None], terms.shape[1], axis=1))), name


@pytest.mark.parametrize("d", [1, 9])
@pytest.mark.parametrize("kernel", ["gaussian", "energy"])
def test_same_bits_across_translation_units(tw, kernel, d):
    """mmd.hip (both kernels), hsic.hip and mmd_perm.hip give one bit pattern per grid point."""
    grid = arg_grid() if kernel == "gaussian" else energy_grid()
    sums, idx, hsic = single_terms(tw, kernel, d)
    ref = bits(sums[:, 0])
    for name, terms in (("tw_mmd_sums", sums), ("tw_mmd_idx32", idx), ("tw_hsic_idx32", hsic)):
        for k in range(terms.shape[1]):
            assert np.array_equal(bits(terms[:, k]), ref), (name, k, np.flatnonzero(bits(terms[:, k]) != ref)[:8])
    # the permutation kernel: N = 4, labels 1, 1, 0, 0, so Sxx is the single term g(w0, w1).  The
    # other two rows repeat the pair where it is finite (g(w0, w2) = g(0)) and are two finite
    # points where it is not (inf - inf would be a NaN, which fills every column).
    kid = kid_of(tw, kernel)
    labels = np.array([[True, True, False, False]])
    at = subset(grid, G_REGIMES if kernel == "gaussian" else E_REGIMES)
    assert len(at) == 4 * len(G_REGIMES if kernel == "gaussian" else E_REGIMES)
    for p in at:
        a, b = grid["a"][p], grid["b"][p]
        rest = [a, b] if np.isfinite(a) and np.isfinite(b) else [0.25, 1.75]
        got = perm_c(tw, rows_of(np.array([a, b] + rest), d), labels, kid, float(grid["c"][p]))[0]
        if kernel == "energy" and np.isinf(grid["D"][p]):
            assert np.isnan(got).all(), (p, got)  # the contract of DESIGN.md §4.13
        else:
            assert bits(got[0])[0] == ref[p], (kernel, d, p, grid["regime"][p], got, sums[p])


# --------------------------------------------------------------- sums over a wide range
SCALES = {"1e-150": 1e-150, "1": 1.0, "1e120": 1e120, "mixed": None}
TARGETS = {"g-1e-12": -1e-12, "g-1": -1.0, "g-720": -720.0, "g-under": -1e8, "energy": None}


def scaled(A, scale):
    """A times the scale; "mixed": the odd rows times 1e3."""
    A = A.copy()
    if scale is None:
        A[1::2] *= 1e3
        return A
    return A * scale


def sigma_for(D, target):
    """sigma with -1 / (2 sigma^2) * median(D) close to the target (D: squared distances > 0)."""
    c = target / float(np.median(D[D > 0.0]))
    sigma = math.sqrt(-1.0 / (2.0 * c))
    assert math.isfinite(MC.o_coef("gaussian", sigma)) and 2.0 * sigma * sigma > 0.0
    return sigma


def premise(want):
    """Every oracle sum is exactly 0.0 or large enough for its subnormal terms not to matter."""
    w = np.asarray(want, dtype=np.float64).reshape(-1)
    assert np.all((w == 0.0) | (w > 1e-300)) and np.isfinite(w).all(), w


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("scale", list(SCALES))
def test_mmd_sums_over_a_wide_range(tw, tile, scale, target):
    d, n, m = 3, 65, tile + 1
    X, Z = mmd_data("gauss", n, m, d, 11)
    X, Z = scaled(X, SCALES[scale]), scaled(Z, SCALES[scale])
    kernel = "energy" if target == "energy" else "gaussian"
    sigma = sigma_for(o_dist_rows(X, Z), TARGETS[target]) if kernel == "gaussian" else None
    kid, c = kid_of(tw, kernel), (MC.o_coef(kernel, sigma) if kernel == "gaussian" else 0.0)
    # tw_mmd_sums
    want = MC.o_components(X, Z, kernel, sigma)
    premise(want)
    if target == "g-under" and scale != "mixed":
        assert want == (0.0, 0.0, 0.0)  # every term underflows
    close_nf(sums_c(tw, X, Z, [0, n], [0, m], kid, c)[0], want, ("sums", scale, target))
    # tw_mmd_idx32: shards of 300, 0 and 150 quadruples (at a median c * D of -720 a single
    # term is as likely subnormal as not, and the premise is about sums)
    rng = np.random.RandomState(5)
    off = np.array([0, 300, 300, 450])
    T = int(off[-1])
    i, k = rng.randint(0, n, T), rng.randint(0, m, T)
    j, l = rng.randint(0, n - 1, T), rng.randint(0, m - 1, T)  # noqa: E741
    j += j >= i
    l += l >= k  # noqa: E741
    got = idx_c(tw, X, Z, i, j, k, l, off, kid, c)
    for s, (a, b) in enumerate(zip(off, off[1:])):
        w = MC.o_idx_sums(X, Z, i[a:b], j[a:b], k[a:b], l[a:b], kernel, sigma)
        premise(w)
        close_nf(got[s], w, ("idx", scale, target, s))
    # tw_mmd_perm_sums: 17 columns at atol 1e-12 * T
    labels = labels_for(17, n, n + m, 9)
    want = o_perm_sums(X, Z, labels, kernel, sigma)
    premise(want)
    tol = RTOL * math.fsum(want[0])
    got = perm_c(tw, np.concatenate([X, Z]), labels, kid, c)
    err = np.abs(got - want).max()
    print("perm", scale, target, "max |diff|", err, "tol", tol)
    assert np.isfinite(got).all() and err <= tol
    if tol == 0.0:
        assert np.all(bits(got) == bits(0.0))


@pytest.mark.parametrize("target", list(TARGETS))
@pytest.mark.parametrize("scale", list(SCALES))
def test_hsic_sums_over_a_wide_range(tw, tile, scale, target):
    dx, dy, n = 3, 2, tile + 1
    X, Y = HC.paired(n, dx, dy, 12)
    X, Y = scaled(X, SCALES[scale]), scaled(Y, SCALES[scale])
    kernel = "distance" if target == "energy" else "gaussian"
    if kernel == "gaussian":
        sigma = (sigma_for(o_dist_rows(X, X), TARGETS[target]), sigma_for(o_dist_rows(Y, Y), TARGETS[target]))
        coefs = (tw._lib.TW_HSIC_GAUSSIAN, MC.o_coef(kernel, sigma[0]), MC.o_coef(kernel, sigma[1]))
    else:
        sigma, coefs = None, (tw._lib.TW_HSIC_DISTANCE, 0.0, 0.0)
    want, want_rows = HC.o_components(X, Y, kernel, sigma), HC.o_row_sums(X, Y, kernel, sigma)
    premise(want)
    premise(want_rows)
    if target == "g-under" and scale != "mixed":
        assert want == (0.0,) * 8 and not np.any(want_rows)
    got, rows = TH.raw_sums(tw, X, Y, [0, n], kernel, coefs=coefs)
    close_nf(got[0], want, ("hsic sums", scale, target))
    close_nf(rows[:, 0], want_rows[0], "k")
    close_nf(rows[:, 1], want_rows[1], "l")
    np.random.seed(6)
    off = np.array([0, 300, 300, 450])
    t = HC.o_draw(n, int(off[-1]))
    got = hsic_idx_c(tw, X, Y, *t, off, *coefs)
    for s, (a, b) in enumerate(zip(off, off[1:])):
        w = HC.o_idx_sums(X, Y, *(v[a:b] for v in t), kernel, sigma)
        premise(w)
        close_nf(got[s], w, ("hsic idx", scale, target, s))


# ------------------------------------------------------------------------- non-finite values
SIZES = [(5, 4), (130, 131)]
CASES = ["inf", "infinf-x", "infinf-xz", "big"]


def spoil(X, Z, case):
    """One +inf coordinate in X; +inf in the same coordinate of two rows of X, or of a row of X
    and a row of Z (their difference is NaN); one row of Z at 1e200 (finite, D overflows)."""
    X, Z = X.copy(), Z.copy()
    n, m = len(X), len(Z)
    if case == "inf":
        X[n // 3, 2] = np.inf
    elif case == "infinf-x":
        X[1, 2] = X[n - 1, 2] = np.inf
    elif case == "infinf-xz":
        X[n // 3, 2] = Z[m // 3, 2] = np.inf
    else:
        Z[m // 2] = 1e200
    return X, Z


@pytest.mark.parametrize("kernel", MC.KERNELS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n,m", SIZES)
def test_mmd_non_finite(tw, n, m, case, kernel):
    d = 5
    X, Z = spoil(*mmd_data("gauss", n, m, d, 3), case)
    sigma = sigma_of(kernel, d)
    want = np.array(MC.o_components(X, Z, kernel, sigma))
    inf, nan = np.inf, np.nan
    if kernel == "energy":  # what the oracle holds, spelled out: sqrt(inf) = inf, inf + nan = nan
        shape = {"inf": [inf, 1, inf], "infinf-x": [nan, 1, inf], "infinf-xz": [inf, inf, nan], "big": [1, inf, inf]}
    else:                   # exp(c * inf) = 0: finite unless a difference is inf - inf
        shape = {"inf": [1, 1, 1], "infinf-x": [nan, 1, 1], "infinf-xz": [1, 1, nan], "big": [1, 1, 1]}
    for w, s in zip(want, shape[case]):
        assert (np.isnan(w) and np.isnan(s)) or (w == inf and s == inf) or (np.isfinite(w) and s == 1), (want, case)
    close_nf(raw_sums(tw, X, Z, [0, n], [0, m], kernel)[0], want, (n, m, case, kernel))
    # tw_mmd_idx32: shard 0 is one quadruple of clean rows, the others are drawn
    rng = np.random.RandomState(4)
    off = np.array([0, 1, 4, 261, 272])
    T = int(off[-1])
    i, k = rng.randint(0, n, T), rng.randint(0, m, T)
    j, l = rng.randint(0, n - 1, T), rng.randint(0, m - 1, T)  # noqa: E741
    j += j >= i
    l += l >= k  # noqa: E741
    i[0], j[0], k[0], l[0] = 0, 2, 0, 3
    # and the last shard's last two quadruples hold the spoiled rows, the last one the NaN pair
    i[-2:], j[-2:], k[-2:], l[-2:] = {"inf": ([n // 3, 0], [0, n // 3], [0, 1], [3, 0]),
                                      "infinf-x": ([1, 1], [0, n - 1], [0, 0], [3, 3]),
                                      "infinf-xz": ([n // 3, n // 3], [0, 0], [m // 3, 0], [0, m // 3]),
                                      "big": ([0, 2], [2, 0], [m // 2, 0], [0, m // 2])}[case]
    got = raw_idx(tw, X, Z, i, j, k, l, off, kernel)
    assert np.isfinite(got[0]).all()
    seen = set()
    for s, (a, b) in enumerate(zip(off, off[1:])):
        w = np.array(MC.o_idx_sums(X, Z, i[a:b], j[a:b], k[a:b], l[a:b], kernel, sigma))
        seen |= {"nan"} if np.isnan(w).any() else set()
        seen |= {"inf"} if np.isinf(w).any() else set()
        close_nf(got[s], w, (n, m, case, kernel, s))
    assert ("inf" in seen) == (kernel == "energy") or case == "infinf-x" and n == 5
    assert ("nan" in seen) == case.startswith("infinf")


@pytest.mark.parametrize("kernel", HC.KERNELS)
@pytest.mark.parametrize("case", ["inf", "infinf", "big"])
@pytest.mark.parametrize("n", [5, 130])
def test_hsic_non_finite(tw, n, case, kernel):
    """The spoiled row r of X has K_rj = +inf (distance) or 0 (Gaussian) against every j; Y[0]
    duplicates Y[r], so the distance kernel's S_KL holds 0 * inf = NaN, as the oracle's does."""
    dx = dy = 5
    X, Y = HC.paired(n, dx, dy, 3)
    r = {"inf": n // 3, "infinf": 1, "big": n // 2}[case]
    if case == "inf":
        X[r, 2] = np.inf
    elif case == "infinf":
        X[r, 2] = X[n - 1, 2] = np.inf
    else:
        X[r] = 1e200
    Y[0] = Y[r]
    s = HC.sig(kernel, dx, dy)
    want, want_rows = np.array(HC.o_components(X, Y, kernel, s)), HC.o_row_sums(X, Y, kernel, s)
    if kernel == "distance":
        assert np.isnan(want[0]) and np.isfinite(want[[2, 4, 7]]).all()  # S_KL; S_LL, R_L, R_LL
        assert not np.isfinite(want[[1, 3, 5, 6]]).any() and not np.isfinite(want_rows[0]).any()
        if case != "infinf":
            assert np.all(want[[1, 3, 5, 6]] == np.inf) and np.all(want_rows[0] == np.inf)
    else:
        assert np.isfinite(want).all() == (case != "infinf")
    got, rows = TH.raw_sums(tw, X, Y, [0, n], kernel)
    close_nf(got[0], want, (n, case, kernel))
    close_nf(rows[:, 0], want_rows[0], "k")
    close_nf(rows[:, 1], want_rows[1], "l")
    np.random.seed(9)
    off = np.array([0, 1, 4, 261, 272])
    t = HC.o_draw(n, int(off[-1]))
    got = TH.raw_idx(tw, X, Y, *t, off, kernel)
    for sh, (a, b) in enumerate(zip(off, off[1:])):
        close_nf(got[sh], HC.o_idx_sums(X, Y, *(v[a:b] for v in t), kernel, s), (n, case, kernel, sh))


@pytest.mark.parametrize("kernel", MC.KERNELS)
@pytest.mark.parametrize("case", ["inf", "infinf", "big"])
@pytest.mark.parametrize("n,m,where", [(5, 4, 0), (5, 4, 7), (130, 131, 3), (130, 131, 200)])
def test_permutation_non_finite(tw, mm, n, m, where, case, kernel):
    """Gaussian: a pair with D = +inf is a term of exactly 0 and the columns match the oracle.
    Energy: a pair with g = +inf makes every column's three sums NaN (0 * inf on the matrix unit,
    inf - inf in the reduce), as a NaN does under either kernel; permutation_test then returns a
    NaN statistic, an all-NaN null and the p-value 1 / (n_perm + 1)."""
    d = 5
    X, Z = mmd_data("gauss", n, m, d, 3)
    pool = np.concatenate([X, Z])
    if case == "big":
        pool[where] = 1e200
    else:
        pool[where, 2] = np.inf
        if case == "infinf":
            pool[(where + 2) % (n + m), 2] = np.inf
    X, Z = pool[:n], pool[n:]
    labels = labels_for(17, n, n + m, 8)
    got = raw_perm(tw, X, Z, labels, kernel)
    np.random.seed(4)
    res = mm.permutation_test(X, Z, 20, kernel, sigma_of(kernel, d))
    if kernel == "gaussian" and case != "infinf":
        want = o_perm_sums(X, Z, labels, kernel, sigma_of(kernel, d))
        assert np.isfinite(want).all()
        err, tol = np.abs(got - want).max(), RTOL * math.fsum(want[0])
        print(n, m, where, case, "max |diff|", err, "tol", tol)
        assert err <= tol
        assert np.isfinite(res.statistic) and np.isfinite(res.null).all() and 1 / 21 <= res.pvalue <= 1.0
    else:
        assert np.isnan(got).all(), got
        assert np.isnan(res.statistic) and np.isnan(res.null).all() and res.pvalue == 1 / 21


# --------------------------------------------------------------- the public API at extreme sigma
@pytest.mark.parametrize("sigma", [0.02, 1e6])
def test_public_mmd_at_extreme_sigma(mm, tile, sigma):
    X, Z = mmd_data("gauss", 65, tile + 1, 3, 13)
    got, want, scale = mm.Un(X, Z, "gaussian", sigma), MC.o_Un(X, Z, "gaussian", sigma), MC.o_Un_scale(X, Z, "gaussian", sigma)
    print("Un", sigma, got, want, "tol", RTOL * scale)
    assert isinstance(got, np.float64) and abs(got - want) <= RTOL * scale
    labels = labels_for(17, 65, 65 + tile + 1, 2)
    want = o_perm_sums(X, Z, labels, "gaussian", sigma)
    got = mm.permutation_sums(X, Z, labels, "gaussian", sigma)
    err, tol = np.abs(got - want).max(), RTOL * math.fsum(want[0])
    print("permutation_sums", sigma, "max |diff|", err, "tol", tol)
    assert err <= tol


@pytest.mark.parametrize("sigma", [0.02, 1e6])
def test_public_hsic_at_extreme_sigma(hs, sigma):
    """Un at its scale-based atol.  correlation divides by sqrt(vxx * vyy): at sigma = 0.02 the
    off-diagonal K and L are tiny or 0 but the three statistics do not cancel, so the value (or the
    NaN of a product that is not > 0) must match the oracle's at the tolerance propagated from the
    three atols.  At sigma = 1e6 K = 1 - O(1e-12) and the statistics, of true size 1e-24 of their
    parts, are rounding noise on both sides: there the denominators' handling is pinned against the
    device's own components — NaN exactly when their product is not > 0 — and the comparison with
    the oracle's value is made only if the oracle's vxx and vyy exceed their own atols."""
    X, Y = HC.paired(150, 4, 3, 31)
    n = len(X)
    (vxy, sxy), (vxx, sxx), (vyy, syy) = HC.o_three(X, Y, "gaussian", sigma)
    got = hs.Un(X, Y, "gaussian", sigma)
    print("Un", sigma, got, vxy, "tol", RTOL * sxy)
    assert isinstance(got, np.float64) and abs(got - vxy) <= RTOL * sxy
    # the three statistics from the device's sums, each at its atol
    c = hs.components(X, Y, "gaussian", sigma)
    dev = (HC.o_U(c[0], c[3], c[4], c[5], n), HC.o_U(c[1], c[3], c[3], c[6], n), HC.o_U(c[2], c[4], c[4], c[7], n))
    for g, w, sc in zip(dev, (vxy, vxx, vyy), (sxy, sxx, syy)):
        assert abs(g - w) <= RTOL * sc, (g, w, sc)
    got = hs.correlation(X, Y, "gaussian", sigma)
    own = dev[0] / math.sqrt(dev[1] * dev[2]) if dev[1] * dev[2] > 0.0 else float("nan")
    print("correlation", sigma, got, "from the device's sums", own, "oracle", HC.o_correlation(X, Y, "gaussian", sigma))
    assert isinstance(got, np.float64)
    assert (np.isnan(got) and np.isnan(own)) or got == own
    resolved = vxx > 2.0 * RTOL * sxx and vyy > 2.0 * RTOL * syy
    assert resolved == (sigma == 0.02)
    if resolved:
        want = HC.o_correlation(X, Y, "gaussian", sigma)
        assert not np.isnan(want) and not np.isnan(got)
        tol = abs(want) * RTOL * (sxy / abs(vxy) + sxx / (2.0 * abs(vxx)) + syy / (2.0 * abs(vyy)))
        assert abs(got - want) <= tol, (got, want, tol)
    # a side whose off-diagonal terms all underflow has no variance to normalise by: NaN, as the
    # oracle's (vxx = 0 exactly on both sides)
    far = X * 1e3
    assert HC.o_three(far, Y, "gaussian", 0.02)[1][0] == 0.0
    assert np.isnan(HC.o_correlation(far, Y, "gaussian", 0.02))
    assert np.isnan(hs.correlation(far, Y, "gaussian", 0.02))
