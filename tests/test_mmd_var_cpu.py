"""tuplewise.mmd_var without a GPU: the NumPy oracle the GPU tests compare against (the row sums
by math.fsum over the terms of tests/test_mmd_cpu.py's oracle, the variance restated from the
module's docstring), the oracle against a brute-force double loop, against o_Un / o_components
and against the empirical variance over replications, every argument error before any device work
or RNG draw, the native entry's argument checks, and — with the device glue stubbed to the oracle
— select_sigma's rules and UnN_var against mmd.UnN."""
import ctypes
import math

import numpy as np
import pytest

from test_mmd_cpu import KERNELS, brute_g, o_Un, o_components, o_fsum, o_g, o_sign
from test_triplets_cpu import data, o_dist_rows, same_state


# ------------------------------------------------------------------------------------ oracle
def o_terms(X, Z, kernel, sigma=None):
    """The terms of the four row sums: (gxx without its diagonal (n, n - 1), gxz (n, m), gzz without
    its diagonal (m, m - 1))."""
    n, m = len(X), len(Z)
    gxx, gzz = o_g(o_dist_rows(X, X), kernel, sigma), o_g(o_dist_rows(Z, Z), kernel, sigma)
    gxz = o_g(o_dist_rows(X, Z), kernel, sigma)
    return (gxx[~np.eye(n, dtype=bool)].reshape(n, n - 1), gxz,
            gzz[~np.eye(m, dtype=bool)].reshape(m, m - 1))


def o_row_sums(X, Z, kernel, sigma=None):
    """(a, r, q, b): a_i = sum_{j != i} g(x_i, x_j), r_i = sum_k g(x_i, z_k), q_k = sum_i g(x_i,
    z_k), b_k = sum_{l != k} g(z_k, z_l), each by math.fsum."""
    gxx, gxz, gzz = o_terms(X, Z, kernel, sigma)
    return (np.array([o_fsum(t) for t in gxx]), np.array([o_fsum(t) for t in gxz]),
            np.array([o_fsum(t) for t in gxz.T]), np.array([o_fsum(t) for t in gzz]))


def o_row_scales(X, Z, kernel, sigma=None):
    """The rows' sums of |terms| (g >= 0: the sums themselves, NaN rows as 0)."""
    return tuple(np.nan_to_num(v, nan=0.0) for v in o_row_sums(X, Z, kernel, sigma))


def o_var_of_rows(a, r, q, b, kernel):
    """(value, var, phi_x, phi_z, zeta_x, zeta_z) from the row sums, as the module states it."""
    n, m = len(a), len(b)
    sign = o_sign(kernel)
    with np.errstate(invalid="ignore"):
        phi_x = sign * (a / (n - 1) - r / m)
        phi_z = sign * (b / (m - 1) - q / n)
        zeta_x, zeta_z = np.var(phi_x, ddof=1), np.var(phi_z, ddof=1)
        return (np.float64(np.mean(phi_x) + np.mean(phi_z)),
                np.float64(4.0 * zeta_x / n + 4.0 * zeta_z / m), phi_x, phi_z, zeta_x, zeta_z)


def o_Un_var(X, Z, kernel, sigma=None):
    return o_var_of_rows(*o_row_sums(X, Z, kernel, sigma), kernel)


def o_UnN_var(X, Z, N, kernel, sigma=None):
    """mmd.UnN's shuffles and blocks; (mean of the blocks' values, mean of their var / N)."""
    np.random.shuffle(X)
    np.random.shuffle(Z)
    k, kz = int(X.shape[0] / N), int(Z.shape[0] / N)
    v = [o_Un_var(X[b * k:(b + 1) * k], Z[b * kz:(b + 1) * kz], kernel, sigma) for b in range(N)]
    return np.mean([t[0] for t in v]), np.mean([t[1] for t in v]) / N


def o_select(X, Z, sigmas, reg=1e-8):
    """(index, criterion, value, var) of the grid."""
    v = [o_Un_var(X, Z, "gaussian", s) for s in sigmas]
    value, var = np.array([t[0] for t in v]), np.array([t[1] for t in v])
    crit = value / np.sqrt(np.maximum(var, 0.0) + reg)
    return int(np.nanargmax(crit)), crit, value, var


def fake_rows_blocks(calls=None):
    """The device glue mmd_var._rows_blocks restated on the oracle (Gaussian: sigma from c)."""
    def rows_blocks(Xf, Zf, bxo, bzo, kid, cs):
        if calls is not None:
            calls.append(len(cs))
        kernel = KERNELS[kid]
        rx = np.full((len(cs), int(bxo[-1]), 2), -7.0)
        rz = np.full((len(cs), int(bzo[-1]), 2), -7.0)
        for s, c in enumerate(cs):
            for b in range(len(bxo) - 1):
                x, z = Xf[bxo[b]:bxo[b + 1]], Zf[bzo[b]:bzo[b + 1]]
                if kernel == "gaussian":  # exp(D * c) with the module's own c, not a rebuilt sigma
                    with np.errstate(invalid="ignore"):
                        gxx, gxz, gzz = (np.exp(o_dist_rows(x, x) * c), np.exp(o_dist_rows(x, z) * c),
                                         np.exp(o_dist_rows(z, z) * c))
                else:
                    gxx, gxz, gzz = (o_g(o_dist_rows(x, x), kernel, None),
                                     o_g(o_dist_rows(x, z), kernel, None),
                                     o_g(o_dist_rows(z, z), kernel, None))
                np.fill_diagonal(gxx, 0.0)
                np.fill_diagonal(gzz, 0.0)
                rx[s, bxo[b]:bxo[b + 1], 0] = [o_fsum(t) for t in gxx]
                rx[s, bxo[b]:bxo[b + 1], 1] = [o_fsum(t) for t in gxz]
                rz[s, bzo[b]:bzo[b + 1], 0] = [o_fsum(t) for t in gxz.T]
                rz[s, bzo[b]:bzo[b + 1], 1] = [o_fsum(t) for t in gzz]
        return rx, rz
    return rows_blocks


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [1, 3])
def test_oracle_is_the_double_loop(kernel, d):
    n, m = 5, 4
    X, Z = data("gauss", n, m, d, 3)
    sigma = 1.3 if kernel == "gaussian" else None
    a = [math.fsum(brute_g(X[i], X[j], kernel, sigma) for j in range(n) if j != i) for i in range(n)]
    r = [math.fsum(brute_g(X[i], Z[k], kernel, sigma) for k in range(m)) for i in range(n)]
    q = [math.fsum(brute_g(X[i], Z[k], kernel, sigma) for i in range(n)) for k in range(m)]
    b = [math.fsum(brute_g(Z[k], Z[l], kernel, sigma) for l in range(m) if l != k) for k in range(m)]
    got = o_row_sums(X, Z, kernel, sigma)
    # math.exp and np.exp may differ in the last bit of a term; sqrt is exact on both sides
    for g, w in zip(got, (a, r, q, b)):
        assert np.allclose(g, w, rtol=1e-14 if kernel == "gaussian" else 0, atol=0)
    # the variance, spelled out
    value, var, phi_x, phi_z, zeta_x, zeta_z = o_Un_var(X, Z, kernel, sigma)
    sign = o_sign(kernel)
    px = [sign * (got[0][i] / (n - 1) - got[1][i] / m) for i in range(n)]
    pz = [sign * (got[3][k] / (m - 1) - got[2][k] / n) for k in range(m)]
    zx = sum((p - sum(px) / n) ** 2 for p in px) / (n - 1)
    zz = sum((p - sum(pz) / m) ** 2 for p in pz) / (m - 1)
    assert np.allclose(phi_x, px, rtol=0, atol=1e-15) and np.allclose(phi_z, pz, rtol=0, atol=1e-15)
    assert abs(zeta_x - zx) <= 1e-14 * zx and abs(zeta_z - zz) <= 1e-14 * zz
    assert abs(var - (4 * zx / n + 4 * zz / m)) <= 1e-14 * var


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n,m,d", [(2, 2, 1), (7, 5, 3), (23, 31, 8)])
def test_oracle_value_is_o_Un_and_the_sums_are_the_components(kernel, n, m, d):
    X, Z = data("gauss", n, m, d, 4)
    sigma = math.sqrt(d) if kernel == "gaussian" else None
    a, r, q, b = o_row_sums(X, Z, kernel, sigma)
    value = o_Un_var(X, Z, kernel, sigma)[0]
    assert abs(value - o_Un(X, Z, kernel, sigma)) <= 1e-13
    sxx, szz, sxz = o_components(X, Z, kernel, sigma)
    tol = 1e-14
    assert abs(o_fsum(a) - 2.0 * sxx) <= tol * sxx and abs(o_fsum(b) - 2.0 * szz) <= tol * szz
    assert abs(o_fsum(r) - sxz) <= tol * sxz and abs(o_fsum(q) - sxz) <= tol * sxz


def np_Un_var(X, Z, sigma):
    """(value, var) of the Gaussian kernel by plain NumPy sums (the Monte Carlo's restatement)."""
    c = -1.0 / (2.0 * sigma * sigma)

    def gram(A, B):
        sq = (A * A).sum(1)[:, None] + (B * B).sum(1)[None, :] - 2.0 * A @ B.T
        return np.exp(np.maximum(sq, 0.0) * c)

    n, m = len(X), len(Z)
    gxx, gzz, gxz = gram(X, X), gram(Z, Z), gram(X, Z)
    np.fill_diagonal(gxx, 0.0)
    np.fill_diagonal(gzz, 0.0)
    phi_x = gxx.sum(1) / (n - 1) - gxz.sum(1) / m
    phi_z = gzz.sum(1) / (m - 1) - gxz.sum(0) / n
    return (phi_x.mean() + phi_z.mean(),
            4.0 * np.var(phi_x, ddof=1) / n + 4.0 * np.var(phi_z, ddof=1) / m)


def test_restatement_is_the_oracle():
    X, Z = data("gauss", 40, 30, 2, 9)
    value, var = np_Un_var(X, Z, 1.0)
    want = o_Un_var(X, Z, "gaussian", 1.0)
    assert abs(value - want[0]) <= 1e-12 and abs(var - want[1]) <= 1e-9 * want[1]


@pytest.mark.parametrize("n,m,shift", [(200, 300, 1.0), (150, 150, 0.5), (300, 100, 2.0)])
def test_var_estimates_the_variance_of_the_value(n, m, shift):
    """Away from the null the first-order term carries the variance: over 600 replications the
    mean of var lies within 0.8 - 1.25 of the empirical variance of the value."""
    rng = np.random.RandomState(1234)
    out = np.array([np_Un_var(rng.normal(size=(n, 2)), rng.normal(size=(m, 2)) + shift, 1.0)
                    for _ in range(600)])
    ratio = out[:, 1].mean() / np.var(out[:, 0], ddof=1)
    print(f"n={n} m={m} shift={shift}: mean(var) / var(value) = {ratio:.3f}")
    assert 0.8 <= ratio <= 1.25


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.mmd_var as mv
    for name in ("row_sums", "Un_var", "UnN_var", "select_sigma"):
        assert callable(getattr(mv, name)), name
    assert mv.RowSums._fields == ("a", "r", "q", "b")
    assert mv.MMDVariance._fields == ("value", "var", "phi_x", "phi_z", "zeta_x", "zeta_z")
    assert mv.SigmaSelection._fields == ("sigma", "index", "criterion", "value", "var")


def test_argument_errors_need_no_device(tw, monkeypatch):
    import tuplewise.mmd_var as mv
    L = tw._lib

    def no_device(*a, **k):
        raise AssertionError("device work before the argument checks were done")

    for name in ("call", "to_device_many", "to_device", "empty", "device"):
        monkeypatch.setattr(L, name, no_device)
    X, Z = np.arange(40.0).reshape(10, 4), np.arange(24.0).reshape(6, 4) + 0.5
    X0, Z0 = X.copy(), Z.copy()
    x1 = np.arange(10.0)
    wide = np.zeros((4, 65))
    E = dict(kernel="energy")
    G = dict(sigma=1.0)
    nan, inf = float("nan"), float("inf")
    state = np.random.get_state()

    def refused(fn):
        return [
            # everything mmd.Un refuses: dtype, layout, rank
            lambda: fn(X.astype(np.float32), Z, **E), lambda: fn(X, Z.astype(np.int64), **G),
            lambda: fn(X[:, ::2], Z[:, ::2], **E), lambda: fn(X.T, Z.T, **G),
            lambda: fn(X.reshape(5, 2, 4), Z, **E), lambda: fn(x1[::2], x1, **E),
            # d: a mismatch, above 64, none
            lambda: fn(X, x1, **E), lambda: fn(wide, wide, **G),
            lambda: fn(np.zeros((4, 0)), np.zeros((3, 0)), **E),
            # too few rows
            lambda: fn(X[:1], Z, **E), lambda: fn(X, Z[:1], **G), lambda: fn(X[:0], Z, **E),
            # the kernel and its sigma
            lambda: fn(X, Z, kernel="laplace", sigma=1.0), lambda: fn(X, Z, kernel=None),
            lambda: fn(X, Z), lambda: fn(X, Z, kernel="gaussian"), lambda: fn(X, Z, sigma=0.0),
            lambda: fn(X, Z, sigma=-1.0), lambda: fn(X, Z, sigma=nan), lambda: fn(X, Z, sigma=inf),
            lambda: fn(X, Z, sigma="wide"), lambda: fn(X, Z, sigma=1e-200),
            lambda: fn(X, Z, kernel="energy", sigma=1.0),
            # grids: empty, a bad entry, the energy kernel
            lambda: fn(X, Z, sigma=[]), lambda: fn(X, Z, sigma=()), lambda: fn(X, Z, sigma=np.zeros(0)),
            lambda: fn(X, Z, sigma=[1.0, 0.0]), lambda: fn(X, Z, sigma=[1.0, -2.0, 3.0]),
            lambda: fn(X, Z, sigma=[nan]), lambda: fn(X, Z, sigma=(1.0, inf)),
            lambda: fn(X, Z, sigma=[1.0, "wide"]), lambda: fn(X, Z, sigma=[1.0, None]),
            lambda: fn(X, Z, sigma=np.ones((2, 2))), lambda: fn(X, Z, kernel="energy", sigma=[1.0]),
            lambda: fn(X, Z, kernel="energy", sigma=[]), lambda: fn(X, Z, kernel="x", sigma=[1.0]),
        ]

    calls = refused(mv.row_sums) + refused(mv.Un_var) + refused(
        lambda X, Z, **k: mv.UnN_var(X, Z, 2, **k))
    calls += [
        # the block estimator: partitions out of scope, short blocks, lists, a grid
        lambda: mv.UnN_var(X, Z, 2, "SWOR", **E), lambda: mv.UnN_var(X, Z, 2, "prop-SWR", **G),
        lambda: mv.UnN_var(X, Z, 6, **E), lambda: mv.UnN_var(X, Z, 4, **G),
        lambda: mv.UnN_var(X.tolist(), Z, 2, **G), lambda: mv.UnN_var(X, Z.tolist(), 2, **E),
        lambda: mv.UnN_var(X, Z, 2, sigma=[1.0, 2.0]),
        # select_sigma: the energy kernel, no grid, reg
        lambda: mv.select_sigma(X, Z, [1.0], kernel="energy"), lambda: mv.select_sigma(X, Z, 1.0),
        lambda: mv.select_sigma(X, Z, []), lambda: mv.select_sigma(X, Z, [1.0, 0.0]),
        lambda: mv.select_sigma(X, Z, [1.0], reg=-1e-9), lambda: mv.select_sigma(X, Z, [1.0], reg=nan),
        lambda: mv.select_sigma(X, Z, [1.0], reg=inf), lambda: mv.select_sigma(X, Z, [1.0], reg="x"),
        lambda: mv.select_sigma(X[:1], Z, [1.0]), lambda: mv.select_sigma(X, Z.astype(np.float32), [1.0]),
    ]
    for n, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
        assert same_state(np.random.get_state(), state), n
    with pytest.raises(ValueError, match="empty"):
        mv.Un_var(X, Z, sigma=[])
    with pytest.raises(ValueError, match="no sigma"):
        mv.Un_var(X, Z, kernel="energy", sigma=[1.0])
    with pytest.raises(ValueError, match="Gaussian kernel only"):
        mv.select_sigma(X, Z, [1.0], kernel="energy")
    with pytest.raises(ValueError, match="reg"):
        mv.select_sigma(X, Z, [1.0], reg=-1.0)
    assert np.array_equal(X, X0) and np.array_equal(Z, Z0)
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.mmd_var as mv
    X, Z = data("gauss", 6, 4, 3, 0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        mv.row_sums(X, Z, sigma=1.0)
    with pytest.raises(RuntimeError, match="no HIP device"):
        mv.Un_var(X, Z, kernel="energy")
    with pytest.raises(RuntimeError, match="no HIP device"):
        mv.select_sigma(X, Z, [0.5, 1.0])
    with pytest.raises(RuntimeError, match="no HIP device"):
        mv.UnN_var(X, Z, 2, sigma=1.0)


def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    S = lib.tw_mmd_rows_max_sigma()
    assert 8 <= S <= 64

    def rows(d=3, n_blocks=1, max_n=2, max_m=2, kern=L.TW_MMD_GAUSSIAN, c=p, n_sigma=1, ptr=p,
             rx=p, rz=p):
        return lib.tw_mmd_rows(p, ptr, d, p, p, n_blocks, max_n, max_m, kern, c, n_sigma, p, rx, rz,
                               None)

    E = dict(kern=L.TW_MMD_ENERGY)
    for call, word in ((lambda: rows(ptr=None), b"null pointer"),
                       (lambda: rows(rx=None), b"null pointer"),
                       (lambda: rows(rz=None), b"null pointer"),
                       (lambda: rows(c=None), b"null pointer"),
                       (lambda: rows(n_blocks=-1), b"negative size"),
                       (lambda: rows(max_n=-1), b"negative size"),
                       (lambda: rows(max_m=-2), b"negative size"),
                       (lambda: rows(d=0), b"outside [1, 64]"),
                       (lambda: rows(d=65), b"outside [1, 64]"),
                       (lambda: rows(kern=2), b"unknown kernel"),
                       (lambda: rows(kern=-1), b"unknown kernel"),
                       (lambda: rows(n_sigma=0), b"n_sigma"),
                       (lambda: rows(n_sigma=-3), b"n_sigma"),
                       (lambda: rows(n_sigma=S + 1), b"n_sigma"),
                       (lambda: rows(n_sigma=2, **E), b"energy kernel"),
                       (lambda: rows(max_n=1 << 31), b"2^31"),
                       (lambda: rows(max_m=1 << 31), b"2^31"),
                       (lambda: rows(n_blocks=1 << 30, max_n=1000, max_m=1000), b"grid too large"),
                       (lambda: rows(max_n=10 ** 5, max_m=10 ** 5), b"d_work past"),
                       (lambda: rows(n_blocks=256, max_n=1562, max_m=1562, n_sigma=S), b"d_work past")):
        assert call() == L.TW_ERR_ARG, word
        msg = lib.tw_last_error()
        assert word in msg and b"tw_mmd_rows" in msg, msg
    # nothing to do: no blocks (the energy kernel reads no coefficient)
    assert rows(n_blocks=0) == L.TW_OK and rows(n_blocks=0, c=None, **E) == L.TW_OK
    with pytest.raises(ValueError, match="n_sigma"):
        L.call("tw_mmd_rows", p, p, 3, p, p, 1, 2, 2, 0, p, 0, p, p, p, None)
    wb = lib.tw_mmd_rows_work_bytes
    P = lib.tw_mmd_tile()
    # one tile a side: 3 columns of 4 rows per sigma
    assert wb(1, 2, 2, 1) == 3 * 4 * 8 and wb(1, 2, 2, S) == S * wb(1, 2, 2, 1)
    assert wb(5, P + 1, 3, 2) == 5 * 2 * (2 + 1 + 1) * (P + 4) * 8
    assert wb(0, 2, 2, 1) == 8 and 0 < wb(1, 10 ** 4, 10 ** 4, S) <= 1 << 30
    for bad in ((-1, 2, 2, 1), (1, -1, 2, 1), (1, 2, -1, 1), (1, 2, 2, 0), (1, 2, 2, S + 1),
                (1, 1 << 31, 2, 1), (1, 2, 1 << 31, 1), (1 << 30, 1000, 1000, 1),
                (1, 10 ** 5, 10 ** 5, 1), (256, 1562, 1562, S)):
        assert wb(*bad) == 0, bad


# -------------------------------------------------- the host arithmetic on the oracle's rows
def test_public_functions_on_stubbed_rows(tw, monkeypatch):
    import tuplewise.mmd_var as mv
    monkeypatch.setattr(mv, "_rows_blocks", fake_rows_blocks())
    X, Z = data("gauss", 23, 17, 3, 5)
    for kernel, sigma in (("gaussian", 1.5), ("energy", None)):
        rows, want = mv.row_sums(X, Z, kernel, sigma), o_row_sums(X, Z, kernel, sigma)
        for g, w in zip(rows, want):
            assert g.shape == w.shape and g.dtype == np.float64
            assert np.allclose(g, w, rtol=1e-14, atol=0)
        v, w = mv.Un_var(X, Z, kernel, sigma), o_Un_var(X, Z, kernel, sigma)
        assert isinstance(v.value, np.float64) and isinstance(v.var, np.float64)
        assert abs(v.value - w[0]) <= 1e-13 and abs(v.var - w[1]) <= 1e-12 * w[1]
        assert np.allclose(v.phi_x, w[2], rtol=0, atol=1e-13) and v.phi_x.shape == (23,)
        assert np.allclose(v.phi_z, w[3], rtol=0, atol=1e-13) and v.phi_z.shape == (17,)
        assert abs(v.zeta_x - w[4]) <= 1e-12 * w[4] and abs(v.zeta_z - w[5]) <= 1e-12 * w[5]
        assert abs(v.value - o_Un(X, Z, kernel, sigma)) <= 1e-13
    grid = [0.5, 1.5, 4.0]
    rows = mv.row_sums(X, Z, sigma=grid)
    assert rows.a.shape == rows.r.shape == (3, 23) and rows.q.shape == rows.b.shape == (3, 17)
    v = mv.Un_var(X, Z, sigma=tuple(grid))
    assert v.value.shape == v.var.shape == v.zeta_x.shape == (3,) and v.phi_z.shape == (3, 17)
    for s, sigma in enumerate(grid):
        one = mv.Un_var(X, Z, sigma=sigma)
        assert v.value[s] == one.value and v.var[s] == one.var
        assert np.array_equal(v.phi_x[s], one.phi_x) and np.array_equal(rows.b[s], mv.row_sums(X, Z, sigma=sigma).b)
    assert mv.row_sums(X, Z, sigma=[1.5]).a.shape == (1, 23)


def test_select_sigma_rules_and_split(tw, monkeypatch):
    import tuplewise.mmd_var as mv
    S = tw._lib.lib().tw_mmd_rows_max_sigma()
    launches = []
    monkeypatch.setattr(mv, "_rows_blocks", fake_rows_blocks(launches))
    rng = np.random.RandomState(2)
    X, Z = rng.normal(size=(30, 2)), rng.normal(size=(25, 2)) + 1.0
    grid = list(np.geomspace(0.05, 20.0, 2 * S + 3))
    sel = mv.select_sigma(X, Z, grid)
    assert launches == [S, S, 3]  # launches of the native maximum, then the rest
    index, crit, value, var = o_select(X, Z, grid)
    assert sel.index == index and sel.sigma == grid[index] and isinstance(sel.sigma, float)
    assert np.allclose(sel.criterion, crit, rtol=1e-9, atol=0)
    assert np.allclose(sel.value, value, rtol=0, atol=1e-13) and np.allclose(sel.var, var, rtol=1e-9)
    assert sel.criterion.shape == sel.value.shape == sel.var.shape == (2 * S + 3,)
    assert 0 < index < 2 * S + 2  # an interior maximum: the grid brackets the planted shift
    # reg enters as stated
    big = mv.select_sigma(X, Z, grid, reg=4.0)
    assert np.allclose(big.criterion, value / np.sqrt(var + 4.0), rtol=1e-9, atol=0)
    # ties: the first wins
    tie = mv.select_sigma(X, Z, [0.3, grid[index], 7.0, grid[index]])
    assert tie.index == 1 and tie.criterion[1] == tie.criterion[3]
    # a NaN criterion never wins; all NaN is an error
    Xn = X.copy()
    Xn[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        mv.select_sigma(Xn, Z, [0.5, 1.0])
    real = mv._variance

    def nan_at_the_best(a, r, q, b, kid):
        v = real(a, r, q, b, kid)
        value = v.value.copy()
        value[index] = np.nan
        return v._replace(value=value)

    monkeypatch.setattr(mv, "_variance", nan_at_the_best)
    masked = mv.select_sigma(X, Z, grid)
    c = crit.copy()
    c[index] = np.nan
    assert masked.index == int(np.nanargmax(c)) != index and np.isnan(masked.criterion[index])


@pytest.mark.parametrize("kernel", KERNELS)
def test_UnN_var_is_UnN_with_a_variance(tw, monkeypatch, kernel):
    import tuplewise.mmd as mm
    import tuplewise.mmd_var as mv
    sigma = 1.3 if kernel == "gaussian" else None
    launches = []
    monkeypatch.setattr(mv, "_rows_blocks", fake_rows_blocks(launches))

    def sums_blocks(Xf, Zf, bxo, bzo, kid, c):  # mmd's device glue on the oracle
        return np.array([o_components(Xf[bxo[b]:bxo[b + 1]], Zf[bzo[b]:bzo[b + 1]], kernel, sigma)
                         for b in range(len(bxo) - 1)])

    monkeypatch.setattr(mm, "_sums_blocks", sums_blocks)
    X, Z = data("gauss", 41, 30, 3, 6)
    N = 4
    X1, Z1, X2, Z2, X3, Z3 = X.copy(), Z.copy(), X.copy(), Z.copy(), X.copy(), Z.copy()
    np.random.seed(77)
    value, var = mv.UnN_var(X1, Z1, N, kernel=kernel, sigma=sigma)
    s1 = np.random.get_state()
    np.random.seed(77)
    want = mm.UnN(X2, Z2, N, kernel=kernel, sigma=sigma)
    s2 = np.random.get_state()
    np.random.seed(77)
    o_value, o_var = o_UnN_var(X3, Z3, N, kernel, sigma)
    assert launches == [1]  # all N blocks in one launch of one sigma
    assert abs(value - want) <= 1e-13 and abs(value - o_value) <= 1e-13
    assert abs(var - o_var) <= 1e-12 * o_var and var > 0
    assert same_state(s1, s2) and same_state(s1, np.random.get_state())
    assert np.array_equal(X1, X2) and np.array_equal(Z1, Z2) and not np.array_equal(X1, X)
    assert np.array_equal(X1, X3) and np.array_equal(Z1, Z3)
