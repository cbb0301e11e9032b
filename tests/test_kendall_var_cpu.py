"""tuplewise.kendall_var without a GPU: the brute-force oracle of the per-point row sums (signs
over all ordered pairs, one matrix product per point to c_i, then R, Q, F, E) and its identities; the variance
expressions with the device glue stubbed to the oracle, against a fractions.Fraction evaluation
(==) and against 4/n var(psi_i, ddof=1) of the per-point linearisation; calibration over seeded
replications; UnN_var against kendall.UnN; every argument error before any device work or RNG
draw; the native entries' argument checks."""
import math
import statistics
from fractions import Fraction

import numpy as np
import pytest

from test_kendall_matrix_cpu import o_sign_counts, same_state, stub_launch, table


# ------------------------------------------------------------------------------------ oracle
def o_c(S, lo=0, hi=None):
    """c_i(a, b) for the points i in [lo, hi) against all points: (hi - lo, p, p) int64."""
    S = np.asarray(S)
    A = S[lo:hi]
    s = ((A[:, None, :] > S[None, :, :]).astype(np.int8)
         - (A[:, None, :] < S[None, :, :]).astype(np.int8)).astype(np.float64)
    # einsum("ija,ijb->iab") as a batched product: float64 sums of -1, 0, 1 over fewer than
    # 2^53 points are exact (and use BLAS)
    return np.matmul(s.transpose(0, 2, 1), s).astype(np.int64)


def o_row_moments(S, rows=4096):
    """(R, Q, F, E) int64 (p, p), the points taken in chunks of `rows`."""
    S = np.asarray(S)
    n, p = S.shape
    R, Q, F, E = (np.zeros((p, p), np.int64) for _ in range(4))
    for lo in range(0, n, rows):
        c = o_c(S, lo, min(n, lo + rows))
        u = np.einsum("iaa->ia", c)
        R += c.sum(axis=0)
        Q += (c * c).sum(axis=0)
        F += (c * u[:, :, None]).sum(axis=0)
        E += u.T @ u
    return R, Q, F, E


def stub_rows(X, off):
    """kendall_var._launch by the oracle."""
    out = [o_row_moments(X[int(off[s]):int(off[s + 1])]) for s in range(len(off) - 1)]
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


def f_var_a(R, Q, n, a, b):
    Sm = int(R[a, b])
    return Fraction(4 * (n * int(Q[a, b]) - Sm * Sm), n * n * (n - 1) ** 3)


def f_var_b(R, Q, F, E, n, a, b):
    """The issue's expression as a Fraction; None where a column is constant."""
    Sm, Sa, Sb = int(R[a, b]), int(R[a, a]), int(R[b, b])
    if Sa == 0 or Sb == 0:
        return None
    Cmm, Caa, Cbb = n * int(Q[a, b]) - Sm * Sm, n * int(Q[a, a]) - Sa * Sa, n * int(Q[b, b]) - Sb * Sb
    Cma, Cmb, Cab = n * int(F[a, b]) - Sm * Sa, n * int(F[b, a]) - Sm * Sb, n * int(E[a, b]) - Sa * Sb
    num = (4 * Sa ** 2 * Sb ** 2 * Cmm - 4 * Sm * Sa * Sb ** 2 * Cma - 4 * Sm * Sa ** 2 * Sb * Cmb
           + Sm ** 2 * Sb ** 2 * Caa + Sm ** 2 * Sa ** 2 * Cbb + 2 * Sm ** 2 * Sa * Sb * Cab)
    return Fraction(num, (n - 1) * Sa ** 3 * Sb ** 3)


def np_var(S, variant):
    """4/n var(psi_i, ddof=1) of the per-point linearisation, in float64 NumPy."""
    n = S.shape[0]
    c = o_c(S).astype(np.float64)
    u = np.einsum("iaa->ia", c)
    if variant == "a":
        psi = c / (n - 1)
    else:
        m, ua = c.mean(axis=0), u.mean(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            tb = m / np.sqrt(ua[:, None] * ua[None, :])
            psi = tb * (c / m - u[:, :, None] / (2 * ua[:, None]) - u[:, None, :] / (2 * ua[None, :]))
            psi = np.where(m == 0, c / np.sqrt(ua[:, None] * ua[None, :]), psi)
    return 4.0 / n * psi.var(axis=0, ddof=1)


def special_table(n, seed, dtype=np.float64):
    """Ties, a constant column (2), a duplicated (4 = 0) and a negated (5 = -1) column."""
    rng = np.random.RandomState(seed)
    S = rng.randint(0, 5, size=(n, 6)).astype(dtype)
    S[:, 3] = rng.permutation(n)
    S[:, 2] = 3
    S[:, 4] = S[:, 0]
    S[:, 5] = -S[:, 1]
    return S


@pytest.fixture
def stubbed(tw, monkeypatch):
    import tuplewise.kendall as K
    import tuplewise.kendall_var as V
    monkeypatch.setattr(V, "_launch", stub_rows)
    monkeypatch.setattr(K, "_launch", stub_launch)
    return V


# ------------------------------------------------------------------- the oracle's own checks
@pytest.mark.parametrize("n,seed", [(2, 1), (3, 2), (41, 3), (130, 4)])
def test_oracle_identities(n, seed):
    for dtype in (np.float64, np.int64):
        S = special_table(n, seed, dtype)
        R, Q, F, E = o_row_moments(S, rows=50)
        M, Us, _, _ = o_sign_counts(S)
        assert np.array_equal(R, 2 * M) and np.array_equal(np.diag(R), 2 * Us)
        for a in range(S.shape[1]):
            _, t = np.unique(S[:, a], return_counts=True)
            assert int(Q[a, a]) == int(np.sum(t * (n - t) ** 2))
        u = np.einsum("iaa->ia", o_c(S))
        assert np.array_equal(E, u.T @ u)
        assert np.array_equal(R, R.T) and np.array_equal(Q, Q.T) and np.array_equal(E, E.T)
        assert np.array_equal(np.diag(F), np.diag(Q)) and np.array_equal(np.diag(E), np.diag(Q))
        assert not R[2].any() and not Q[2].any() and not F[2].any() and not E[2].any()
        if n > 3:
            assert not np.array_equal(F, F.T)
        # a duplicated column shares its row with the original, a negated one up to the sign
        assert np.array_equal(R[4], R[0]) and np.array_equal(Q[4], Q[0])
        assert np.array_equal(R[5], -R[1]) and np.array_equal(Q[5], Q[1])


# ------------------------------------------------------------------------ the module, no GPU
def test_module_imports(tw):
    import tuplewise.kendall_var as V
    for name in ("row_moments", "tau_var", "tau_ci", "z_scores", "UnN_var"):
        assert callable(getattr(V, name)), name
    assert V.RowMoments._fields == ("R", "Q", "F", "E", "n")
    assert V.TauVariance._fields == ("tau", "var", "se")


def _fail(*a, **k):
    raise AssertionError("device work before an argument error")


def test_argument_errors_need_no_device(tw, monkeypatch):
    import tuplewise.kendall_var as V
    L = tw._lib
    for name in ("call", "device", "to_device", "to_device_many", "empty", "stream_handle"):
        monkeypatch.setattr(L, name, _fail)
    S = np.arange(40.0).reshape(10, 4)
    nan = S.copy()
    nan[3, 1] = np.nan
    state = np.random.get_state()
    fns = (V.row_moments, V.tau_var, V.tau_ci, V.z_scores, lambda s: V.UnN_var(s, 2))
    bad = []
    for f in fns:
        bad += [lambda f=f: f(np.arange(10.0)),                      # shape
                lambda f=f: f(np.zeros((4, 2, 2))),
                lambda f=f: f(np.zeros((4, 3), np.float32)),         # dtype
                lambda f=f: f(np.zeros((4, 3), np.int32)),
                lambda f=f: f(np.zeros((3, 8)).T),                   # contiguity
                lambda f=f: f(S[:, ::2]),
                lambda f=f: f(S[:1]),                                # n < 2
                lambda f=f: f(np.zeros((4, 0))),                     # p out of range
                lambda f=f: f(np.zeros((2, 1025))),
                lambda f=f: f(np.zeros((2 ** 20 + 1, 1))),           # rows past 2^20
                lambda f=f: f(nan)]                                  # NaN
    bad += [lambda: V.tau_var(S, variant="c"), lambda: V.tau_ci(S, variant=None),
            lambda: V.z_scores(S, variant="tau-b"),
            lambda: V.tau_ci(S, level=0.0), lambda: V.tau_ci(S, level=1.0),
            lambda: V.tau_ci(S, level=-0.5), lambda: V.tau_ci(S, level=float("nan")),
            lambda: V.UnN_var(S, 6), lambda: V.UnN_var(S, 0)]        # blocks of < 2 rows
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        V.UnN_var(S.tolist(), 2)
    assert np.array_equal(S.reshape(-1), np.arange(40.0))
    assert same_state(np.random.get_state(), state)


def test_no_device_raises(tw):
    import torch
    if torch.cuda.is_available():
        return  # (the GPU tests cover the device path)
    import tuplewise.kendall_var as V
    with pytest.raises(RuntimeError, match="no HIP device"):
        V.row_moments(np.arange(10.0).reshape(5, 2))
    with pytest.raises(RuntimeError, match="no HIP device"):
        V.UnN_var(np.arange(20.0).reshape(10, 2), 2)


# ------------------------------------------------------------------------- native entries
def test_native_argument_errors(tw):
    L = tw._lib
    lib = L.lib()

    def rows(p=2, n_shards=1, max_n=4, width=16):
        return lib.tw_kendall_rows(None, p, None, n_shards, max_n, width, None, None, None, None,
                                   None, None)

    for call, word in ((lambda: rows(n_shards=-1), b"n_shards"), (lambda: rows(max_n=-1), b"max_n"),
                       (lambda: rows(max_n=2 ** 20 + 1, width=32), b"max_n"),
                       (lambda: rows(p=0), b"columns"), (lambda: rows(p=1025), b"columns"),
                       (lambda: rows(width=24), b"width"),
                       (lambda: rows(max_n=65537), b"16-bit"), (lambda: rows(), b"null")):
        assert call() == L.TW_ERR_ARG
        msg = lib.tw_last_error()
        assert word in msg and b"tw_kendall_rows" in msg, msg
    assert rows(n_shards=0) == L.TW_OK


def test_work_sizes_and_hook_ranges(tw):
    lib = tw._lib.lib()
    # five int64 sums per entry and shard
    assert lib.tw_kendall_rows_work_bytes(3, 5) >= 5 * 3 * 25 * 8
    assert lib.tw_kendall_rows_work_bytes(1, 1024) >= 5 * 8 << 20
    assert lib.tw_kendall_rows_work_bytes(1, 1024) % 8 == 0
    assert lib.tw_kendall_rows_work_bytes(1, 0) == 0 and lib.tw_kendall_rows_work_bytes(1, 1025) == 0
    assert lib.tw_kendall_rows_work_bytes(-1, 4) == 0
    for hook, good, bad in ((lib.tw_kendall_rows_set_plan, (1, 7, 100000), (-1, -7)),
                            (lib.tw_kendall_rows_set_anchors, (1, 2, 4), (-1, 3, 5, 8))):
        try:
            assert hook(0) >= 0
            prev = 0
            for v in good:  # a hook returns the value it replaced
                assert hook(v) == prev
                prev = v
            for v in bad:
                assert hook(v) == -1 and b"tw_kendall_rows_set_" in lib.tw_last_error()
                assert hook(prev) == prev  # a refused value changed nothing
        finally:
            hook(0)
        assert hook(0) == 0


# --------------------------------------------------- the host half on the oracle's integers
@pytest.mark.parametrize("n,seed", [(60, 5), (33, 6)])
def test_variances_are_the_expressions(stubbed, n, seed):
    """var == the Fraction evaluation converted to float (one rounding), for both variants; the
    Fraction and the float64 per-point forms agree to 1e-9 relative (the NumPy form subtracts a
    mean of size <= n from values of that size: about n 2^-52 relative per term)."""
    V = stubbed
    import tuplewise.kendall as K
    S = special_table(n, seed)
    keep = S.copy()
    m = V.row_moments(S)
    R, Q, F, E = o_row_moments(S)
    assert isinstance(m, V.RowMoments) and type(m.n) is int and m.n == n
    for got, want in zip(m[:4], (R, Q, F, E)):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    p = S.shape[1]
    for variant in ("a", "b"):
        tv = V.tau_var(S, variant)
        assert isinstance(tv, V.TauVariance) and tv.var.dtype == np.float64
        assert np.array_equal(tv.tau, K.tau_matrix(S, variant=variant), equal_nan=True)
        ref = np_var(S, variant)
        for a in range(p):
            for b in range(p):
                fr = f_var_a(R, Q, n, a, b) if variant == "a" else f_var_b(R, Q, F, E, n, a, b)
                if fr is None:
                    assert a == 2 or b == 2
                    assert np.isnan(tv.var[a, b]) and np.isnan(tv.se[a, b])
                    continue
                assert tv.var[a, b] == float(fr), (variant, a, b)
                assert tv.se[a, b] == math.sqrt(max(float(fr), 0.0))
                assert fr >= 0
                assert abs(float(fr) - ref[a, b]) <= 1e-9 * max(float(fr), ref[a, b]) + 1e-18, \
                    (variant, a, b, float(fr), ref[a, b])
        if variant == "b":
            for a in range(p):
                if a != 2:
                    assert tv.var[a, a] == 0.0 and tv.tau[a, a] == 1.0
            # tau-b of a duplicated or negated column is +-1 with no spread
            assert tv.var[0, 4] == 0.0 and tv.var[4, 0] == 0.0 and abs(tv.tau[0, 4] - 1) < 1e-15
            assert tv.var[1, 5] == 0.0 and tv.var[5, 1] == 0.0 and abs(tv.tau[1, 5] + 1) < 1e-15
        else:
            assert not np.isnan(tv.var).any() and (tv.var[2] == 0.0).all()
    assert np.array_equal(S, keep)


def test_var_is_zero_without_ties_for_equal_and_negated_columns(stubbed):
    """Distinct values: c_i(a, a) = n - 1 for every i, so tau-a of a column with itself or with
    its negation has variance exactly 0.0 too."""
    V = stubbed
    rng = np.random.RandomState(8)
    x = rng.permutation(50).astype(np.float64)
    S = np.ascontiguousarray(np.stack([x, x, -x, rng.normal(size=50)], axis=1))
    for variant in ("a", "b"):
        tv = V.tau_var(S, variant)
        for a, b in ((0, 0), (0, 1), (0, 2), (1, 2), (3, 3)):
            assert tv.var[a, b] == 0.0 and tv.var[b, a] == 0.0
        assert tv.var[0, 3] > 0.0
    assert np.array_equal(V.tau_var(S, "a").var, V.tau_var(S, "b").var)  # no ties: tau-a = tau-b


def test_ci_and_z_scores(stubbed):
    V = stubbed
    S = special_table(45, 9)
    for variant in ("a", "b"):
        tau, var, se = V.tau_var(S, variant)
        for level in (0.5, 0.95, 0.999):
            z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * level)
            t, lo, hi = V.tau_ci(S, variant, level)
            assert np.array_equal(t, tau, equal_nan=True)
            assert np.array_equal(lo, np.clip(tau - z * se, -1, 1), equal_nan=True)
            assert np.array_equal(hi, np.clip(tau + z * se, -1, 1), equal_nan=True)
            ok = ~np.isnan(tau)
            assert (lo[ok] >= -1).all() and (hi[ok] <= 1).all() and (lo[ok] <= hi[ok]).all()
        zs = V.z_scores(S, variant)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert np.array_equal(zs, tau / se, equal_nan=True)
    zs = V.z_scores(S, "b")
    assert zs[0, 0] == np.inf and zs[0, 4] == np.inf and zs[1, 5] == -np.inf
    assert np.isnan(zs[2, 0]) and np.isnan(zs[2, 2])
    assert np.isnan(V.z_scores(S, "a")[2, 0])  # 0 / 0


# ------------------------------------------------------------------------------ calibration
REPS = 400
SETTINGS = [(100, 0.0, False), (100, 0.6, False), (80, 0.5, True)]


def population_tau(rho, ties):
    """(tau-a, tau-b) of the population: 2/pi asin(rho) for the bivariate normal itself; for
    the floored pair (x, y) = floor(1.5 (z0, rho z0 + sqrt(1 - rho^2) z1)), which has another
    tau, from its cell probabilities: P(x = i, y = j) is the integral over z0 in cell i of the
    normal density times the conditional probability of cell j (midpoint rule, 1200 points a
    cell, cells out to 6 sigma), then tau-a = P(concordant) - P(discordant) over two
    independent draws and tau-b = tau-a / sqrt(P(x differs) P(y differs))."""
    if not ties:
        return (2 / math.pi * math.asin(rho),) * 2
    Phi = np.vectorize(statistics.NormalDist().cdf)
    cells = np.arange(-9, 9)
    sd = math.sqrt(1 - rho * rho)
    P = np.zeros((len(cells), len(cells)))
    for a, i in enumerate(cells):
        z = (i + (np.arange(1200) + 0.5) / 1200) / 1.5
        w = np.exp(-0.5 * z * z) / math.sqrt(2 * math.pi) / (1.5 * 1200)
        edges = Phi((np.arange(cells[0], cells[-1] + 2)[:, None] / 1.5 - rho * z[None, :]) / sd)
        P[a] = ((edges[1:] - edges[:-1]) * w[None, :]).sum(axis=1)
    assert abs(P.sum() - 1) < 1e-7
    below = np.zeros_like(P)                  # P(x' < i, y' < j)
    below[1:, 1:] = P.cumsum(axis=0).cumsum(axis=1)[:-1, :-1]
    cross = np.zeros_like(P)                  # P(x' < i, y' > j)
    cross[1:, :-1] = P.cumsum(axis=0)[:-1, ::-1].cumsum(axis=1)[:, ::-1][:, 1:]
    tau_a = 2 * float((P * (below - cross)).sum())
    px, py = P.sum(axis=1), P.sum(axis=0)
    return tau_a, tau_a / math.sqrt((1 - float(px @ px)) * (1 - float(py @ py)))


def _draw(rng, n, rho, ties):
    z = rng.normal(size=(n, 2))
    S = np.stack([z[:, 0], rho * z[:, 0] + math.sqrt(1 - rho * rho) * z[:, 1]], axis=1)
    return np.ascontiguousarray(np.floor(1.5 * S) if ties else S)


@pytest.mark.parametrize("n,rho,ties", SETTINGS)
def test_calibration(stubbed, n, rho, ties):
    """mean(estimated variance) / empirical variance of tau over seeded replications lies in
    0.8-1.25 for both variants, and tau_ci at level 0.95 covers the population tau in 0.90-0.99
    of them at every setting and for both variants: 2/pi asin(rho) for the bivariate normal,
    and for the floored pair its own tau-a and tau-b (flooring moves them to 0.308 and 0.377
    from 0.333; 0.940 and 0.9375 seen).  Against 2/pi asin(rho) the floored setting is asserted for tau-a too
    (0.953 seen); tau-b, which no longer estimates that number, covers it in 0.853 of the
    replications and is printed only."""
    V = stubbed
    rng = np.random.RandomState(1000 + n + int(10 * rho))
    normal = 2 / math.pi * math.asin(rho)
    target = dict(zip("ab", population_tau(rho, ties)))
    taus, vars_, hit = {"a": [], "b": []}, {"a": [], "b": []}, {"a": 0, "b": 0}
    hit_normal = {"a": 0, "b": 0}
    for _ in range(REPS):
        S = _draw(rng, n, rho, ties)
        for variant in ("a", "b"):
            tau, lo, hi = V.tau_ci(S, variant, 0.95)
            taus[variant].append(tau[0, 1])
            vars_[variant].append(V.tau_var(S, variant).var[0, 1])
            hit[variant] += bool(lo[0, 1] <= target[variant] <= hi[0, 1])
            hit_normal[variant] += bool(lo[0, 1] <= normal <= hi[0, 1])
    for variant in ("a", "b"):
        ratio = np.mean(vars_[variant]) / np.var(taus[variant], ddof=1)
        print(f"n={n} rho={rho} ties={ties} variant={variant}: ratio {ratio:.3f}, coverage of "
              f"tau = {target[variant]:.4f} {hit[variant] / REPS:.4f}, of 2/pi asin(rho) "
              f"{hit_normal[variant] / REPS:.4f}")
        assert 0.8 <= ratio <= 1.25, (variant, ratio)
        assert 0.90 <= hit[variant] / REPS <= 0.99, (variant, hit[variant] / REPS)
        if variant == "a" or not ties:
            assert 0.90 <= hit_normal[variant] / REPS <= 0.99, (variant, hit_normal[variant] / REPS)


# ------------------------------------------------------------------------------ UnN_var
@pytest.mark.parametrize("N", [3, 8])
def test_UnN_var_is_UnN_with_a_variance(stubbed, N):
    V = stubbed
    import tuplewise.kendall as K
    S = table(64 * 3 + 5, 3, 200 + N, ties=True)
    A, B = S.copy(), S.copy()
    np.random.seed(4321 + N)
    value, var = V.UnN_var(A, N)
    after = np.random.get_state()
    np.random.seed(4321 + N)
    want = K.UnN(B, N)
    assert np.array_equal(value, want) and np.array_equal(A, B)
    assert same_state(after, np.random.get_state())
    k = int(S.shape[0] / N)
    blocks = []
    for b in range(N):
        R, Q, _, _ = o_row_moments(B[b * k:(b + 1) * k])
        blocks.append([[float(f_var_a(R, Q, k, a, c)) for c in range(3)] for a in range(3)])
    assert var.shape == (3, 3)
    assert np.array_equal(var, K._last_axis_mean(np.array(blocks)).reshape(3, 3) / N)
