"""The pair function g of tuplewise.mmd / tuplewise.hsic at the edges of its range, without a GPU:
the exact references the GPU tests of tests/test_gpu_kernel_range.py compare single terms with,
the argument grids those tests run on the device, and a chunked exact integer oracle for the
large launch plans of tests/test_gpu_mmd_perm_plan.py.

References for single terms are exact arithmetic, not NumPy: `decimal` at 60 digits (exp and sqrt
are correctly rounded there), rounded once more to float64 by float() of the decimal string, which
is correctly rounded too (subnormals and the underflow to 0.0 included).  A float64 result can sit
within 1e-60 of a rounding boundary only if exp(a) or sqrt(D) agrees with a midpoint to 200 bits:
exp of a non-zero float64 is transcendental and such an agreement is not expected among a few
hundred points; a square root of a float64 differs from every midpoint by more than 2^-108
relative.

A grid point is two coordinates (a, b) and a coefficient c: D is the squared distance the kernels
form from the rows, fl(fl(a - b) * fl(a - b)), and the Gaussian argument is p = fl(c * D).  c is a
launch parameter, so the Gaussian grid uses a few values of c (one launch each) and reaches the
regimes through D.  Regimes are named by what the exact exp(p) rounds to; the tests below check
every point's membership with the reference, never with NumPy."""
import decimal
import functools
import math

import numpy as np
import pytest

from test_gpu_mmd_perm import int_oracle
from test_mmd_perm_cpu import random_labels
from test_triplets_cpu import o_dist_pairs

CTX = decimal.Context(prec=60, Emin=-999999, Emax=999999,
                      traps=[decimal.InvalidOperation, decimal.DivisionByZero])
TINY = 2.0 ** -1074   # the spacing of subnormal results
MIN_NORMAL = 2.0 ** -1022
PER_REGIME = 64       # points per finite regime, at least

# The Gaussian regimes: name -> (lo, hi) of p = c * D (None: not an interval of p)
G_REGIMES = {
    "one": (-(2.0 ** -54), 0.0),          # |p| < 2^-54: exp rounds to exactly 1.0
    "small": (-1.0, -(2.0 ** -30)),
    "mid": (-700.0, -1.0),
    "last_normal": (-708.4, -700.0),      # (2^-1022 = exp(-708.396...): -708.4 is already past it)
    "subnormal": (-745.13, -708.4),
    "cut": None,                          # the two float64 either side of ln(2^-1075)
    "zero": (-1e4, -746.0),
    "inf": None,                          # D = +inf, c < 0
}
E_REGIMES = ("subnormal", "tiny", "ordinary", "huge", "inf")
# launch coefficients of the interval regimes: D around 1e-280 ... 1e283 reaches the same p
G_COEFS = (-0.5, -1e280, -1e-280)


# --------------------------------------------------------------------------------- references
def ref_exp(a):
    """exp(a) of a float64 a to 60 digits (a Decimal)."""
    return CTX.exp(decimal.Decimal(float(a)))


def ref_sqrt(D):
    """sqrt(D) of a finite float64 D >= 0 to 60 digits (a Decimal)."""
    return CTX.sqrt(decimal.Decimal(float(D)))


def rounded(exact):
    """The float64 nearest to a Decimal (ties to even; 0.0 below 2^-1075)."""
    return float(exact)


def ulps(got, exact):
    """|got - exact| / np.spacing(round(exact)): the spacing is 2^-1074 for subnormal and zero
    results, so one definition covers normal, subnormal and underflowed results."""
    got = float(got)
    if math.isnan(got):
        return float("nan")
    if math.isinf(got):
        return float("inf")
    sp = decimal.Decimal(float(np.spacing(abs(rounded(exact)))))
    return float(CTX.divide(abs(CTX.subtract(decimal.Decimal(got), exact)), sp))


@functools.lru_cache(maxsize=None)
def cut_pair():
    """(a0, a1): the largest float64 whose exact exp rounds to 0.0 and its successor towards 0,
    the smallest whose exp rounds to 2^-1074 — found with the reference, not assumed."""
    lo, hi = -745.25, -745.0  # exp is monotone: bisect on the floats
    assert rounded(ref_exp(lo)) == 0.0 and rounded(ref_exp(hi)) > 0.0
    while True:
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if rounded(ref_exp(mid)) == 0.0:
            lo = mid
        else:
            hi = mid
    a = lo
    assert np.nextafter(a, 0.0) == hi
    return float(a), float(np.nextafter(a, 0.0))


# --------------------------------------------------------------------------------------- grids
def _rows_for(t, rng):
    """Coordinates (a, b) with a - b close to t: half the pairs at a = 0, the rest shifted."""
    k = rng.randint(-3, 4, size=t.shape) * (rng.uniform(size=t.shape) < 0.5)
    a = k * t
    return a, a - t


def _grid(a, b, c, regime):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        D = o_dist_pairs(a[:, None], b[:, None])
    return dict(a=a, b=b, D=D, c=np.broadcast_to(np.float64(c), a.shape).copy(),
                regime=np.asarray(regime))


def _concat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


@functools.lru_cache(maxsize=None)
def arg_grid():
    """The Gaussian grid: arrays a, b (the two rows' coordinate), D (their squared distance as the
    kernels form it), c (the launch coefficient) and regime (a name of G_REGIMES)."""
    rng = np.random.RandomState(54)
    parts = []
    for c in G_COEFS:
        for name, iv in G_REGIMES.items():
            if iv is None:
                continue
            lo, hi = iv
            if name == "one":
                # p from -2^-55 down to subnormal products, and D = 0, D subnormal, D underflowed
                p = -(2.0 ** rng.uniform(-1000.0 if c > -1.0 else -130.0, -55.0, size=32))
            elif name == "small":
                p = -(2.0 ** rng.uniform(-29.9, -0.1, size=32))
            else:
                w = hi - lo
                p = rng.uniform(lo + 1e-3 * w, hi - 1e-3 * w, size=32)
            t = np.sqrt(p / c) * rng.choice([-1.0, 1.0], size=32)
            if name == "one":
                t[:3] = [0.0, 1e-160 if c > -1.0 else 1e-161, 1e-170]  # D = 0, subnormal, underflowed
            a, b = _rows_for(t, rng)
            parts.append(_grid(a, b, c, [name] * 32))
        # D = +inf from a finite coordinate whose square overflows, and from an infinite one
        parts.append(_grid([0.0, 1e200, np.inf, 3.0], [1e160, -1e200, 0.0, -np.inf], c, ["inf"] * 4))
    a0, a1 = cut_pair()
    shifts = [0.0, 1.0, -3.0, 0.5, 1024.0, -0.25, 7.0, -100.0, 2.0 ** 20, -6.5, 12.0]
    for arg in (a0, a1):
        for t in (0.5, 1.0, 2.0):  # D = t * t and c = arg / D, both exact: p = arg exactly
            s = np.array(shifts) * t
            parts.append(_grid(s, s + t, arg / (t * t), ["cut"] * len(s)))
    # c = 0 is allowed (sigma = inf is not, but the native entry takes it): p = 0 whatever D is
    parts.append(_grid([0.0, 1.0, -2.5, 1e150], [1.0, 1.0, 4.0, -1e150], 0.0, ["one"] * 4))
    return _concat(parts)


@functools.lru_cache(maxsize=None)
def energy_grid():
    """The energy grid: a, b, D and regime (a name of E_REGIMES); c is unused (0.0)."""
    rng = np.random.RandomState(55)
    n = PER_REGIME
    sign = lambda: rng.choice([-1.0, 1.0], size=n)  # noqa: E731
    t = {
        "subnormal": sign() * 10.0 ** rng.uniform(-161.5, -154.2, size=n),  # coordinates ~1e-160
        "tiny": sign() * 2.0 ** rng.uniform(-510.9, -500.1, size=n),        # D in [2^-1022, 2^-1000]
        "ordinary": sign() * 10.0 ** rng.uniform(-3.0, 3.0, size=n),
        "huge": sign() * np.concatenate([2.0 ** rng.uniform(511.0, 511.99, size=n // 2),
                                         10.0 ** rng.uniform(149.5, 150.5, size=n - n // 2)]),
    }
    t["ordinary"][:8] = [0.0, 1.0, 3.0, 1e-3, 12345.0, 2.0 ** -20, 1e8 + 1.0, 0.1]
    parts = []
    for name, tt in t.items():
        a, b = _rows_for(tt, rng)
        parts.append(_grid(a, b, 0.0, [name] * n))
    parts.append(_grid([0.0, 1e200, np.inf, 3.0, -1e160, -np.inf],
                       [1e160, -1e200, 0.0, -np.inf, 1e160, np.inf], 0.0, ["inf"] * 6))
    return _concat(parts)


def gauss_arg(grid):
    """p = fl(c * D), the argument of exp, as the kernels and the oracle form it."""
    with np.errstate(over="ignore"):
        return grid["c"] * grid["D"]


@functools.lru_cache(maxsize=None)
def gauss_refs():
    """The exact exp(p) of every point of arg_grid() (Decimals; 0 for D = +inf)."""
    g = arg_grid()
    return tuple(decimal.Decimal(0) if np.isinf(p) else ref_exp(p) for p in gauss_arg(g))


def subset(grid, regimes, per=4):
    """The first `per` points of every regime: the indices."""
    return np.concatenate([np.flatnonzero(grid["regime"] == r)[:per] for r in regimes])


# ------------------------------------------------------------------------ chunked int oracle
def int_oracle_chunked(a, labels, chunk=512):
    """(P, 3) int64 sums of |a_i - a_j| (Sxx, Szz, Sxz of every label row) for N distinct
    integers a below 2^20, in row chunks of at most 512 rows: no N x N array is held.  The matrix
    products run in float64 and are exact: every partial sum of a product is a non-negative
    integer below 512 * 2^20 = 2^29, whatever the order; the sums over a row are accumulated in
    int64."""
    assert 1 <= chunk <= 512
    a = np.asarray(a, dtype=np.int64)
    S = np.asarray(labels, dtype=np.float64)
    S0 = 1.0 - S
    P, N = S.shape
    assert a.shape == (N,) and a.min() >= 0 and a.max() < 2 ** 20
    out = np.zeros((P, 3), dtype=np.int64)
    for r0 in range(0, N, chunk):
        G = np.abs(a[r0:r0 + chunk, None] - a[None, :]).astype(np.float64)
        R1 = S[:, r0:r0 + chunk] @ G   # (P, N): sum over the chunk's rows in the first sample
        R0 = S0[:, r0:r0 + chunk] @ G
        assert R1.max() < 2.0 ** 53 and R0.max() < 2.0 ** 53
        out[:, 0] += (R1 * S).astype(np.int64).sum(axis=1)    # ordered pairs, both in the first
        out[:, 1] += (R0 * S0).astype(np.int64).sum(axis=1)
        out[:, 2] += (R1 * S0).astype(np.int64).sum(axis=1)   # first-sample row, second-sample column
    assert np.all(out[:, :2] % 2 == 0)
    out[:, :2] //= 2
    return out


# ---------------------------------------------------------------------------------- the tests
def test_references():
    assert rounded(ref_exp(0.0)) == 1.0 and rounded(ref_exp(1.0)) == math.e
    assert rounded(ref_exp(-800.0)) == 0.0 and rounded(ref_exp(-744.0)) == 2 * TINY
    assert rounded(ref_sqrt(4.0)) == 2.0 and rounded(ref_sqrt(2.0)) == math.sqrt(2.0)
    assert ulps(1.0, ref_exp(0.0)) == 0.0 and ulps(1.0 + 2.0 ** -52, ref_exp(0.0)) == 1.0
    assert 1.55 < ulps(0.0, ref_exp(-744.0)) < 1.56  # exp(-744) = 1.553 * 2^-1074
    assert ulps(TINY, ref_exp(-800.0)) == pytest.approx(1.0, abs=1e-9)
    assert math.isnan(ulps(float("nan"), ref_exp(0.0))) and math.isinf(ulps(float("inf"), ref_exp(0.0)))
    a0, a1 = cut_pair()
    assert a0 < a1 == np.nextafter(a0, 0.0) and abs(a0 + 1075.0 * math.log(2.0)) < 1e-12
    assert rounded(ref_exp(a0)) == 0.0 and rounded(ref_exp(a1)) == TINY
    assert ref_exp(a0) < decimal.Decimal(TINY) / 2 < ref_exp(a1)


def test_grid_regimes():
    """Every point is in its regime and every finite regime holds its count — by the reference."""
    g, p, refs = arg_grid(), gauss_arg(arg_grid()), gauss_refs()
    r = np.array([rounded(e) for e in refs])
    a0, a1 = cut_pair()
    for name, iv in G_REGIMES.items():
        at = g["regime"] == name
        print(name, int(at.sum()), "p in", [p[at].min(), p[at].max()], "exp in", [r[at].min(), r[at].max()])
        if name != "inf":
            assert at.sum() >= PER_REGIME and np.isfinite(g["D"][at]).all(), name
        if iv is not None:
            assert np.all((p[at] >= iv[0]) & (p[at] <= iv[1])), name
    assert set(g["regime"]) == set(G_REGIMES)
    at = lambda name: g["regime"] == name  # noqa: E731
    assert np.all(np.abs(p[at("one")]) < 2.0 ** -54) and np.all(r[at("one")] == 1.0)
    assert (g["D"][at("one")] == 0.0).any() and ((g["D"][at("one")] > 0) & (g["D"][at("one")] < MIN_NORMAL)).any()
    assert (p[at("one")] == 0.0).any() and ((p[at("one")] < 0) & (p[at("one")] > -MIN_NORMAL)).any()
    for name in ("small", "mid", "last_normal"):
        assert np.all((r[at(name)] >= MIN_NORMAL) & (r[at(name)] < 1.0)), name
    assert np.all((r[at("subnormal")] > 0.0) & (r[at("subnormal")] < MIN_NORMAL))
    assert r[at("subnormal")].min() <= 4 * TINY and r[at("subnormal")].max() >= 2.0 ** -1030
    assert np.all(r[at("zero")] == 0.0)
    cut = p[at("cut")]
    assert set(cut.tolist()) == {a0, a1} and (cut == a0).sum() >= 32 and (cut == a1).sum() >= 32
    assert np.all(r[at("cut")] == np.where(cut == a0, 0.0, TINY))
    assert np.all(np.isinf(g["D"][at("inf")]) & (g["c"][at("inf")] < 0.0)) and at("inf").sum() >= 8
    assert np.all(g["c"] <= 0.0) and np.isfinite(g["c"]).all() and not np.isnan(p).any()
    assert len(np.unique(g["c"])) <= 12  # one launch per coefficient
    # D spans the whole exponent range for every interval regime
    for name in ("small", "mid", "last_normal", "subnormal", "zero"):
        assert g["D"][at(name)].min() < 1e-270 and g["D"][at(name)].max() > 1e270, name


def test_numpy_exp_is_within_one_ulp():
    """The oracle's np.exp against the exact exp on the grid (0.62 ulp at most was seen on 800
    such arguments); exactly 1 and exactly 0 where the reference says so."""
    g, p, refs = arg_grid(), gauss_arg(arg_grid()), gauss_refs()
    got = np.exp(p)
    err = np.array([ulps(v, e) for v, e in zip(got, refs)])
    for name in G_REGIMES:
        print(name, "np.exp max ulps", err[g["regime"] == name].max())
    assert err.max() <= 1.0
    r = np.array([rounded(e) for e in refs])
    assert np.all(got[r == 0.0] == 0.0) and np.all(got[r == 1.0] == 1.0)


def test_numpy_sqrt_is_correctly_rounded():
    g = energy_grid()
    D, root = g["D"], np.sqrt(g["D"])
    for name in E_REGIMES:
        at = g["regime"] == name
        print(name, int(at.sum()), "D in", [D[at].min(), D[at].max()])
        assert at.sum() >= (PER_REGIME if name != "inf" else 4), name
    at = lambda name: g["regime"] == name  # noqa: E731
    assert np.all((D[at("subnormal")] > 0.0) & (D[at("subnormal")] < MIN_NORMAL))
    assert np.all((D[at("tiny")] >= MIN_NORMAL) & (D[at("tiny")] <= 2.0 ** -1000))
    assert np.all((D[at("ordinary")] >= 0.0) & (D[at("ordinary")] < 1e17))
    assert (D[at("ordinary")] == 0.0).any()
    assert np.all((D[at("huge")] > 1e298) & np.isfinite(D[at("huge")])) and D[at("huge")].max() > 2.0 ** 1023
    assert np.all(np.isposinf(D[at("inf")])) and np.all(np.isposinf(root[at("inf")]))
    fin = np.isfinite(D)
    want = np.array([rounded(ref_sqrt(v)) for v in D[fin]])
    assert np.array_equal(root[fin].view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("chunk", [512, 64, 7])
def test_chunked_int_oracle(chunk):
    N, n, P = 300, 131, 19
    rng = np.random.RandomState(chunk)
    a = rng.choice(2 ** 20, size=N, replace=False)
    labels = random_labels(rng, P, n, N)
    labels[0] = False
    labels[0, :n] = True
    want = int_oracle(a, labels)
    got = int_oracle_chunked(a, labels, chunk)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    # the observed split by the definition
    x, z = a[:n].astype(np.int64), a[n:].astype(np.int64)
    assert got[0, 0] == np.abs(x[:, None] - x[None, :]).sum() // 2
    assert got[0, 1] == np.abs(z[:, None] - z[None, :]).sum() // 2
    assert got[0, 2] == np.abs(x[:, None] - z[None, :]).sum()
