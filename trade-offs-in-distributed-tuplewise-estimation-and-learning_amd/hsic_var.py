"""The variance of HSIC_u (and of the unbiased squared distance covariance) estimated from the
sample, a normal confidence interval, and the bandwidth pair of a grid chosen by estimated test
power (an extension).

X, Y, kernel and sigma are tuplewise.hsic's, checked by its own functions: everything that is a
ValueError in hsic.Un is one here, raised before any device work with the RNG untouched.  sigma
may also be a SEQUENCE OF PAIRS (sigma_x, sigma_y) — a list or tuple of 2-sequences, or an (S, 2)
array; Gaussian kernel only; an entry of a pair positive and finite, or the string "median":
every result then has a leading axis of its length S.  "median", alone or inside a pair, is
resolved once per public call (per side: hsic's rule), before any shuffle.

The device (csrc/hsic_rows.hip, tw_hsic_rows) returns three row sums per point and pair of a
launch; with K and L of tuplewise.hsic (zero diagonals), two launches on one upload give

    p_i = sum_j K_ij L_ij      k_i = sum_j K_ij      l_i = sum_j L_ij        (no weights)
    u_i = sum_j K_ij l_j       v_i = sum_j L_ij k_j      (the first launch's rows as weights)

each squared distance evaluated once and held while g is applied per pair of the grid, so a K_ij
has the bits tw_hsic_sums gives it.  The rest is float64 NumPy on those rows.  With S_KL = sum(p)
/ 2, R_K = sum(k), R_L = sum(l), R_KL = k . l and T = 2 (n - 1)(n - 2) S_KL + R_K R_L - 2 (n - 1)
R_KL, the statistic is T / (n (n - 1)(n - 2)(n - 3)), and the first-order (Hajek) component of
item i — the mean of the symmetrised degree-4 kernel over the 4-tuples that contain i (Song et
al. 2012, Theorem 5), (T - T_{-i}) / (4 (n - 1)(n - 2)(n - 3)) with T_{-i} on the sample without
i — is, expanded so that nothing cancels,

    h_i = ((n - 2)^2 p_i + (n - 2)(2 S_KL - u_i - v_i) - n k_i l_i + R_L k_i + R_K l_i - R_KL)
          / (2 (n - 1)(n - 2)(n - 3))

value = mean(h) is the statistic exactly, zeta = var(h, ddof=1), and

    var = 16 zeta / n          se = sqrt(max(var, 0))

is the first-order term of Var(HSIC_u).  It omits the second-order term (of order 1 / n^2).
Under independence zeta -> 0 and that omitted term dominates: this variance is NOT a test of
independence — tuplewise.hsic_perm is.  It is for standard errors and intervals of a dependence
that is there, and for choosing a bandwidth.

select_sigma maximises the test-power criterion J = value / sqrt(max(var, 0) + reg) over a grid
of pairs.  A grid longer than tw_hsic_rows_max_sigma() takes several pairs of launches of that
size; a pair's rows do not depend on the other pairs of its launch or on its position, so the
split changes no number.
"""
from __future__ import annotations

import math
import statistics
from typing import NamedTuple

import numpy as np

from . import _lib as L
from . import hsic as _hsic
from .kendall_var import _check_level


class HSICRows(NamedTuple):
    """p, k, l, u, v: (n,) float64 — or (S, n) for a sequence of S pairs."""
    p: np.ndarray
    k: np.ndarray
    l: np.ndarray  # noqa: E741
    u: np.ndarray
    v: np.ndarray


class HSICVariance(NamedTuple):
    """value: the statistic (= mean(h)); var = 16 zeta / n; se = sqrt(max(var, 0)); h (n,): the
    components; zeta: their sample variance.  A leading S axis for a sequence of pairs."""
    value: np.ndarray
    var: np.ndarray
    se: np.ndarray
    h: np.ndarray
    zeta: np.ndarray


class SigmaSelection(NamedTuple):
    """sigma = the grid's pair at index = argmax criterion (two numbers, "median" resolved);
    criterion, value, var: (S,) float64."""
    sigma: tuple
    index: int
    criterion: np.ndarray
    value: np.ndarray
    var: np.ndarray


# ------------------------------------------------------------------------------ host checks
_SEQ = (list, tuple, np.ndarray)


def _is_grid(sigma) -> bool:
    """A sequence of pairs: an array of two or more axes, or a list / tuple with a sequence in
    it.  (A flat list or tuple is hsic's own pair.)"""
    if isinstance(sigma, np.ndarray):
        return sigma.ndim >= 2
    return isinstance(sigma, (list, tuple)) and any(isinstance(s, _SEQ) for s in sigma)


def _sides(sigma):
    """The two entries of one sigma of hsic (a scalar serves both sides)."""
    return tuple(sigma) if isinstance(sigma, _SEQ) else (sigma, sigma)


def _check(X, Y, kernel, sigma):
    """(Xf, Yf, kernel id, sigmas, cs, grid) or a ValueError, before anything touches a device or
    the RNG: sigmas the pairs as given, cs their coefficient pairs (None for a "median" side)."""
    grid = _is_grid(sigma)
    if grid:
        if isinstance(sigma, np.ndarray) and (sigma.ndim != 2 or sigma.shape[1] != 2):
            raise ValueError(f"a grid of sigma pairs has shape (S, 2), not {sigma.shape}")
        sigmas = list(sigma)
        if kernel == "distance":
            raise ValueError("the distance kernel takes no sigma")
        if not sigmas and kernel in _hsic._KERNELS:
            raise ValueError("the grid of sigma pairs is empty")
        for s in sigmas:
            if not isinstance(s, _SEQ):
                raise ValueError(f"sigma={s!r} inside a grid: every entry is a pair "
                                 f"(sigma_x, sigma_y)")
    else:
        sigmas = [sigma]
    cs = [_hsic._coef(kernel, s)[1:] for s in sigmas]
    Xf, Yf, kid, _, _ = _hsic._check(X, Y, kernel, sigmas[0] if sigmas else None)
    return Xf, Yf, kid, sigmas, cs, grid


def _resolve(Xf, Yf, kernel, sigmas, cs):
    """(pairs, cs) as numbers: every "median" side becomes that side's median distance, each
    side's taken once (device work: after every check, before any shuffle)."""
    if kernel == "distance":
        return [None], cs
    need_x, need_y = any(c[0] is None for c in cs), any(c[1] is None for c in cs)
    pairs = [_sides(s) for s in sigmas]
    if not (need_x or need_y):
        return [(float(sx), float(sy)) for sx, sy in pairs], cs
    (mx, my), cmx, cmy = _hsic._resolve(
        Xf, Yf, ("median" if need_x else 1.0, "median" if need_y else 1.0),
        None if need_x else 0.0, None if need_y else 0.0)
    return ([(float(mx if c[0] is None else sx), float(my if c[1] is None else sy))
             for (sx, sy), c in zip(pairs, cs)],
            [(cmx if c[0] is None else c[0], cmy if c[1] is None else c[1]) for c in cs])


def _work_bytes(nb: int, max_n: int, S: int) -> int:
    """tw_hsic_rows_work_bytes (a host computation), or a ValueError for a refused shape."""
    nbytes = int(L.lib().tw_hsic_rows_work_bytes(nb, max_n, S))
    if nbytes == 0:
        raise ValueError(f"tw_hsic_rows refuses {nb} block(s) of up to {max_n} rows at {S} sigma "
                         f"pair(s): its partials would pass 1 GiB")
    return nbytes


# ------------------------------------------------------------------------------ device glue
def _rows_blocks(Xf, Yf, off, kid, cs):
    """tw_hsic_rows twice on one upload: (first, second), each (S, rows, 3) float64, for the
    blocks b = rows [off[b], off[b + 1]) of both arrays and the S = len(cs) <=
    tw_hsic_rows_max_sigma() coefficient pairs.  first[..., :] = (p, k, l), the launch without
    weights; second[..., :] = (p, K l, L k), the launch that reads first as its weights."""
    t = L.torch()
    off = np.asarray(off, dtype=np.int64)
    nb, S = len(off) - 1, len(cs)
    max_n, rows = int(np.diff(off).max()), int(off[-1])
    nbytes = _work_bytes(nb, max_n, S)
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    xd, yd, od, cd = L.to_device_many(
        [Xf.reshape(-1), Yf.reshape(-1), off, np.asarray(cs, dtype=np.float64).reshape(-1)])
    work = L.empty((nbytes // 8,), t.float64)
    first, second = L.empty((S, rows, 3), t.float64), L.empty((S, rows, 3), t.float64)
    for weights, out in ((None, first), (first, second)):
        L.call("tw_hsic_rows", xd, Xf.shape[1], yd, Yf.shape[1], od, nb, max_n, kid, cd, S,
               weights, work, out, L.stream_handle())
    return first.cpu().numpy(), second.cpu().numpy()


def _grid_step(nb: int, max_n: int, S: int) -> int:
    """The pairs per launch of a grid of S: tw_hsic_rows_max_sigma(), fewer where the partials of
    that many would pass the work budget; a ValueError where one pair's do (a host computation:
    callers run it before any device work)."""
    step = min(S, int(L.lib().tw_hsic_rows_max_sigma()))
    while step > 1 and int(L.lib().tw_hsic_rows_work_bytes(nb, max_n, step)) == 0:
        step -= 1
    _work_bytes(nb, max_n, step)
    return step


def _rows_grid(Xf, Yf, off, kid, cs):
    """_rows_blocks for a grid of any length: launches of _grid_step pairs."""
    step = _grid_step(len(off) - 1, int(np.diff(np.asarray(off)).max()), len(cs))
    parts = [_rows_blocks(Xf, Yf, off, kid, cs[s0:s0 + step]) for s0 in range(0, len(cs), step)]
    if len(parts) == 1:
        return parts[0]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _five(first, second):
    """(p, k, l, u, v) of the two launches' rows."""
    return first[..., 0], first[..., 1], first[..., 2], second[..., 1], second[..., 2]


def _variance(p, k, l, u, v):  # noqa: E741
    """HSICVariance of rows with a trailing axis of n and any leading axes."""
    n = p.shape[-1]
    with np.errstate(invalid="ignore", over="ignore"):
        s_kl = p.sum(axis=-1, keepdims=True) / 2.0
        r_k, r_l = k.sum(axis=-1, keepdims=True), l.sum(axis=-1, keepdims=True)
        r_kl = (k * l).sum(axis=-1, keepdims=True)
        h = ((n - 2.0) ** 2 * p + (n - 2.0) * (2.0 * s_kl - u - v) - n * (k * l) + r_l * k
             + r_k * l - r_kl) / (2.0 * (n - 1.0) * (n - 2.0) * (n - 3.0))
        value = h.mean(axis=-1)
        zeta = ((h - value[..., None]) ** 2).sum(axis=-1) / (n - 1)
        var = 16.0 * zeta / n
        return HSICVariance(value, var, np.sqrt(np.maximum(var, 0.0)), h, zeta)


def _level(level) -> float:
    try:
        return _check_level(level)
    except TypeError:
        raise ValueError(f"level={level!r} is not a number") from None


# ------------------------------------------------------------------------------- public
def row_sums(X, Y, kernel="gaussian", sigma=None):
    """HSICRows(p, k, l, u, v) of the whole sample; a sequence of S pairs gives (S, n)."""
    Xf, Yf, kid, sigmas, cs, grid = _check(X, Y, kernel, sigma)
    _grid_step(1, Xf.shape[0], len(cs))  # a refused shape: a ValueError before any device work
    _, cs = _resolve(Xf, Yf, kernel, sigmas, cs)
    rows = _five(*_rows_grid(Xf, Yf, [0, Xf.shape[0]], kid, cs))
    return HSICRows(*(np.ascontiguousarray(r if grid else r[0]) for r in rows))


def Un_var(X, Y, kernel="gaussian", sigma=None):
    """The complete statistic and its first-order variance estimate from the sample.  Not a test
    of independence (under independence the omitted second-order term dominates):
    tuplewise.hsic_perm is."""
    Xf, Yf, kid, sigmas, cs, grid = _check(X, Y, kernel, sigma)
    _grid_step(1, Xf.shape[0], len(cs))  # a refused shape: a ValueError before any device work
    _, cs = _resolve(Xf, Yf, kernel, sigmas, cs)
    v = _variance(*_five(*_rows_grid(Xf, Yf, [0, Xf.shape[0]], kid, cs)))
    if grid:
        return v
    return HSICVariance(np.float64(v.value[0]), np.float64(v.var[0]), np.float64(v.se[0]), v.h[0],
                        np.float64(v.zeta[0]))


def Un_ci(X, Y, level=0.95, kernel="gaussian", sigma=None):
    """(value, lo, hi): value -+ z se with z the normal quantile of (1 + level) / 2.  The
    interval of a dependence that is there, not a test of independence (tuplewise.hsic_perm)."""
    z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * _level(level))
    v = Un_var(X, Y, kernel, sigma)
    return v.value, v.value - z * v.se, v.value + z * v.se


def UnN_var(X, Y, N, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """(value, var) of the block-wise complete statistic: hsic.UnN's draw and blocks (one
    np.random.permutation(n) applied in place to both arrays: the RNG is consumed identically and
    X, Y are left as hsic.UnN leaves them), all N blocks through the two tw_hsic_rows launches;
    value is the mean of the blocks' values, var the mean of the blocks' var divided by N (the
    blocks are disjoint).  sigma is one bandwidth (a scalar or a pair), not a sequence of pairs."""
    if _is_grid(sigma):
        raise ValueError("UnN_var takes one sigma (a scalar or a pair), not a sequence of pairs")
    sigma = _hsic._resolve_blocks(X, Y, N, sampling_type, kernel, sigma, True)
    _, _, kid, cx, cy = _hsic._check(X, Y, kernel, sigma)
    Xf, Yf, k = _hsic._partition(X, Y, N, sampling_type, True)
    _work_bytes(N, k, 1)  # a refused shape: a ValueError before the draw
    perm = np.random.permutation(Xf.shape[0])
    X[:] = X[perm]
    Y[:] = Y[perm]
    first, second = _rows_blocks(Xf[:N * k], Yf[:N * k], np.arange(N + 1) * k, kid,
                                 [(cx, cy)])  # Xf / Yf view the shuffled arrays
    v = _variance(*_five(first[0].reshape(N, k, 3), second[0].reshape(N, k, 3)))
    return np.float64(np.mean(v.value)), np.float64(np.mean(v.var) / N)


def select_sigma(X, Y, sigmas, reg=1e-8, kernel="gaussian"):
    """The pair of the grid that maximises criterion[s] = value[s] / sqrt(max(var[s], 0) + reg);
    the first on ties; a NaN criterion never wins and an all-NaN grid is a ValueError."""
    if kernel != "gaussian":
        raise ValueError(f"kernel={kernel!r}: select_sigma is offered for the Gaussian kernel only")
    if not _is_grid(sigmas):
        raise ValueError("sigmas must be a sequence of pairs (sigma_x, sigma_y)")
    try:
        reg = float(reg)
    except (TypeError, ValueError):
        raise ValueError(f"reg={reg!r} is not a number") from None
    if not (math.isfinite(reg) and reg >= 0.0):
        raise ValueError(f"reg = {reg} must be finite and >= 0")
    Xf, Yf, _, grid, cs, _ = _check(X, Y, kernel, sigmas)
    grid, _ = _resolve(Xf, Yf, kernel, grid, cs)
    v = Un_var(Xf, Yf, kernel, grid)
    with np.errstate(invalid="ignore", divide="ignore"):
        crit = v.value / np.sqrt(np.maximum(v.var, 0.0) + reg)
    if np.isnan(crit).all():
        raise ValueError("every criterion of the grid is NaN")
    index = int(np.nanargmax(crit))
    return SigmaSelection(grid[index], index, crit, v.value, v.var)
