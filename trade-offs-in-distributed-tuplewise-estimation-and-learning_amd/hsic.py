"""Kernel independence U-statistics of degree 4 on MI355X (an extension; the reference has
none): are two vector-valued measurements of the same items dependent?  The unbiased
Hilbert-Schmidt independence criterion HSIC_u (Song et al. 2012), the unbiased squared distance
covariance dCov^2_u (Szekely-Rizzo 2014: the same formula with the kernel |a - b|) and their
normalised forms (the unbiased CKA, the bias-corrected distance correlation).

The sample is paired rows: X is (n, dx) and Y is (n, dy), float64 and C-contiguous (a 1-D array
is d = 1), 1 <= dx, dy <= 64, n >= 4; anything else is a ValueError before any device work or
RNG draw.  D is the squared Euclidean distance of tuplewise.triplets in its arithmetic order and
g the pair function of tuplewise.mmd:

    kernel="gaussian"  K_ij = exp(c_x * D(x_i, x_j)), L_ij = exp(c_y * D(y_i, y_j)), c = -1.0 /
                       (2.0 * sigma * sigma) computed here in Python floats; sigma is required: a
                       positive finite scalar for both sides or a pair (sigma_x, sigma_y); either
                       may be the string "median" (below)
    kernel="distance"  K_ij = sqrt(D(x_i, x_j)), L_ij = sqrt(D(y_i, y_j)); sigma must be None

with zero diagonals.  The device reduces (csrc/hsic.hip): every unordered pair
is evaluated once, and with the row sums k_i = sum_j K_ij, l_i = sum_j L_ij eight doubles leave
the chip per block,

    S_KL S_KK S_LL = sums over i < j of K L, K K, L L
    R_K R_L R_KL R_KK R_LL = sums over i of k, l, k l, k k, l l

(and, for row_sums, the two row-sum vectors).  The statistic is formed here in Python floats:

    U(S, Ra, Rb, Rab) = (2 S + Ra Rb / ((n - 1)(n - 2)) - 2 Rab / (n - 2)) / (n (n - 3))
    Un          = U(S_KL, R_K, R_L, R_KL)     HSIC_u, or dCov^2_u for "distance"; no sign flip
    correlation = Un / sqrt(U(S_KK, R_K, R_K, R_KK) * U(S_LL, R_L, R_L, R_LL)), NaN if the
                  product is not > 0

Un is the mean over all ordered 4-tuples of distinct indices of f(i, j, q, r) = K_ij (L_ij +
L_qr - 2 L_iq); the incomplete statistic is the mean of f over drawn 4-tuples (tw_hsic_idx32).
The sums are floats added in the kernel's order: no bit contract, but run-to-run deterministic,
and a block's sums are the same bits alone or beside other blocks.  The estimators mirror
tuplewise.mmd for the proportional partition without replacement: the host owns the shuffle and
the draws (NumPy's global legacy RNG, in NumPy's order), the device the arithmetic.

The permutation test that judges Un is its own module, tuplewise.hsic_perm.

sigma="median" is the median heuristic PER SIDE: sigma_x is the median Euclidean distance over the
pairs i < j of X and sigma_y that of Y, exact (tuplewise.bandwidth.median_distance(X), DESIGN.md
§4.16); a pair may mix, e.g. ("median", 2.0).  It is resolved ONCE per public call, after every
argument check and before the shuffle or the first draw, and the numbers are passed down: a side's
median does not change when the rows are permuted, so the reshuffled estimators (UnNT, UnNBT) use
one value and the RNG is consumed exactly as with those numbers.  With "median" a non-finite entry
on that side is a ValueError (with a numeric sigma a NaN propagates into the sums instead), and so
is a median of 0; with the distance kernel "median" is a ValueError like any other sigma.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib as L
from .compute_stats import _check_index
from .numpy_rng import randint_batch
from .triplets import _rows

_KERNELS = {"gaussian": L.TW_HSIC_GAUSSIAN, "distance": L.TW_HSIC_DISTANCE}
MAX_D = 64
MIN_N = 4


class Components(NamedTuple):
    """The eight sums of one block, in tw_hsic_sums' order."""
    S_KL: np.float64
    S_KK: np.float64
    S_LL: np.float64
    R_K: np.float64
    R_L: np.float64
    R_KL: np.float64
    R_KK: np.float64
    R_LL: np.float64


# ------------------------------------------------------------------------------ host checks
def _is_median(sigma) -> bool:
    return isinstance(sigma, str) and sigma == "median"


def _one_coef(sigma):
    if _is_median(sigma):
        return None  # resolved by _resolve once the rows are checked
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"sigma={sigma!r} is not a number") from None
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma = {sigma} must be positive and finite")
    if 2.0 * sigma * sigma == 0.0:
        raise ValueError(f"sigma = {sigma}: -1 / (2 sigma^2) overflows")
    return -1.0 / (2.0 * sigma * sigma)


def _coef(kernel, sigma):
    """(kernel id, c_x, c_y) or a ValueError: c = -1 / (2 sigma^2) per side for the Gaussian
    kernel, 0.0 (unused) for the distance kernel; a side's c is None for "median", which _resolve
    turns into a number."""
    if kernel not in _KERNELS:
        raise ValueError(f"kernel={kernel!r} is not one of {list(_KERNELS)}")
    if kernel == "distance":
        if sigma is not None:
            raise ValueError("the distance kernel takes no sigma")
        return _KERNELS[kernel], 0.0, 0.0
    if sigma is None:
        raise ValueError("the Gaussian kernel needs sigma")
    if isinstance(sigma, (tuple, list, np.ndarray)):
        if len(np.shape(sigma)) != 1 or len(sigma) != 2:
            raise ValueError(f"sigma={sigma!r}: a scalar or a pair (sigma_x, sigma_y)")
        return _KERNELS[kernel], _one_coef(sigma[0]), _one_coef(sigma[1])
    c = _one_coef(sigma)
    return _KERNELS[kernel], c, c


def _check(X, Y, kernel, sigma):
    """(Xf, Yf, kernel id, c_x, c_y) or a ValueError, before anything touches a device or the
    RNG."""
    kid, cx, cy = _coef(kernel, sigma)
    Xf, Yf = _rows(X, "X"), _rows(Y, "Y")
    if Xf.shape[0] != Yf.shape[0]:
        raise ValueError(f"X has {Xf.shape[0]} rows and Y has {Yf.shape[0]}: the sample is paired")
    for A, name in ((Xf, "X"), (Yf, "Y")):
        if not 1 <= A.shape[1] <= MAX_D:
            raise ValueError(f"{name} has d = {A.shape[1]}, outside [1, {MAX_D}]")
    if Xf.shape[0] < MIN_N:
        raise ValueError(f"{Xf.shape[0]} row(s): a 4-tuple needs four items")
    if Xf.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    return Xf, Yf, kid, cx, cy


def _resolve(Xf, Yf, sigma, cx, cy):
    """(sigma, c_x, c_y) as numbers: a side given as "median" (its c is None) gets the median
    distance over the pairs of that side's rows — device work, so callers finish their argument
    checks first and call this once, before any shuffle or draw.  With no such side everything is
    returned as it is."""
    if cx is not None and cy is not None:
        return sigma, cx, cy
    from . import bandwidth
    _median_sigma = bandwidth._median_sigma
    sx, sy = sigma if isinstance(sigma, (tuple, list, np.ndarray)) else (sigma, sigma)
    for A, name, c in ((Xf, "X", cx), (Yf, "Y", cy)):  # both sides' rows before any device work
        if c is None:
            bandwidth._check_finite(A, name)
    if cx is None:
        sx = _median_sigma(Xf, None, "within", "X")
    if cy is None:
        sy = _median_sigma(Yf, None, "within", "Y")
    return (sx, sy), _one_coef(sx), _one_coef(sy)


def _checked(X, Y, kernel, sigma):
    """_check and _resolve: for the calls whose every argument check is _check's."""
    Xf, Yf, kid, cx, cy = _check(X, Y, kernel, sigma)
    sigma, cx, cy = _resolve(Xf, Yf, sigma, cx, cy)
    return Xf, Yf, kid, cx, cy, sigma


def _u(s, ra, rb, rab, n: int) -> float:
    s, ra, rb, rab = float(s), float(ra), float(rb), float(rab)
    return (2.0 * s + ra * rb / ((n - 1) * (n - 2)) - 2.0 * rab / (n - 2)) / (n * (n - 3))


def _value(c, n: int) -> np.float64:
    return np.float64(_u(c[0], c[3], c[4], c[5], n))


def _corr(c, n: int) -> np.float64:
    vxy = _u(c[0], c[3], c[4], c[5], n)
    vxx, vyy = _u(c[1], c[3], c[3], c[6], n), _u(c[2], c[4], c[4], c[7], n)
    prod = vxx * vyy
    if not prod > 0.0:
        return np.float64("nan")
    return np.float64(vxy / math.sqrt(prod))


def _value_indexed(s, B: int) -> np.float64:
    return np.float64((float(s[0]) + float(s[1]) - 2.0 * float(s[2])) / B)


# ------------------------------------------------------------------------------ device glue
def _work_bytes(nb: int, max_n: int, group: int = 0) -> int:
    """tw_hsic_work_bytes (a host computation), or a ValueError for a shape the launch refuses."""
    nbytes = int(L.lib().tw_hsic_work_bytes(nb, max_n, group))
    if nbytes == 0:
        raise ValueError(f"{nb} block(s) of up to {max_n} rows: the row-sum partials would pass "
                         f"the device work budget (DESIGN.md §4.14)")
    return nbytes


def _sums_blocks(Xf, Yf, off, kid, cx, cy, want_rows=False, group=0):
    """tw_hsic_sums on one upload: the (n_blocks, 8) doubles of the blocks b = rows [off[b],
    off[b + 1]) of both arrays and, if asked, the (rows, 2) row sums."""
    t = L.torch()
    off = np.asarray(off, dtype=np.int64)
    nb = len(off) - 1
    max_n = int(np.diff(off).max())
    nbytes = _work_bytes(nb, max_n, group)
    L.device()  # no HIP device: the package's RuntimeError, before any device call
    xd, yd, od = L.to_device_many([Xf.reshape(-1), Yf.reshape(-1), off])
    work = L.empty((nbytes // 8,), t.float64)
    out = L.empty((nb, 8), t.float64)
    rows = L.empty((Xf.shape[0], 2), t.float64) if want_rows else None
    L.call("tw_hsic_sums", xd, Xf.shape[1], yd, Yf.shape[1], od, nb, max_n, kid, cx, cy, group,
           work, rows, out, L.stream_handle())
    return out.cpu().numpy(), (rows.cpu().numpy() if want_rows else None)


def _sums_indexed(Xf, Yf, ii, jj, qq, rr, quad_off, kid, cx, cy):
    """tw_hsic_idx32 on one upload: the (n_shards, 3) doubles A, B, C of the given 4-tuples
    (absolute rows)."""
    t = L.torch()
    L.device()
    quad_off = np.asarray(quad_off, dtype=np.int64)
    ns = len(quad_off) - 1
    xd, yd, id_, jd, qd, rd, od = L.to_device_many(
        [Xf.reshape(-1), Yf.reshape(-1), ii.astype(np.int32), jj.astype(np.int32),
         qq.astype(np.int32), rr.astype(np.int32), quad_off])
    max_q = int(np.diff(quad_off).max()) if ns else 0
    work = L.empty((max(1, int(L.lib().tw_hsic_idx_work_bytes(ns, max_q)) // 8),), t.float64)
    out = L.empty((ns, 3), t.float64)
    L.call("tw_hsic_idx32", xd, Xf.shape[1], yd, Yf.shape[1], id_, jd, qd, rd, od, ns, max_q, kid,
           cx, cy, work, out, L.stream_handle())
    return out.cpu().numpy()


# ------------------------------------------------------------------------------- estimators
def components(X, Y, kernel="gaussian", sigma=None):
    """The eight sums S_KL, S_KK, S_LL, R_K, R_L, R_KL, R_KK, R_LL of the whole sample."""
    Xf, Yf, kid, cx, cy, _ = _checked(X, Y, kernel, sigma)
    s = _sums_blocks(Xf, Yf, [0, Xf.shape[0]], kid, cx, cy)[0][0]
    return Components(*(np.float64(v) for v in s))


def row_sums(X, Y, kernel="gaussian", sigma=None):
    """(k, l): the (n,) float64 row sums k_i = sum_j K_ij and l_i = sum_j L_ij."""
    Xf, Yf, kid, cx, cy, _ = _checked(X, Y, kernel, sigma)
    rows = _sums_blocks(Xf, Yf, [0, Xf.shape[0]], kid, cx, cy, want_rows=True)[1]
    return rows[:, 0].copy(), rows[:, 1].copy()


def Un(X, Y, kernel="gaussian", sigma=None):
    """The complete statistic: HSIC_u (Gaussian) or the unbiased squared distance covariance."""
    Xf, Yf, kid, cx, cy, _ = _checked(X, Y, kernel, sigma)
    s = _sums_blocks(Xf, Yf, [0, Xf.shape[0]], kid, cx, cy)[0][0]
    return _value(s, Xf.shape[0])


def correlation(X, Y, kernel="gaussian", sigma=None):
    """Un / sqrt(Un(X, X) Un(Y, Y)): the unbiased CKA (Gaussian) or the bias-corrected squared
    distance correlation; NaN if the product of the two self terms is not > 0."""
    Xf, Yf, kid, cx, cy, _ = _checked(X, Y, kernel, sigma)
    s = _sums_blocks(Xf, Yf, [0, Xf.shape[0]], kid, cx, cy)[0][0]
    return _corr(s, Xf.shape[0])


def UB_indices(X, Y, i, j, q, r, kernel="gaussian", sigma=None):
    """The mean of f(i, j, q, r) = K_ij (L_ij + L_qr - 2 L_iq) over the given 4-tuples of rows,
    the four indices of a tuple distinct."""
    Xf, Yf, kid, cx, cy = _check(X, Y, kernel, sigma)
    n = Xf.shape[0]
    i, j, q, r = (_check_index(np.asarray(a), n) for a in (i, j, q, r))
    if not i.shape == j.shape == q.shape == r.shape:
        raise ValueError(f"operands could not be broadcast together with shapes "
                         f"{i.shape} {j.shape} {q.shape} {r.shape}")
    i, j, q, r = (a.reshape(-1) for a in (i, j, q, r))
    # (rows as _check_index returns them, >= 0)
    if (np.any(i == j) or np.any(i == q) or np.any(i == r) or np.any(j == q) or np.any(j == r)
            or np.any(q == r)):
        raise ValueError("a 4-tuple needs four distinct rows")
    _, cx, cy = _resolve(Xf, Yf, sigma, cx, cy)
    if i.size == 0:
        return np.float64("nan")  # the mean of no terms
    s = _sums_indexed(Xf, Yf, i, j, q, r, [0, i.size], kid, cx, cy)[0]
    return _value_indexed(s, i.size)


def _tuples_from(a0, a1, a2, a3):
    """The draws a0 in [0, n), a1 in [0, n - 1), a2 in [0, n - 2), a3 in [0, n - 3) as four
    distinct rows: each later index is stepped past the earlier ones in ascending order."""
    i = a0
    j = a1 + (a1 >= i)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    q = a2 + (a2 >= lo)
    q = q + (q >= hi)
    s = np.sort(np.stack([i, j, q]), axis=0)
    r = a3 + (a3 >= s[0])
    r = r + (r >= s[1])
    r = r + (r >= s[2])
    return i, j, q, r


def _draw_tuples(n: int, B: int):
    """B 4-tuples, uniform over four distinct rows: randint(0, n, B), randint(0, n - 1, B),
    randint(0, n - 2, B), randint(0, n - 3, B) from the global legacy RNG, in this order."""
    try:  # the same four calls (values and state) in one native call
        a = randint_batch([(0, n, B), (0, n - 1, B), (0, n - 2, B), (0, n - 3, B)])
    except NotImplementedError:  # the global generator is not the legacy MT19937
        a = [np.random.randint(0, n - t, B) for t in range(4)]
    return _tuples_from(*a)


def UB(X, Y, B, kernel="gaussian", sigma=None):
    """The incomplete statistic: B 4-tuples drawn with replacement."""
    Xf, Yf, _, _, _, sigma = _checked(X, Y, kernel, sigma)
    i, j, q, r = _draw_tuples(Xf.shape[0], int(B))
    return UB_indices(Xf, Yf, i, j, q, r, kernel, sigma)


class _Complete:
    """Tag of a block function made by UnN: every block's Un, all blocks in one tw_hsic_sums
    launch."""

    def __init__(self, kernel, sigma):
        self.kid, self.cx, self.cy = _coef(kernel, sigma)

    def precheck(self, k, N):
        _work_bytes(N, k)

    def evaluate(self, Xf, Yf, k, N):
        s = _sums_blocks(Xf[:N * k], Yf[:N * k], np.arange(N + 1) * k, self.kid, self.cx,
                         self.cy)[0]
        return [_value(b, k) for b in s]


class _Incomplete:
    """Tag of a block function made by UnNB: every block's UB, the draws in block order (four
    calls for each block), all blocks in one tw_hsic_idx32 launch."""

    def __init__(self, B, kernel, sigma):
        self.B = int(B)
        self.kid, self.cx, self.cy = _coef(kernel, sigma)

    def evaluate(self, Xf, Yf, k, N):
        B = self.B
        try:  # the 4N calls of the N blocks, in their order, in one native call
            d = randint_batch([(0, k, B), (0, k - 1, B), (0, k - 2, B), (0, k - 3, B)] * N)
            draws = [_tuples_from(*d[4 * b:4 * b + 4]) for b in range(N)]
        except NotImplementedError:  # the global generator is not the legacy MT19937
            draws = [_draw_tuples(k, B) for _ in range(N)]
        if B == 0:
            return [np.float64("nan")] * N
        idx = [np.concatenate([t[c] + b * k for b, t in enumerate(draws)]) for c in range(4)]
        s = _sums_indexed(Xf[:N * k], Yf[:N * k], *idx, np.arange(N + 1) * B, self.kid, self.cx,
                          self.cy)
        return [_value_indexed(b, B) for b in s]


def _block_fn(spec, fn):
    fn._tw_hsic_block = spec
    return fn


def _partition(X, Y, N, sampling_type, complete):
    """UN's argument checks: (Xf, Yf, k) or a ValueError, before the draw.  complete: the blocks
    go through tw_hsic_sums, which refuses some shapes."""
    if sampling_type != "prop-SWOR":
        raise ValueError(f"sampling_type={sampling_type!r}: only the proportional partition "
                         f"without replacement ('prop-SWOR') is offered for HSIC; 'SWOR' and "
                         f"'prop-SWR' are out of scope (DESIGN.md §4.14)")
    if not isinstance(X, np.ndarray) or not isinstance(Y, np.ndarray):
        raise ValueError("UN shuffles the caller's NumPy arrays in place")
    Xf, Yf, _, _, _ = _check(X, Y, "distance", None)
    n = Xf.shape[0]
    try:
        k = int(n / N)
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f"N = {N!r} is not a number of blocks") from None
    if N < 1 or k < MIN_N:
        raise ValueError(f"N = {N} blocks of {k} row(s): a block needs at least {MIN_N} rows")
    if complete:
        _work_bytes(N, k)  # a refused shape: a ValueError before the draw
    return Xf, Yf, k


def _resolve_blocks(X, Y, N, sampling_type, kernel, sigma, complete):
    """sigma of a block estimator as numbers: where a side is "median", every check of the call
    (the rows, then UN's partition) runs first, then each such side's median is taken once.  Any
    other sigma is returned as it is, with nothing checked here."""
    if not (_is_median(sigma) or (isinstance(sigma, (tuple, list))
                                  and any(_is_median(s) for s in sigma))):
        return sigma
    Xf, Yf, _, cx, cy = _check(X, Y, kernel, sigma)
    if cx is not None and cy is not None:
        return sigma
    _partition(X, Y, N, sampling_type, complete)
    return _resolve(Xf, Yf, sigma, cx, cy)[0]


def UN(X, Y, N, f_block, sampling_type="prop-SWOR"):
    """Draws perm = np.random.permutation(n) once and applies it in place to BOTH arrays (X[:] =
    X[perm]; Y[:] = Y[perm]: the pairing survives), cuts N blocks of k = int(n / N) >= 4 rows
    (the remainder is left out) and averages f_block(x, y) over them.  Block functions made by
    this module (the closures of UnN / UnNB) are evaluated together on the device; any other
    callable is called block by block."""
    spec = getattr(f_block, "_tw_hsic_block", None)
    Xf, Yf, k = _partition(X, Y, N, sampling_type, hasattr(spec, "precheck"))
    n = Xf.shape[0]
    perm = np.random.permutation(n)
    X[:] = X[perm]
    Y[:] = Y[perm]
    if spec is not None:
        return np.mean(spec.evaluate(Xf, Yf, k, N))  # Xf / Yf view the shuffled arrays
    return np.mean([f_block(X[b * k:(b + 1) * k], Y[b * k:(b + 1) * k]) for b in range(N)])


def UnN(X, Y, N, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Block-wise complete statistic."""
    sigma = _resolve_blocks(X, Y, N, sampling_type, kernel, sigma, True)

    def fun_block(x, y):
        return Un(x, y, kernel=kernel, sigma=sigma)

    _check(X, Y, kernel, sigma)
    return UN(X, Y, N, _block_fn(_Complete(kernel, sigma), fun_block), sampling_type)


def UnNB(X, Y, N, B, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Block-wise incomplete statistic."""
    sigma = _resolve_blocks(X, Y, N, sampling_type, kernel, sigma, False)

    def fun_block(x, y):
        return UB(x, y, B, kernel=kernel, sigma=sigma)

    _check(X, Y, kernel, sigma)
    return UN(X, Y, N, _block_fn(_Incomplete(B, kernel, sigma), fun_block), sampling_type)


def UnNT(X, Y, N, T, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Reshuffled block-wise complete statistic."""
    sigma = _resolve_blocks(X, Y, N, sampling_type, kernel, sigma, True)  # once for all T
    return np.mean([UnN(X, Y, N, sampling_type, kernel, sigma) for _ in range(T)])


def UnNBT(X, Y, N, B, T, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Reshuffled block-wise incomplete statistic."""
    sigma = _resolve_blocks(X, Y, N, sampling_type, kernel, sigma, False)  # once for all T
    return np.mean([UnNB(X, Y, N, B, sampling_type, kernel, sigma) for _ in range(T)])
