"""Kernel two-sample U-statistics of degree (2,2) on MI355X (an extension; the reference has
none): the unbiased squared maximum mean discrepancy MMD^2_u (Gretton et al.) and the energy
distance (Szekely-Rizzo), both the mean over quadruples of

    h((x, x'), (z, z')) = g(x, x') + g(z, z') - g(x, z') - g(x', z)

X is (n, d) and Z is (m, d), float64 and C-contiguous (a 1-D array is d = 1), 1 <= d <= 64,
n >= 2, m >= 2; anything else is a ValueError before any device work or RNG draw.

D(a, b) is the squared Euclidean distance of tuplewise.triplets, in its arithmetic order (acc =
0.0; for c in 0..d-1: t = a_c - b_c; acc = acc + t * t, never fused, direct differences only), so
D(a, a) = 0 exactly and D(a, b) = D(b, a) bit for bit.  The pair function:

    kernel="gaussian"  g = exp(c * D), c = -1.0 / (2.0 * sigma * sigma) computed here in Python
                       floats; sigma is required: positive and finite, or the string "median"
    kernel="energy"    g = sqrt(D); sigma must be None

The device reduces (csrc/mmd.hip): per block three doubles leave the chip,

    Sxx = sum_{i<j} g(x_i, x_j)    Szz = sum_{k<l} g(z_k, z_l)    Sxz = sum_{i,k} g(x_i, z_k)

and the statistic is formed here: V = 2 Sxx / (n (n - 1)) + 2 Szz / (m (m - 1)) - 2 Sxz / (n m);
the Gaussian value is V (MMD^2_u), the energy value is -V (the energy distance is MMD^2_u with
k = -|.|).  The sums are floats added in the kernel's order: no bit contract, but run-to-run
deterministic, and a block's sums are the same bits alone or beside other blocks.  The
incomplete statistic evaluates h on drawn quadruples (i != j rows of X, k != l rows of Z) through
tw_mmd_idx32.  The estimators mirror tuplewise.triplets for the proportional partition without
replacement: the host owns the shuffles and the draws (NumPy's global legacy RNG, in NumPy's
order), the device the arithmetic.

The permutation test (permutation_sums, permutation_test; csrc/mmd_perm.hip)
relabels the pooled sample: every permutation's three sums come from ONE launch that evaluates
each g(w_i, w_j) once per pass of tw_mmd_perm_cols() permutations and multiplies it by the 0 / 1
labels on the float64 matrix unit.  A column's sums depend only on the rows and on that column's
labels, bit for bit, so a permutation that reproduces the observed split compares equal to the
observed value.  A NaN or, under the energy kernel, an overflowing distance (D = +inf, g = +inf)
anywhere in the pooled sample makes all three sums of every column NaN (0 * inf in the label
products, inf - inf in the identities): permutation_test then returns a NaN statistic, an all-NaN
null and pvalue = 1 / (n_perm + 1).  Under the Gaussian kernel a pair with D = +inf is a term of
exactly 0 and every column is finite.

sigma="median" is the median heuristic: the median Euclidean distance over the pairs of the POOLED
sample [X; Z], exact (tuplewise.bandwidth.median_distance(X, Z, pairs="pooled")).
It is resolved ONCE per public call, after every argument check and before the first shuffle or
draw, and the number is passed down: the pooled median does not change under the shuffles of the
block estimators or under the relabellings of the permutation test, so the reshuffled estimators
(UnNT, UnNBT) and every null column use the same value, and the RNG is consumed exactly as with
that number.  With sigma="median" a non-finite entry in X or Z is a ValueError (with a numeric
sigma a NaN propagates into the sums instead), and so is a median of 0; with the energy kernel
"median" is a ValueError like any other sigma.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib as L
from .compute_stats import _check_index
from .numpy_rng import randint_batch
from .triplets import _rows

_KERNELS = {"gaussian": L.TW_MMD_GAUSSIAN, "energy": L.TW_MMD_ENERGY}
MAX_D = 64


# ------------------------------------------------------------------------------ host checks
def _is_median(sigma) -> bool:
    return isinstance(sigma, str) and sigma == "median"


def _coef(kernel, sigma):
    """(kernel id, c) or a ValueError: c = -1 / (2 sigma^2) for the Gaussian kernel, 0.0 (unused)
    for the energy kernel; c is None for sigma="median", which _resolve turns into a number."""
    if kernel not in _KERNELS:
        raise ValueError(f"kernel={kernel!r} is not one of {list(_KERNELS)}")
    if kernel == "energy":
        if sigma is not None:
            raise ValueError("the energy kernel takes no sigma")
        return _KERNELS[kernel], 0.0
    if sigma is None:
        raise ValueError("the Gaussian kernel needs sigma")
    if _is_median(sigma):
        return _KERNELS[kernel], None  # resolved by _resolve once the rows are checked
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"sigma={sigma!r} is not a number") from None
    if not (math.isfinite(sigma) and sigma > 0.0):
        raise ValueError(f"sigma = {sigma} must be positive and finite")
    if 2.0 * sigma * sigma == 0.0:
        raise ValueError(f"sigma = {sigma}: -1 / (2 sigma^2) overflows")
    return _KERNELS[kernel], -1.0 / (2.0 * sigma * sigma)


def _check(X, Z, kernel, sigma):
    """(Xf, Zf, kernel id, c) or a ValueError, before anything touches a device or the RNG."""
    kid, c = _coef(kernel, sigma)
    Xf, Zf = _rows(X, "X"), _rows(Z, "Z")
    d = Xf.shape[1]
    if Zf.shape[1] != d:
        raise ValueError(f"X has {d} coordinates and Z has {Zf.shape[1]}")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d = {d} is outside [1, {MAX_D}]")
    for A, name in ((Xf, "X"), (Zf, "Z")):
        if A.shape[0] < 2:
            raise ValueError(f"{name} has {A.shape[0]} row(s): a quadruple needs two points of "
                             f"each sample")
    if max(Xf.shape[0], Zf.shape[0]) >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows per sample")
    return Xf, Zf, kid, c


def _resolve(Xf, Zf, kernel, sigma, c):
    """(sigma, c) as numbers: sigma="median" (c is None) becomes the pooled median distance of the
    checked rows — device work, so callers finish their argument checks first and call this once,
    before any shuffle or draw.  Any other sigma is returned as it is."""
    if c is not None:
        return sigma, c
    from .bandwidth import _median_sigma
    sigma = _median_sigma(Xf, Zf, "pooled", "the pooled sample")
    return sigma, _coef(kernel, sigma)[1]


def _value(sxx, szz, sxz, n: int, m: int, kid: int) -> np.float64:
    v = 2.0 * sxx / (n * (n - 1)) + 2.0 * szz / (m * (m - 1)) - 2.0 * sxz / (n * m)
    return np.float64(v if kid == L.TW_MMD_GAUSSIAN else -v)


def _value_indexed(s, B: int, kid: int) -> np.float64:
    v = (s[0] + s[1] - s[2] - s[3]) / B
    return np.float64(v if kid == L.TW_MMD_GAUSSIAN else -v)


# ------------------------------------------------------------------------------ device glue
def _sums_blocks(Xf, Zf, bxo, bzo, kid, c):
    """tw_mmd_sums on one upload: the (n_blocks, 3) doubles Sxx, Szz, Sxz of the blocks b = rows
    [bxo[b], bxo[b + 1]) of Xf against rows [bzo[b], bzo[b + 1]) of Zf."""
    t = L.torch()
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb = len(bxo) - 1
    max_n, max_m = int(np.diff(bxo).max()), int(np.diff(bzo).max())
    xd, zd, bx, bz = L.to_device_many([Xf.reshape(-1), Zf.reshape(-1), bxo, bzo])
    work = L.empty((max(1, int(L.lib().tw_mmd_work_bytes(nb, max_n, max_m)) // 8),), t.float64)
    out = L.empty((nb, 3), t.float64)
    L.call("tw_mmd_sums", xd, zd, Xf.shape[1], bx, bz, nb, max_n, max_m, kid, c, work, out,
           L.stream_handle())
    return out.cpu().numpy()


def _sums_indexed(Xf, Zf, ii, jj, kk, ll, quad_off, kid, c):
    """tw_mmd_idx32 on one upload: the (n_shards, 4) doubles of the given quadruples (absolute
    rows)."""
    t = L.torch()
    L.device()
    quad_off = np.asarray(quad_off, dtype=np.int64)
    ns = len(quad_off) - 1
    xd, zd, id_, jd, kd, ld, od = L.to_device_many(
        [Xf.reshape(-1), Zf.reshape(-1), ii.astype(np.int32), jj.astype(np.int32),
         kk.astype(np.int32), ll.astype(np.int32), quad_off])
    max_q = int(np.diff(quad_off).max()) if ns else 0
    work = L.empty((max(1, int(L.lib().tw_mmd_idx_work_bytes(ns, max_q)) // 8),), t.float64)
    out = L.empty((ns, 4), t.float64)
    L.call("tw_mmd_idx32", xd, zd, Xf.shape[1], id_, jd, kd, ld, od, ns, max_q, kid, c, work, out,
           L.stream_handle())
    return out.cpu().numpy()


# ------------------------------------------------------------------------------- estimators
def components(X, Z, kernel="gaussian", sigma=None):
    """(Sxx, Szz, Sxz): the three sums of g over the pairs of X, the pairs of Z and all (x, z)."""
    Xf, Zf, kid, c = _check(X, Z, kernel, sigma)
    _, c = _resolve(Xf, Zf, kernel, sigma, c)
    s = _sums_blocks(Xf, Zf, [0, Xf.shape[0]], [0, Zf.shape[0]], kid, c)[0]
    return np.float64(s[0]), np.float64(s[1]), np.float64(s[2])


def Un(X, Z, kernel="gaussian", sigma=None):
    """The complete statistic: MMD^2_u (Gaussian) or the energy distance."""
    Xf, Zf, kid, c = _check(X, Z, kernel, sigma)
    _, c = _resolve(Xf, Zf, kernel, sigma, c)
    sxx, szz, sxz = _sums_blocks(Xf, Zf, [0, Xf.shape[0]], [0, Zf.shape[0]], kid, c)[0]
    return _value(sxx, szz, sxz, Xf.shape[0], Zf.shape[0], kid)


def UB_indices(X, Z, i, j, k, l, kernel="gaussian", sigma=None):  # noqa: E741
    """The mean of h over the given quadruples ((x_i[p], x_j[p]), (z_k[p], z_l[p])), i[p] != j[p]
    and k[p] != l[p]."""
    Xf, Zf, kid, c = _check(X, Z, kernel, sigma)
    n, m = Xf.shape[0], Zf.shape[0]
    i, j = _check_index(np.asarray(i), n), _check_index(np.asarray(j), n)
    k, l = _check_index(np.asarray(k), m), _check_index(np.asarray(l), m)  # noqa: E741
    if not i.shape == j.shape == k.shape == l.shape:
        raise ValueError(f"operands could not be broadcast together with shapes "
                         f"{i.shape} {j.shape} {k.shape} {l.shape}")
    i, j, k, l = (a.reshape(-1) for a in (i, j, k, l))  # noqa: E741
    if np.any(i == j) or np.any(k == l):  # (rows as _check_index returns them, >= 0)
        raise ValueError("a quadruple needs i != j and k != l")
    _, c = _resolve(Xf, Zf, kernel, sigma, c)
    if i.size == 0:
        return np.float64("nan")  # the mean of no terms
    s = _sums_indexed(Xf, Zf, i, j, k, l, [0, i.size], kid, c)[0]
    return _value_indexed(s, i.size, kid)


def _pairs_from(a, b):
    return a, b + (b >= a)


def _draw_quadruples(n: int, m: int, B: int):
    """B quadruples, uniform over i != j and k != l: i = randint(0, n, B); j = randint(0, n - 1,
    B); j += (j >= i); k = randint(0, m, B); l = randint(0, m - 1, B); l += (l >= k) — from the
    global legacy RNG, in this order."""
    try:  # the same four calls (values and state) in one native call
        i, j, k, l = randint_batch([(0, n, B), (0, n - 1, B), (0, m, B), (0, m - 1, B)])  # noqa: E741
    except NotImplementedError:  # the global generator is not the legacy MT19937
        i = np.random.randint(0, n, B)
        j = np.random.randint(0, n - 1, B)
        k = np.random.randint(0, m, B)
        l = np.random.randint(0, m - 1, B)  # noqa: E741
    return _pairs_from(i, j) + _pairs_from(k, l)


def UB(X, Z, B, kernel="gaussian", sigma=None):
    """The incomplete statistic: B quadruples drawn with replacement."""
    Xf, Zf, _, c = _check(X, Z, kernel, sigma)
    sigma, _ = _resolve(Xf, Zf, kernel, sigma, c)
    i, j, k, l = _draw_quadruples(Xf.shape[0], Zf.shape[0], int(B))  # noqa: E741
    return UB_indices(Xf, Zf, i, j, k, l, kernel, sigma)


class _Complete:
    """Tag of a block function made by UnN: every block's Un, all blocks in one tw_mmd_sums
    launch."""

    def __init__(self, kernel, sigma):
        self.kid, self.c = _coef(kernel, sigma)

    def evaluate(self, Xf, Zf, k, kz, N):
        s = _sums_blocks(Xf[:N * k], Zf[:N * kz], np.arange(N + 1) * k, np.arange(N + 1) * kz,
                         self.kid, self.c)
        return [_value(b[0], b[1], b[2], k, kz, self.kid) for b in s]


class _Incomplete:
    """Tag of a block function made by UnNB: every block's UB, the draws in block order (i, j,
    k, l for each block), all blocks in one tw_mmd_idx32 launch."""

    def __init__(self, B, kernel, sigma):
        self.B = int(B)
        self.kid, self.c = _coef(kernel, sigma)

    def evaluate(self, Xf, Zf, k, kz, N):
        B = self.B
        try:  # the 4N calls of the N blocks, in their order, in one native call
            d = randint_batch([(0, k, B), (0, k - 1, B), (0, kz, B), (0, kz - 1, B)] * N)
            draws = [_pairs_from(d[4 * b], d[4 * b + 1]) + _pairs_from(d[4 * b + 2], d[4 * b + 3])
                     for b in range(N)]
        except NotImplementedError:  # the global generator is not the legacy MT19937
            draws = [_draw_quadruples(k, kz, B) for _ in range(N)]
        if B == 0:
            return [np.float64("nan")] * N
        ii = np.concatenate([q[0] + b * k for b, q in enumerate(draws)])
        jj = np.concatenate([q[1] + b * k for b, q in enumerate(draws)])
        kk = np.concatenate([q[2] + b * kz for b, q in enumerate(draws)])
        ll = np.concatenate([q[3] + b * kz for b, q in enumerate(draws)])
        s = _sums_indexed(Xf[:N * k], Zf[:N * kz], ii, jj, kk, ll, np.arange(N + 1) * B,
                          self.kid, self.c)
        return [_value_indexed(b, B, self.kid) for b in s]


def _block_fn(spec, fn):
    fn._tw_mmd_block = spec
    return fn


def _partition(X, Z, N, sampling_type):
    """UN's argument checks: (Xf, Zf, k, kz) or a ValueError, before any shuffle."""
    if sampling_type != "prop-SWOR":
        raise ValueError(f"sampling_type={sampling_type!r}: only the proportional partition "
                         f"without replacement ('prop-SWOR') is offered for the MMD; 'SWOR' and "
                         f"'prop-SWR' are out of scope (DESIGN.md §4.12)")
    if not isinstance(X, np.ndarray) or not isinstance(Z, np.ndarray):
        raise ValueError("UN shuffles the caller's NumPy arrays in place")
    Xf, Zf, _, _ = _check(X, Z, "energy", None)
    k, kz = int(Xf.shape[0] / N), int(Zf.shape[0] / N)
    if k < 2 or kz < 2:
        raise ValueError(f"N = {N} blocks of {k} row(s) of X and {kz} of Z: a block needs at "
                         f"least 2 rows of each sample")
    return Xf, Zf, k, kz


def _resolve_blocks(X, Z, N, sampling_type, kernel, sigma):
    """sigma of a block estimator as a number: for sigma="median" every check of the call (the
    rows, then UN's partition) runs first, then the median is taken once.  Any other sigma is
    returned as it is, with nothing checked here."""
    if not _is_median(sigma):
        return sigma
    Xf, Zf, _, c = _check(X, Z, kernel, sigma)
    if c is not None:
        return sigma
    _partition(X, Z, N, sampling_type)
    return _resolve(Xf, Zf, kernel, sigma, c)[0]


def UN(X, Z, N, f_block, sampling_type="prop-SWOR"):
    """Shuffles X, then Z, in place (rows), cuts N blocks of k = int(n / N) rows of X and
    kz = int(m / N) rows of Z (the remainders are left out) and averages f_block(x, z) over
    them.  Block functions made by this module (the closures of UnN / UnNB) are evaluated
    together on the device; any other callable is called block by block."""
    Xf, Zf, k, kz = _partition(X, Z, N, sampling_type)
    spec = getattr(f_block, "_tw_mmd_block", None)
    np.random.shuffle(X)
    np.random.shuffle(Z)
    if spec is not None:
        return np.mean(spec.evaluate(Xf, Zf, k, kz, N))  # Xf / Zf view the shuffled arrays
    return np.mean([f_block(X[b * k:(b + 1) * k], Z[b * kz:(b + 1) * kz]) for b in range(N)])


def UnN(X, Z, N, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Block-wise complete statistic."""
    sigma = _resolve_blocks(X, Z, N, sampling_type, kernel, sigma)

    def fun_block(x, z):
        return Un(x, z, kernel=kernel, sigma=sigma)

    _check(X, Z, kernel, sigma)
    return UN(X, Z, N, _block_fn(_Complete(kernel, sigma), fun_block), sampling_type)


def UnNB(X, Z, N, B, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Block-wise incomplete statistic."""
    sigma = _resolve_blocks(X, Z, N, sampling_type, kernel, sigma)

    def fun_block(x, z):
        return UB(x, z, B, kernel=kernel, sigma=sigma)

    _check(X, Z, kernel, sigma)
    return UN(X, Z, N, _block_fn(_Incomplete(B, kernel, sigma), fun_block), sampling_type)


def UnNT(X, Z, N, T, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Reshuffled block-wise complete statistic."""
    sigma = _resolve_blocks(X, Z, N, sampling_type, kernel, sigma)  # once, not per repetition
    return np.mean([UnN(X, Z, N, sampling_type, kernel, sigma) for _ in range(T)])


def UnNBT(X, Z, N, B, T, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """Reshuffled block-wise incomplete statistic."""
    sigma = _resolve_blocks(X, Z, N, sampling_type, kernel, sigma)  # once, not per repetition
    return np.mean([UnNB(X, Z, N, B, sampling_type, kernel, sigma) for _ in range(T)])


# ------------------------------------------------------------------------- permutation test
class PermutationResult(NamedTuple):
    """statistic: the observed value; null: the (n_perm,) values under the permutations;
    pvalue = (1 + #{null >= statistic}) / (1 + n_perm)."""
    statistic: np.float64
    null: np.ndarray
    pvalue: float


def _check_labels(labels, n: int, N: int):
    """labels as a (P, N) bool array with exactly n True a row, P >= 1, or a ValueError."""
    if not isinstance(labels, np.ndarray) or labels.dtype != np.bool_:
        raise ValueError("labels must be a NumPy bool array")
    if labels.ndim != 2 or labels.shape[1] != N or labels.shape[0] < 1:
        raise ValueError(f"labels has shape {labels.shape}: (P, n + m) = (P >= 1, {N}) expected")
    if labels.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 permutations")
    counts = labels.sum(axis=1)
    if np.any(counts != n):
        bad = int(np.flatnonzero(counts != n)[0])
        raise ValueError(f"labels[{bad}] marks {int(counts[bad])} rows, not the n = {n} of X")
    return labels


def _perm_sums(Xf, Zf, labels, kid, c):
    """tw_mmd_perm_sums on one upload: the (P, 3) doubles Sxx, Szz, Sxz of every row of labels."""
    t = L.torch()
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    P, N = labels.shape
    # bit b of word w of row r: permutation 32 w + b (little-endian words, zero padding)
    packed = np.packbits(labels.T, axis=1, bitorder="little")
    W = (P + 31) // 32
    words = np.zeros((N, 4 * W), dtype=np.uint8)
    words[:, :packed.shape[1]] = packed
    pool = np.concatenate([Xf, Zf]).reshape(-1)
    wd, ld = L.to_device_many([pool, words.view("<i4").reshape(-1)])
    work = L.empty((max(1, int(L.lib().tw_mmd_perm_work_bytes(N, P)) // 8),), t.float64)
    out = L.empty((P, 3), t.float64)
    L.call("tw_mmd_perm_sums", wd, N, Xf.shape[1], ld, P, kid, c, work, out, L.stream_handle())
    return out.cpu().numpy()


def permutation_sums(X, Z, labels, kernel="gaussian", sigma=None):
    """The (P, 3) float64 sums (Sxx, Szz, Sxz) of the P relabellings of the pooled sample
    W = [X; Z]: labels is a (P, n + m) bool array, row p marking the n rows of W that are the
    first sample under permutation p.  The device path of permutation_test with nothing drawn:
    one upload and one launch."""
    Xf, Zf, kid, c = _check(X, Z, kernel, sigma)
    labels = _check_labels(labels, Xf.shape[0], Xf.shape[0] + Zf.shape[0])
    _, c = _resolve(Xf, Zf, kernel, sigma, c)
    return _perm_sums(Xf, Zf, labels, kid, c)


def permutation_test(X, Z, n_perm, kernel="gaussian", sigma=None):
    """The permutation test of the complete statistic (MMD^2_u or the energy distance): the
    observed value, its n_perm values under uniform relabellings of the pooled sample and
    pvalue = (1 + #{null >= statistic}) / (1 + n_perm).

    Permutation p = 1 .. n_perm is pi = np.random.permutation(n + m) on NumPy's global legacy
    RNG, drawn in this order; its first sample is rows pi[:n] of the pool [X; Z].  X and Z are not
    modified.  The observed split is column 0 of the same launch, so `statistic` may differ from
    Un(X, Z) in the last bits (a different order of summation), while a permutation that
    reproduces the observed split gives exactly `statistic`."""
    if isinstance(n_perm, bool) or not isinstance(n_perm, (int, np.integer)) or n_perm < 1:
        raise ValueError(f"n_perm = {n_perm!r} must be an int >= 1")
    n_perm = int(n_perm)
    if n_perm >= 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 2 permutations")
    Xf, Zf, kid, c = _check(X, Z, kernel, sigma)
    _, c = _resolve(Xf, Zf, kernel, sigma, c)  # sigma="median": once, before any draw
    L.device()  # no HIP device: the package's RuntimeError, before any draw
    n, m = Xf.shape[0], Zf.shape[0]
    labels = np.zeros((n_perm + 1, n + m), dtype=np.bool_)
    labels[0, :n] = True
    for p in range(1, n_perm + 1):
        labels[p, np.random.permutation(n + m)[:n]] = True
    s = _perm_sums(Xf, Zf, labels, kid, c)
    values = np.asarray(_value(s[:, 0], s[:, 1], s[:, 2], n, m, kid), dtype=np.float64)
    statistic, null = np.float64(values[0]), values[1:].copy()
    return PermutationResult(statistic, null,
                             (1 + int(np.count_nonzero(null >= statistic))) / (1 + n_perm))
