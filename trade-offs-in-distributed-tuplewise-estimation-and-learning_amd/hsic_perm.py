"""The permutation test of tuplewise.hsic's complete statistic on MI355X (an extension; the
reference has none): HSIC_u or the unbiased squared distance covariance under n_perm permutations
of the pairing, all in one launch (csrc/hsic_perm.hip).

The sample, the kernels and every argument check are tuplewise.hsic's.  Under a permutation pi of
the pairing, (X[i], Y[pi[i]]), only two of that module's eight sums move,

    S_p = sum over i < j of K_ij L_{pi(i) pi(j)}      Rab_p = sum over i of k_i l_{pi(i)}

so the device evaluates one side once per group of permutations and the other side per
permutation on gathered rows; the row sums k, l and R_K, R_L come from one tw_hsic_sums call on
the unpermuted sample, and the value of a permutation is hsic's U(S_p, R_K, R_L, Rab_p) in Python
floats.  The host owns the draws (NumPy's global legacy RNG, in NumPy's order), the device the
arithmetic.  (tuplewise.hsic itself keeps its surface: this module adds to it, as a sibling.)

sigma="median" (for both sides, or inside a pair such as ("median", 2.0)) is tuplewise.hsic's: each
such side's exact median distance over the pairs of its own rows, resolved once per call after
every argument check and before the first draw.  A permutation of the pairing reorders one side's
rows and leaves both medians as they are, so the observed column and every null column use the same
two bandwidths.  With "median" a non-finite entry on that side is a ValueError (with a numeric sigma
a NaN propagates instead), and so is a median of 0.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from . import _lib as L
from .hsic import _check, _resolve, _u, _work_bytes


class PermutationResult(NamedTuple):
    """statistic: the observed value; null: the (n_perm,) values under the permutations;
    pvalue = (1 + #{null >= statistic}) / (1 + n_perm)."""
    statistic: np.float64
    null: np.ndarray
    pvalue: float


def _check_perms(perms, n: int):
    """perms as a (P, n) integer array, P >= 1, every row a permutation of range(n), or a
    ValueError (a scatter into a bool array: no sort)."""
    if not isinstance(perms, np.ndarray) or perms.dtype.kind not in "iu":
        raise ValueError("perms must be a NumPy integer array")
    if perms.ndim != 2 or perms.shape[1] != n or perms.shape[0] < 1:
        raise ValueError(f"perms has shape {perms.shape}: (P, n) = (P >= 1, {n}) expected")
    if perms.shape[0] >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 permutations")
    if perms.min() < 0 or perms.max() >= n:
        bad = int(np.flatnonzero(((perms < 0) | (perms >= n)).any(axis=1))[0])
        raise ValueError(f"perms[{bad}] has an entry outside [0, {n})")
    seen = np.zeros(perms.shape, dtype=np.bool_)
    seen[np.arange(perms.shape[0])[:, None], perms] = True
    if not seen.all():
        bad = int(np.flatnonzero(~seen.all(axis=1))[0])
        raise ValueError(f"perms[{bad}] repeats a row: not a permutation of range({n})")
    return perms


def _perm_sums(Xf, Yf, perms, kid, cx, cy, wgs=0):
    """One upload, one tw_hsic_sums call on the unpermuted sample (its eight sums and the row
    sums) and one tw_hsic_perm_sums launch: the (P, 2) doubles S_p, Rab_p of the rows of perms
    (row p pairs X[i] with Y[perms[p, i]]) and the eight sums.  The side of fewer columns moves
    (Y if dy <= dx, by the rows of perms; else X, by their inverses): a host decision that depends
    on (dx, dy) alone."""
    t = L.torch()
    n, P = Xf.shape[0], perms.shape[0]
    nbytes = _work_bytes(1, n)
    pbytes = int(L.lib().tw_hsic_perm_work_bytes(n, P, wgs))
    if pbytes == 0:
        raise ValueError(f"{P} permutation(s) of {n} rows: the launch is refused (DESIGN.md §4.15)")
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    move_y = Yf.shape[1] <= Xf.shape[1]
    if move_y:
        idx = perms.astype(np.int32, copy=False)
    else:
        idx = np.empty(perms.shape, dtype=np.int32)
        idx[np.arange(P)[:, None], perms] = np.arange(n, dtype=np.int32)
    xd, yd, od, idd = L.to_device_many(
        [Xf.reshape(-1), Yf.reshape(-1), np.array([0, n], dtype=np.int64), idx.reshape(-1)])
    work = L.empty((max(nbytes, pbytes) // 8,), t.float64)
    comp = L.empty((1, 8), t.float64)
    rows = L.empty((n, 2), t.float64)
    L.call("tw_hsic_sums", xd, Xf.shape[1], yd, Yf.shape[1], od, 1, n, kid, cx, cy, 0, work, rows,
           comp, L.stream_handle())
    rows = rows.t().contiguous()  # (2, n): k, then l
    out = L.empty((P, 2), t.float64)
    if move_y:
        args = (xd, Xf.shape[1], yd, Yf.shape[1], n, idd, P, rows[0], rows[1], kid, cx, cy)
    else:
        args = (yd, Yf.shape[1], xd, Xf.shape[1], n, idd, P, rows[1], rows[0], kid, cy, cx)
    L.call("tw_hsic_perm_sums", *args, wgs, work, out, L.stream_handle())
    return out.cpu().numpy(), comp.cpu().numpy()[0]


def permutation_sums(X, Y, perms, kernel="gaussian", sigma=None):
    """The (P, 2) float64 sums (S_p, Rab_p) of P permutations of the pairing: perms is a (P, n)
    integer array, row p meaning "row i of the permuted sample is (X[i], Y[perms[p, i]])";
    S_p = sum over i < j of K_ij L_{perms[p, i], perms[p, j]} and Rab_p = sum over i of
    k_i l_{perms[p, i]}.  Every row must be a permutation of range(n) (a ValueError before any
    device work).  The device path of permutation_test with nothing drawn: one upload."""
    Xf, Yf, kid, cx, cy = _check(X, Y, kernel, sigma)
    perms = _check_perms(perms, Xf.shape[0])
    _, cx, cy = _resolve(Xf, Yf, sigma, cx, cy)
    return _perm_sums(Xf, Yf, perms, kid, cx, cy)[0]


def permutation_test(X, Y, n_perm, kernel="gaussian", sigma=None):
    """The permutation test of the complete statistic (HSIC_u or dCov^2_u): the observed value,
    its n_perm values under uniform permutations of the pairing and
    pvalue = (1 + #{null >= statistic}) / (1 + n_perm).

    Permutation p = 1 .. n_perm is pi = np.random.permutation(n) on NumPy's global legacy RNG,
    drawn in this order; its sample is (X[i], Y[pi[i]]).  X and Y are not modified.  The observed
    pairing is column 0 (the identity) of the same launch, so `statistic` may differ from
    Un(X, Y) in the last bits (a different order of summation), while a drawn permutation equal to
    the identity gives exactly `statistic`.  A NaN coordinate gives a NaN statistic, an all-NaN
    null and pvalue 1 / (n_perm + 1) (no comparison with NaN holds), as in tuplewise.mmd.  The
    permutation p-value of `correlation` is this one: its denominator is invariant and positive."""
    if isinstance(n_perm, bool) or not isinstance(n_perm, (int, np.integer)) or n_perm < 1:
        raise ValueError(f"n_perm = {n_perm!r} must be an int >= 1")
    n_perm = int(n_perm)
    if n_perm >= 2 ** 31 - 1:
        raise ValueError("at most 2^31 - 2 permutations")
    Xf, Yf, kid, cx, cy = _check(X, Y, kernel, sigma)
    n = Xf.shape[0]
    _work_bytes(1, n)  # a refused shape: a ValueError before the draws
    _, cx, cy = _resolve(Xf, Yf, sigma, cx, cy)  # a "median" side: once, before any draw
    L.device()  # no HIP device: the package's RuntimeError, before any draw
    perms = np.empty((n_perm + 1, n), dtype=np.int32)
    perms[0] = np.arange(n, dtype=np.int32)
    for p in range(1, n_perm + 1):
        perms[p] = np.random.permutation(n)
    s, comp = _perm_sums(Xf, Yf, perms, kid, cx, cy)
    values = np.array([_u(sp, comp[3], comp[4], rab, n) for sp, rab in s], dtype=np.float64)
    statistic, null = np.float64(values[0]), values[1:].copy()
    return PermutationResult(statistic, null,
                             (1 + int(np.count_nonzero(null >= statistic))) / (1 + n_perm))
