"""Sample variances, confidence intervals and z-scores for Kendall tau matrices on MI355X (an
extension; the reference has none).

tuplewise.kendall returns the tau-a / tau-b matrix of an (n, p) table as exact integers; this
module says how precise an entry is.  With s_a(i, j) = sign(S[i, a] - S[j, a]) and, per point,

    c_i(a, b) = sum_{j != i} s_a(i, j) s_b(i, j)        c_i(a, a) = u_i(a)

csrc/kendall_rows.hip (tw_kendall_rows, on the rank image of tw_col_ranks) returns four exact
(p, p) int64 matrices

    R = sum_i c_i (= 2 M of kendall.sign_counts)     Q = sum_i c_i^2
    F[a, b] = sum_i c_i(a, b) u_i(a)                 E[a, b] = sum_i u_i(a) u_i(b)

and the first-order (Hajek) variances are rationals in them.  With Sm = R[a, b], Sa = R[a, a],
Sb = R[b, b], Cmm = n Q[a, b] - Sm^2, Caa = n Q[a, a] - Sa^2, Cbb likewise, Cma = n F[a, b] - Sm Sa,
Cmb = n F[b, a] - Sm Sb, Cab = n E[a, b] - Sa Sb:

    var tau-a = 4 Cmm / (n^2 (n - 1)^3)              4 zeta_1 / n, zeta_1 the ddof = 1 sample
                                                     variance of c_i / (n - 1)
    var tau-b = NUM / ((n - 1) Sa^3 Sb^3)            the delta method on M / sqrt(U_a U_b)
    NUM = 4 Sa^2 Sb^2 Cmm - 4 Sm Sa Sb^2 Cma - 4 Sm Sa^2 Sb Cmb
          + Sm^2 Sb^2 Caa + Sm^2 Sa^2 Cbb + 2 Sm^2 Sa Sb Cab

Numerator and denominator are Python ints (object arrays) and each entry is ONE true division,
so it is the correctly rounded value of the expression.  tau is not degenerate under
independence (zeta_1 = 1/9), so the first-order term also holds at the null.

Inputs follow tuplewise.kendall's rules (host NumPy arrays, (n, p) float64 or int64,
C-contiguous, no NaN, 1 <= p <= 1024) and n <= 2^20 rows a shard; the symmetric case only.
DESIGN.md §4.19 lists what is out of scope.
"""
from __future__ import annotations

import statistics
from typing import NamedTuple

import numpy as np

from . import _lib as L
from . import kendall as K

MAX_ROWS = 1 << 20
_VARIANTS = K._VARIANTS


class RowMoments(NamedTuple):
    R: np.ndarray    # (p, p) int64: sum_i c_i(a, b) = 2 M[a, b]
    Q: np.ndarray    # (p, p) int64: sum_i c_i(a, b)^2
    F: np.ndarray    # (p, p) int64: sum_i c_i(a, b) c_i(a, a); not symmetric
    E: np.ndarray    # (p, p) int64: sum_i c_i(a, a) c_i(b, b)
    n: int


class TauVariance(NamedTuple):
    tau: np.ndarray  # (p, p) float64, bit-equal to kendall.tau_matrix
    var: np.ndarray  # (p, p) float64 estimated variance of tau
    se: np.ndarray   # sqrt(max(var, 0))


# ------------------------------------------------------------------------------ host checks
def _table(S):
    S = K._table(S)
    if S.shape[0] > MAX_ROWS:
        raise ValueError(f"S has {S.shape[0]} rows (at most 2^20: the sums of squares stay "
                         "below 2^63)")
    return S


def _check_level(level) -> float:
    level = float(level)
    if not 0.0 < level < 1.0:
        raise ValueError(f"level={level!r} is not inside (0, 1)")
    return level


# ------------------------------------------------------------------------------ device glue
def _rows_device(ra, p, od, n_shards, max_n, width):
    """tw_kendall_rows on a resident rank image: the (R, Q, F, E) tensors."""
    t = L.torch()
    need = int(L.lib().tw_kendall_rows_work_bytes(n_shards, p))
    work = L.empty((max(1, need // 8),), t.int64)
    out = [L.empty((n_shards, p, p), t.int64) for _ in range(4)]
    L.call("tw_kendall_rows", ra, p, od, n_shards, max_n, width, work, *out, L.stream_handle())
    return out


def _launch(X, off):
    """One tw_col_ranks and one tw_kendall_rows for all shards of `off` (row offsets into X):
    R, Q, F, E as (shards, p, p) int64 on the host."""
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    n_shards = len(off) - 1
    total = int(off[-1] - off[0])
    max_n = int(np.diff(off).max()) if n_shards else 0
    width = int(L.lib().tw_kendall_matrix_width(max_n))
    p = X.shape[1]
    xd, od = L.to_device_many([X.reshape(-1), off])
    ra = K._ranks_device(xd, od, n_shards, total, max_n, p, K._code(X), width)
    return tuple(m.cpu().numpy() for m in _rows_device(ra, p, od, n_shards, max_n, width))


# ------------------------------------------------------------------------------ expressions
def _obj(M):
    return np.asarray(M).astype(object)  # Python ints: no overflow, true division rounds once


def _var_a_matrix(R, Q, n: int) -> np.ndarray:
    R, Q = _obj(R), _obj(Q)
    num = 4 * (n * Q - R * R)
    return (num / (n * n * (n - 1) ** 3)).astype(np.float64)


def _var_b_matrix(R, Q, F, E, n: int) -> np.ndarray:
    R, Q, F, E = _obj(R), _obj(Q), _obj(F), _obj(E)
    d, qd = np.diagonal(R), np.diagonal(Q)
    Sm, Sa, Sb = R, d[:, None], d[None, :]
    Cmm = n * Q - Sm * Sm
    Caa, Cbb = (n * qd - d * d)[:, None], (n * qd - d * d)[None, :]
    Cma, Cmb, Cab = n * F - Sm * Sa, n * F.T - Sm * Sb, n * E - Sa * Sb
    Sm2, Sa2, Sb2 = Sm * Sm, Sa * Sa, Sb * Sb
    num = (4 * Sa2 * Sb2 * Cmm - 4 * Sm * Sa * Sb2 * Cma - 4 * Sm * Sa2 * Sb * Cmb
           + Sm2 * Sb2 * Caa + Sm2 * Sa2 * Cbb + 2 * Sm2 * Sa * Sb * Cab)
    den = (n - 1) * (Sa2 * Sa) * (Sb2 * Sb)
    const = (den == 0)  # a constant column: U = 0
    out = (num / np.where(const, 1, den)).astype(np.float64)
    out[const.astype(bool)] = np.nan
    return out


def _tau(R, n: int, variant) -> np.ndarray:
    M = np.asarray(R) // 2  # exact: every entry is even
    if variant == "a":
        return K._tau_a_matrix(M, K._pairs(n))
    U = np.diagonal(M)
    return K._tau_b_matrix(M, U, U, True)


def _var(m: RowMoments, variant) -> np.ndarray:
    if variant == "a":
        return _var_a_matrix(m.R, m.Q, m.n)
    return _var_b_matrix(m.R, m.Q, m.F, m.E, m.n)


# ------------------------------------------------------------------------------ statistics
def row_moments(S) -> RowMoments:
    """The exact integers (R, Q, F, E, n) of S.  S is not modified."""
    S = _table(S)
    n = S.shape[0]
    R, Q, F, E = _launch(S, np.array([0, n], dtype=np.int64))
    return RowMoments(R[0], Q[0], F[0], E[0], n)


def tau_var(S, variant="b") -> TauVariance:
    """(tau, var, se): the tau matrix of kendall.tau_matrix (bit-equal, from the same integers),
    its estimated variance (variant b: exactly 0.0 on the diagonal, NaN where a column is
    constant) and se = sqrt(max(var, 0))."""
    K._check_variant(variant)
    m = row_moments(S)
    var = _var(m, variant)
    return TauVariance(_tau(m.R, m.n, variant), var, np.sqrt(np.maximum(var, 0.0)))


def tau_ci(S, variant="b", level=0.95):
    """(tau, lo, hi): tau -+ z se with z the normal quantile of (1 + level) / 2, clipped to
    [-1, 1]."""
    K._check_variant(variant)
    z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * _check_level(level))
    tau, _, se = tau_var(S, variant)
    return tau, np.clip(tau - z * se, -1.0, 1.0), np.clip(tau + z * se, -1.0, 1.0)


def z_scores(S, variant="b") -> np.ndarray:
    """tau / se; +-inf or NaN where se is 0."""
    tau, _, se = tau_var(S, variant)
    with np.errstate(divide="ignore", invalid="ignore"):
        return tau / se


def UnN_var(S, N):
    """(value, var) of kendall.UnN: the same shuffle of S in place (same draws, same array left
    behind) and blocks, all N blocks in one tw_col_ranks and one tw_kendall_rows launch.  value
    is the block mean of tau-a, var the mean of the blocks' variances divided by N."""
    if not isinstance(S, np.ndarray):
        raise TypeError("UnN_var shuffles the caller's NumPy array in place")
    _table(S)
    N = int(N)
    k = K._block_size(S, N)
    p = S.shape[1]
    np.random.shuffle(S)  # in place, on the rows
    off = np.arange(N + 1, dtype=np.int64) * k
    R, Q, _, _ = _launch(np.ascontiguousarray(S[:N * k]), off)
    vals = np.stack([K._tau_a_matrix(R[b] // 2, K._pairs(k)) for b in range(N)])
    vars_ = np.stack([_var_a_matrix(R[b], Q[b], k) for b in range(N)])
    return (K._last_axis_mean(vals).reshape(p, p), K._last_axis_mean(vars_).reshape(p, p) / N)
