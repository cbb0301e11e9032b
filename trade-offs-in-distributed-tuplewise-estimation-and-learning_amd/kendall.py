"""Kendall tau matrices over many columns on MI355X (an extension; the reference has none).

tuplewise.onesample takes Kendall's tau of ONE pair of columns, an (n, 2) sample.  This module
takes all pairs of columns of an (n, p) table at once.  With s_a(i, j) = sign(S[i, a] - S[j, a]),

    M[a, b] = sum_{i<j} s_a(i, j) s_b(i, j)      C - D of columns a and b
    U_a     = M[a, a]                            the pairs not tied in column a
    tau-a   = M[a, b] / P,  P = n (n - 1) / 2
    tau-b   = M[a, b] / (sqrt(U_a) sqrt(U_b))

so the whole matrix is Sgn^T Sgn of a (pairs x p) sign matrix.  csrc/kendall.hip replaces every
column by its strict-less ranks (tw_col_ranks; a sign then costs a few 16-bit integer
instructions and is the same for float64 and int64) and multiplies the signs, generated on the
fly, on the int8 matrix unit (tw_kendall_matrix).  All results are exact integers; the float
expressions below are those of onesample._tau_a and onesample.kendall_tau_b, so an entry equals
the (n, 2) functions bit for bit.

All functions take host NumPy arrays: S is (n, p), float64 or int64 (compared as int64, never
converted), C-contiguous, n >= 2, 1 <= p <= 1024; Y, where given, has the same n and the same
rules.  A NaN has no rank: it raises a ValueError (the (n, 2) Kendall of tuplewise.onesample
keeps NumPy's comparison semantics for NaN).  DESIGN.md §4.18 lists what is out of scope.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib as L

MAX_COLUMNS = 1024
_VARIANTS = ["a", "b"]


class SignCounts(NamedTuple):
    M: np.ndarray    # (p, q) int64: C - D of column a of S and column b of Y
    Us: np.ndarray   # (p,) int64: pairs not tied in each column of S
    Uy: np.ndarray   # (q,) int64: the same for Y
    pairs: int       # n (n - 1) / 2


# ------------------------------------------------------------------------------ host checks
def _table(S, name="S"):
    S = np.asarray(S)
    if S.ndim != 2:
        raise ValueError(f"{name} is an (n, p) table, not shape {S.shape}")
    if S.dtype not in (np.float64, np.int64):
        raise ValueError(f"{name} holds float64 or int64 values, not {S.dtype}")
    if not S.flags.c_contiguous:
        raise ValueError(f"{name} must be a C-contiguous (n, p) array")
    n, p = S.shape
    if n < 2:
        raise ValueError(f"a sample of {n} row(s) has no pairs (at least 2 are needed)")
    if not 1 <= p <= MAX_COLUMNS:
        raise ValueError(f"{name} has {p} columns (1 to {MAX_COLUMNS})")
    if S.dtype == np.float64 and np.isnan(S).any():
        raise ValueError(f"{name} holds a NaN: ranks are undefined (the (n, 2) Kendall of "
                         "tuplewise.onesample keeps NumPy's comparison semantics for NaN)")
    return S


def _tables(S, Y):
    S = _table(S)
    if Y is None:
        return S, None
    Y = _table(Y, "Y")
    if Y.shape[0] != S.shape[0]:
        raise ValueError(f"Y has {Y.shape[0]} rows, S has {S.shape[0]}")
    return S, Y


def _check_variant(variant):
    if variant not in _VARIANTS:
        raise ValueError(f"variant={variant!r} is not one of {_VARIANTS}")
    return variant


def _pairs(n: int) -> int:
    return n * (n - 1) // 2


def _code(A):
    return L.TW_F64 if A.dtype == np.float64 else L.TW_I64


# ------------------------------------------------------------------------------ device glue
def _ranks_device(xd, od, n_shards, total, max_n, p, code, width):
    """tw_col_ranks on resident rows: the rank image tensor."""
    t = L.torch()
    need = int(L.lib().tw_col_ranks_work_bytes(n_shards, total, max_n, p))
    work = L.empty((max(1, need // 8),), t.int64)
    ranks = L.empty((max(1, total * p),), t.int16 if width == 16 else t.int32)
    L.call("tw_col_ranks", xd, od, n_shards, total, max_n, p, code, width, work, ranks,
           L.stream_handle())
    return ranks


def _matrix_device(ra, pa, rb, pb, od, n_shards, max_n, width):
    """tw_kendall_matrix on resident rank images: (M, Ua, Ub) tensors."""
    t = L.torch()
    need = int(L.lib().tw_kendall_matrix_work_bytes(n_shards, pa, pb))
    work = L.empty((max(1, need // 8),), t.int64)
    M = L.empty((n_shards, pa, pb), t.int64)
    Ua = L.empty((n_shards, pa), t.int64)
    Ub = L.empty((n_shards, pb), t.int64)
    L.call("tw_kendall_matrix", ra, pa, rb, pb, od, n_shards, max_n, width, work, M, Ua, Ub,
           L.stream_handle())
    return M, Ua, Ub


def _launch(X, Y, off):
    """One tw_col_ranks per table and one tw_kendall_matrix for all shards of `off` (row
    offsets into X and Y): (M (shards, p, q), Ua (shards, p), Ub (shards, q)) int64, on the
    host."""
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    n_shards = len(off) - 1
    total = int(off[-1] - off[0])
    max_n = int(np.diff(off).max()) if n_shards else 0
    width = int(L.lib().tw_kendall_matrix_width(max_n))
    p = X.shape[1]
    if Y is None:
        xd, od = L.to_device_many([X.reshape(-1), off])
        ra = _ranks_device(xd, od, n_shards, total, max_n, p, _code(X), width)
        rb, q = ra, p
    else:
        q = Y.shape[1]
        xd, yd, od = L.to_device_many([X.reshape(-1), Y.reshape(-1), off])
        ra = _ranks_device(xd, od, n_shards, total, max_n, p, _code(X), width)
        rb = _ranks_device(yd, od, n_shards, total, max_n, q, _code(Y), width)
    M, Ua, Ub = _matrix_device(ra, p, rb, q, od, n_shards, max_n, width)
    return M.cpu().numpy(), Ua.cpu().numpy(), Ub.cpu().numpy()


# ------------------------------------------------------------------------------ statistics
def sign_counts(S, Y=None) -> SignCounts:
    """The exact integers (M, Us, Uy, pairs) of S against Y (Y=None: S against itself, then
    M == M.T and Us == Uy == diag(M)).  S is not modified."""
    S, Y = _tables(S, Y)
    n = S.shape[0]
    M, Ua, Ub = _launch(S, Y, np.array([0, n], dtype=np.int64))
    return SignCounts(M[0], Ua[0], Ub[0], _pairs(n))


def _tau_a_matrix(M, pairs: int) -> np.ndarray:
    out = np.empty(M.shape, np.float64)
    for idx in np.ndindex(*M.shape):
        out[idx] = np.float64(int(M[idx]) / pairs)
    return out


def _tau_b_matrix(M, Us, Uy, symmetric: bool) -> np.ndarray:
    fx = [math.sqrt(float(u)) for u in Us]
    fy = [math.sqrt(float(u)) for u in Uy]
    out = np.empty(M.shape, np.float64)
    for a, b in np.ndindex(*M.shape):
        if fx[a] == 0.0 or fy[b] == 0.0:
            out[a, b] = np.float64("nan")
        elif symmetric and a == b:
            out[a, b] = 1.0
        else:
            out[a, b] = np.float64(int(M[a, b]) / (fx[a] * fy[b]))
    return out


def tau_matrix(S, Y=None, variant="b") -> np.ndarray:
    """The (p, q) float64 matrix of Kendall's tau-b (variant="b"; NaN where a column is
    constant, exactly 1.0 on the diagonal of the symmetric call otherwise) or tau-a
    (variant="a")."""
    _check_variant(variant)
    c = sign_counts(S, Y)
    if variant == "a":
        return _tau_a_matrix(c.M, c.pairs)
    return _tau_b_matrix(c.M, c.Us, c.Uy, Y is None)


def Un(S) -> np.ndarray:
    """The complete U-statistic of the sign-product kernel: the tau-a matrix."""
    return tau_matrix(S, variant="a")


def _block_size(S, N) -> int:
    if not isinstance(S, np.ndarray):
        raise TypeError("UnN shuffles the caller's NumPy array in place")
    N = int(N)
    if N < 1:
        raise ValueError(f"N={N} blocks (at least 1)")
    k = int(S.shape[0] / N)
    if k < 2:
        raise ValueError(f"a block of {k} row(s) has no pairs (at least 2 are needed)")
    return k


def _last_axis_mean(v) -> np.ndarray:
    """np.mean of every contiguous 1-D run along the first axis of v (N, p, p): the block axis
    moved last and made contiguous, so each entry is summed as np.mean sums a 1-D array
    (mean(axis=0) adds in another order and differs in the last bits from N = 8 on)."""
    return np.ascontiguousarray(np.moveaxis(np.asarray(v), 0, -1)).mean(axis=-1)


def _run(S, N, T):
    if not isinstance(S, np.ndarray):
        raise TypeError("UnN shuffles the caller's NumPy array in place")
    _table(S)
    N, T = int(N), int(T)
    k = _block_size(S, N)
    if T < 1:
        raise ValueError(f"T={T} shuffles (at least 1)")
    p = S.shape[1]
    snaps = []
    for t in range(T):
        np.random.shuffle(S)  # in place, on the rows
        used = S[:N * k]
        snaps.append(used if t + 1 == T else used.copy())
    X = snaps[0] if T == 1 else np.concatenate(snaps)
    off = np.arange(T * N + 1, dtype=np.int64) * k
    M, _, _ = _launch(np.ascontiguousarray(X), None, off)
    vals = np.stack([_tau_a_matrix(M[b], _pairs(k)) for b in range(T * N)])
    means = np.stack([_last_axis_mean(vals[t * N:(t + 1) * N]) for t in range(T)])
    return _last_axis_mean(means).reshape(p, p)


def UnN(S, N) -> np.ndarray:
    """Block-wise complete U-statistic: np.random.shuffle(S) on the rows in place, N blocks of
    k = int(n / N) rows (the remainder is left out), the mean of the blocks' tau-a matrices.
    All blocks run in one tw_col_ranks and one tw_kendall_matrix launch."""
    return _run(S, N, 1)


def UnNT(S, N, T) -> np.ndarray:
    """The mean of T UnN calls (T shuffles of S in place), the T x N blocks in one launch."""
    return _run(S, N, T)
