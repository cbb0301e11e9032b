"""The variance of MMD^2_u (and of the energy distance) estimated from the sample, and the
bandwidth of a grid chosen by estimated test power (an extension).

X, Z, kernel and sigma are tuplewise.mmd's, checked by its own functions: everything that is a
ValueError in mmd.Un is one here, raised before any device work with the RNG untouched.  sigma
may also be a SEQUENCE of bandwidths (Gaussian kernel only; entries positive and finite, or the
string "median"): every result then has a leading axis of its length S.  sigma="median", alone
or as an entry, is resolved once per public call, before any shuffle.

The device (csrc/mmd_rows.hip, tw_mmd_rows) returns the row sums of g for every sigma of a launch,

    a_i = sum_{j != i} g(x_i, x_j)    r_i = sum_k g(x_i, z_k)
    q_k = sum_i g(x_i, z_k)           b_k = sum_{l != k} g(z_k, z_l)

each squared distance evaluated once and held while g is applied per sigma, so a term has the
bits tw_mmd_sums gives it.  The rest is float64 NumPy on those rows.  With

    phi_x[i] = a_i / (n - 1) - r_i / m        phi_z[k] = b_k / (m - 1) - q_k / n

(the Hajek projections of the statistic, up to a constant), value = mean(phi_x) + mean(phi_z) is
the statistic 2 Sxx / (n (n - 1)) + 2 Szz / (m (m - 1)) - 2 Sxz / (n m), zeta_x and zeta_z are the
sample variances (ddof = 1) of phi_x and phi_z, and

    var = 4 zeta_x / n + 4 zeta_z / m

is the first-order term of Var(MMD^2_u): the analogue of DeLong's components in
tuplewise.estimation.Un_var.  It omits the second-order term (of order 1 / n^2), which dominates
under the null where zeta -> 0.  For the energy kernel value, phi_x and phi_z are negated, as
mmd.Un negates its value.

select_sigma maximises the test-power criterion J(sigma) = value / sqrt(max(var, 0) + reg)
(Sutherland et al. 2017; Liu et al. 2020) over a grid.  A grid longer than
tw_mmd_rows_max_sigma() takes several launches of that size; a sigma's rows do not depend on the
other sigmas of its launch or on its position, so the split changes no number.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

from . import _lib as L
from . import mmd as _mmd


class RowSums(NamedTuple):
    """a, r: (n,) float64 — or (S, n) for a sequence of S sigmas; q, b: (m,) or (S, m)."""
    a: np.ndarray
    r: np.ndarray
    q: np.ndarray
    b: np.ndarray


class MMDVariance(NamedTuple):
    """value: the statistic; var = 4 zeta_x / n + 4 zeta_z / m; phi_x (n,), phi_z (m,): the
    components; zeta_x, zeta_z: their sample variances.  A leading S axis for a sequence."""
    value: np.ndarray
    var: np.ndarray
    phi_x: np.ndarray
    phi_z: np.ndarray
    zeta_x: np.ndarray
    zeta_z: np.ndarray


class SigmaSelection(NamedTuple):
    """sigma = the grid's entry at index = argmax criterion (a number, "median" resolved);
    criterion, value, var: (S,) float64."""
    sigma: float
    index: int
    criterion: np.ndarray
    value: np.ndarray
    var: np.ndarray


# ------------------------------------------------------------------------------ host checks
def _is_grid(sigma) -> bool:
    return isinstance(sigma, (list, tuple, np.ndarray)) and not (
        isinstance(sigma, np.ndarray) and sigma.ndim == 0)


def _check(X, Z, kernel, sigma):
    """(Xf, Zf, kernel id, sigmas, cs, grid) or a ValueError, before anything touches a device or
    the RNG: sigmas the entries as given, cs their coefficients (None where "median")."""
    grid = _is_grid(sigma)
    if grid:
        if isinstance(sigma, np.ndarray) and sigma.ndim != 1:
            raise ValueError(f"a grid of sigmas is one-dimensional, not of shape {sigma.shape}")
        sigmas = list(sigma)
        if kernel == "energy":
            raise ValueError("the energy kernel takes no sigma")
        if not sigmas and kernel in _mmd._KERNELS:
            raise ValueError("the grid of sigmas is empty")
    else:
        sigmas = [sigma]
    cs = [_mmd._coef(kernel, s)[1] for s in sigmas]
    Xf, Zf, kid, _ = _mmd._check(X, Z, kernel, sigmas[0] if sigmas else None)
    return Xf, Zf, kid, sigmas, cs, grid


def _resolve(Xf, Zf, kernel, sigmas, cs):
    """sigmas and cs as numbers: every "median" entry becomes the pooled median distance, taken
    once (device work: after every check, before any shuffle)."""
    if all(c is not None for c in cs):
        return sigmas, cs
    med, c_med = _mmd._resolve(Xf, Zf, kernel, "median", None)
    return ([med if c is None else s for s, c in zip(sigmas, cs)],
            [c_med if c is None else c for c in cs])


# ------------------------------------------------------------------------------ device glue
def _rows_blocks(Xf, Zf, bxo, bzo, kid, cs):
    """tw_mmd_rows on one upload and ONE launch: (rows_x, rows_z) of shapes (S, nx, 2) and
    (S, nz, 2) for the blocks b = rows [bxo[b], bxo[b + 1]) of Xf against [bzo[b], bzo[b + 1]) of
    Zf and the S = len(cs) <= tw_mmd_rows_max_sigma() coefficients; [..., 0] and [..., 1] as
    include/tuplewise.h orders them (a, r and q, b)."""
    t = L.torch()
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb, S = len(bxo) - 1, len(cs)
    max_n, max_m = int(np.diff(bxo).max()), int(np.diff(bzo).max())
    nx, nz = int(bxo[-1]), int(bzo[-1])
    xd, zd, bx, bz, cd = L.to_device_many(
        [Xf.reshape(-1), Zf.reshape(-1), bxo, bzo, np.asarray(cs, dtype=np.float64)])
    nbytes = int(L.lib().tw_mmd_rows_work_bytes(nb, max_n, max_m, S))
    if nbytes == 0:
        raise ValueError(f"tw_mmd_rows refuses {nb} block(s) of up to {max_n} x {max_m} rows at "
                         f"{S} sigma(s): its partials would pass 1 GiB")
    work = L.empty((nbytes // 8,), t.float64)
    rx, rz = L.empty((S, nx, 2), t.float64), L.empty((S, nz, 2), t.float64)
    L.call("tw_mmd_rows", xd, zd, Xf.shape[1], bx, bz, nb, max_n, max_m, kid, cd, S, work, rx, rz,
           L.stream_handle())
    return rx.cpu().numpy(), rz.cpu().numpy()


def _rows_grid(Xf, Zf, bxo, bzo, kid, cs):
    """_rows_blocks for a grid of any length: launches of tw_mmd_rows_max_sigma() sigmas."""
    step = int(L.lib().tw_mmd_rows_max_sigma())
    parts = [_rows_blocks(Xf, Zf, bxo, bzo, kid, cs[s0:s0 + step])
             for s0 in range(0, len(cs), step)]
    if len(parts) == 1:
        return parts[0]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _variance(a, r, q, b, kid):
    """MMDVariance of rows with a trailing axis of n (a, r) and m (q, b) and any leading axes."""
    n, m = a.shape[-1], b.shape[-1]
    sign = 1.0 if kid == L.TW_MMD_GAUSSIAN else -1.0
    with np.errstate(invalid="ignore", over="ignore"):
        phi_x = sign * (a / (n - 1) - r / m)
        phi_z = sign * (b / (m - 1) - q / n)
        mx, mz = phi_x.mean(axis=-1), phi_z.mean(axis=-1)
        zeta_x = ((phi_x - mx[..., None]) ** 2).sum(axis=-1) / (n - 1)
        zeta_z = ((phi_z - mz[..., None]) ** 2).sum(axis=-1) / (m - 1)
        return MMDVariance(mx + mz, 4.0 * zeta_x / n + 4.0 * zeta_z / m, phi_x, phi_z, zeta_x,
                           zeta_z)


# ------------------------------------------------------------------------------- public
def row_sums(X, Z, kernel="gaussian", sigma=None):
    """RowSums(a, r, q, b) of the whole samples; a sequence of S sigmas gives (S, n) and (S, m)."""
    Xf, Zf, kid, sigmas, cs, grid = _check(X, Z, kernel, sigma)
    _, cs = _resolve(Xf, Zf, kernel, sigmas, cs)
    rx, rz = _rows_grid(Xf, Zf, [0, Xf.shape[0]], [0, Zf.shape[0]], kid, cs)
    out = (rx[..., 0], rx[..., 1], rz[..., 0], rz[..., 1])
    return RowSums(*(np.ascontiguousarray(v if grid else v[0]) for v in out))


def Un_var(X, Z, kernel="gaussian", sigma=None):
    """The complete statistic and its first-order variance estimate from the sample."""
    Xf, Zf, kid, sigmas, cs, grid = _check(X, Z, kernel, sigma)
    _, cs = _resolve(Xf, Zf, kernel, sigmas, cs)
    rx, rz = _rows_grid(Xf, Zf, [0, Xf.shape[0]], [0, Zf.shape[0]], kid, cs)
    v = _variance(rx[..., 0], rx[..., 1], rz[..., 0], rz[..., 1], kid)
    if grid:
        return v
    return MMDVariance(np.float64(v.value[0]), np.float64(v.var[0]), v.phi_x[0], v.phi_z[0],
                       np.float64(v.zeta_x[0]), np.float64(v.zeta_z[0]))


def UnN_var(X, Z, N, sampling_type="prop-SWOR", kernel="gaussian", sigma=None):
    """(value, var) of the block-wise complete statistic: mmd.UnN's shuffles and blocks (the RNG
    is consumed identically and X, Z are left as mmd.UnN leaves them), all N blocks through one
    tw_mmd_rows launch; value is the mean of the blocks' values, var the mean of the blocks' var
    divided by N (the blocks are disjoint).  sigma is one bandwidth, not a sequence."""
    if _is_grid(sigma):
        raise ValueError("UnN_var takes one sigma, not a sequence")
    sigma = _mmd._resolve_blocks(X, Z, N, sampling_type, kernel, sigma)
    _, _, kid, c = _mmd._check(X, Z, kernel, sigma)
    Xf, Zf, k, kz = _mmd._partition(X, Z, N, sampling_type)
    np.random.shuffle(X)
    np.random.shuffle(Z)
    rx, rz = _rows_blocks(Xf[:N * k], Zf[:N * kz], np.arange(N + 1) * k, np.arange(N + 1) * kz,
                          kid, [c])  # Xf / Zf view the shuffled arrays
    rx, rz = rx[0].reshape(N, k, 2), rz[0].reshape(N, kz, 2)
    v = _variance(rx[..., 0], rx[..., 1], rz[..., 0], rz[..., 1], kid)
    return np.float64(np.mean(v.value)), np.float64(np.mean(v.var) / N)


def select_sigma(X, Z, sigmas, reg=1e-8, kernel="gaussian"):
    """The sigma of the grid that maximises criterion[s] = value[s] / sqrt(max(var[s], 0) + reg);
    the first on ties; a NaN criterion never wins and an all-NaN grid is a ValueError."""
    if kernel != "gaussian":
        raise ValueError(f"kernel={kernel!r}: select_sigma is offered for the Gaussian kernel only")
    if not _is_grid(sigmas):
        raise ValueError("sigmas must be a sequence of bandwidths")
    try:
        reg = float(reg)
    except (TypeError, ValueError):
        raise ValueError(f"reg={reg!r} is not a number") from None
    if not (math.isfinite(reg) and reg >= 0.0):
        raise ValueError(f"reg = {reg} must be finite and >= 0")
    Xf, Zf, _, grid, cs, _ = _check(X, Z, kernel, sigmas)
    grid, _ = _resolve(Xf, Zf, kernel, grid, cs)
    v = Un_var(Xf, Zf, kernel, grid)
    with np.errstate(invalid="ignore", divide="ignore"):
        crit = v.value / np.sqrt(np.maximum(v.var, 0.0) + reg)
    if np.isnan(crit).all():
        raise ValueError("every criterion of the grid is NaN")
    index = int(np.nanargmax(crit))
    return SigmaSelection(float(grid[index]), index, crit, v.value, v.var)
