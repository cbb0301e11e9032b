"""One-sample pairwise U-statistics on MI355X (an extension; the reference has none).

Everything else in the package is a two-sample, degree-(1,1) statistic: one point of X against
one of Z.  The textbook U-statistics pair points of ONE sample S over the unordered pairs i < j:

  kernel      h(s_i, s_j)                              value
  "gini"      |s_i - s_j|                              float mean over pairs (Gini mean difference)
  "var"       (s_i - s_j)^2 / 2                        float mean = np.var(S, ddof=1) up to rounding
  "kendall"   +1 concordant, -1 discordant, 0 else     (C - D) / P = Kendall's tau-a, from exact
                                                       integers; S is (n, 2), a row one point (a, b)

The Kendall predicates are comparisons only, so NaN and +-0 behave as NumPy's >, < and ==:
concordant (a_i>a_j and b_i>b_j) or (a_i<a_j and b_i<b_j), discordant the two mixed cases,
Tx = #{a_i==a_j}, Ty = #{b_i==b_j}, Txy = #{both}, P = n(n-1)/2.

S is a host NumPy array: 1-D or (n, 1) for "gini" / "var" (other dtypes are converted with
np.asarray(S, np.float64)); (n, 2), C-contiguous, float64 or int64 for "kendall" (int64 is
compared as int64, never converted).  The estimators mirror compute_stats.py:95-123 with one
sample: UN shuffles the caller's array in place, cuts N blocks of k = int(n / N) points (a
remainder is left out, as prop-SWOR does) and averages the block values; all blocks of a block
function made here run in ONE launch of csrc/selfpairs.hip.  Only the partition without
replacement is offered (DESIGN.md §4.9 lists what is out of scope).

algo= chooses how the complete statistics are evaluated: "pairs" walks all n (n - 1) / 2 pairs
(csrc/selfpairs.hip), "sorted" sorts and searches (csrc/selfsorted.hip, DESIGN.md §4.9b: "gini"
and "kendall"), "auto" takes the sorted path once the largest shard has SORTED_MIN_N points.
Kendall's integers are the same either way, so its default is "auto"; the sorted Gini sum is
rounded once instead of block by block and differs in the last bits, so "gini" stays on "pairs"
unless asked.
"""
from __future__ import annotations

import math

import numpy as np

from . import _lib as L
from .compute_stats import _check_index
from .numpy_rng import randint_batch

_KERNELS = ["gini", "var", "kendall"]
_CODES = {"gini": L.TW_SELF_GINI, "var": L.TW_SELF_VAR, "kendall": L.TW_SELF_KENDALL}
_ALGOS = ["pairs", "sorted", "auto"]
# "auto": the largest shard's size from which the sorted path is taken (the smallest measured n
# at which it beats all pairs for one shard: tools/time_onesample.py)
SORTED_MIN_N = 100_000


# ------------------------------------------------------------------------------ host checks
def _items(S, kernel):
    """The sample as the device reads it: (flat 8-byte values, items, TW dtype code).  Raises
    before anything touches a device."""
    if kernel == "kendall":
        S = np.asarray(S)
        if S.ndim != 2 or S.shape[1] != 2:
            raise ValueError(f"kernel='kendall' takes an (n, 2) array of points (a, b), not "
                             f"shape {S.shape}")
        if S.dtype not in (np.float64, np.int64):
            raise ValueError(f"kernel='kendall' takes float64 or int64 points, not {S.dtype}")
        if not S.flags.c_contiguous:
            raise ValueError("kernel='kendall' takes a C-contiguous (n, 2) array")
        return S.reshape(-1), S.shape[0], (L.TW_F64 if S.dtype == np.float64 else L.TW_I64)
    S = np.asarray(S, np.float64)
    if S.ndim == 2 and S.shape[1] == 1:
        S = S.reshape(-1)
    if S.ndim != 1:
        raise ValueError(f"kernel={kernel!r} takes a 1-D or (n, 1) sample, not shape {S.shape}")
    return S, S.shape[0], L.TW_F64


def _check_algo(kernel, algo):
    """algo= as given by the caller (None: the kernel's default).  Raises before anything else
    happens."""
    if algo is None:
        return "auto" if kernel == "kendall" else "pairs"
    if algo not in _ALGOS:
        raise ValueError(f"algo={algo!r} is not one of {_ALGOS}")
    if algo == "sorted" and kernel == "var":
        raise ValueError("kernel='var' has no sorted path (np.var is the O(n) tool); use "
                         "algo='pairs'")
    return algo


def _choose_algo(kernel, algo, max_n) -> str:
    """"pairs" or "sorted" for a launch whose largest shard has max_n items."""
    algo = _check_algo(kernel, algo)
    if algo == "auto":
        return "sorted" if kernel != "var" and max_n >= SORTED_MIN_N else "pairs"
    return algo


def _need_pairs(n, what="sample"):
    if n < 2:
        raise ValueError(f"a {what} of {n} point(s) has no pairs (at least 2 are needed)")


def _pairs(n: int) -> int:
    return n * (n - 1) // 2


def _tau_a(counts, pairs: int) -> np.float64:
    """(C - D) / pairs from the exact integers (one correctly rounded division)."""
    return np.float64((int(counts[0]) - int(counts[1])) / pairs)


def _float_mean(total, pairs: int) -> np.float64:
    return np.float64(total / np.float64(pairs))


# ------------------------------------------------------------------------------ device glue
def _launch_complete(flat, off, code, kernel, algo=None):
    """tw_self_pairs or tw_self_sorted (_choose_algo) on one upload of (sample, item offsets): the
    (n_shards, 1) float64 sums or the (n_shards, 5) uint64 Kendall counters, on the host."""
    t = L.torch()
    L.device()  # no HIP device: the package's RuntimeError, before any native call
    n_shards = len(off) - 1
    sd, od = L.to_device_many([flat, off])
    max_n = int(np.diff(off).max()) if n_shards else 0
    ken = kernel == "kendall"
    out = L.empty((n_shards, 5 if ken else 1), t.int64 if ken else t.float64)
    if _choose_algo(kernel, algo, max_n) == "sorted":
        total = int(off[-1] - off[0])
        need = L.lib().tw_self_sorted_work_bytes(n_shards, total, max_n, _CODES[kernel], 0)
        work = L.empty((max(1, int(need) // 8),), t.int64)
        L.call("tw_self_sorted", sd, od, n_shards, total, max_n, code, _CODES[kernel], 0, work,
               out, L.stream_handle())
    else:
        work = L.empty((max(1, int(L.lib().tw_self_pairs_work_bytes(n_shards, max_n)) // 8),),
                       t.int64)
        L.call("tw_self_pairs", sd, od, n_shards, max_n, code, _CODES[kernel], work, out,
               L.stream_handle())
    host = out.cpu().numpy()
    return host.view(np.uint64) if ken else host


def _launch_indexed(flat, n_items, ii, jj, pair_off, code, kernel):
    """tw_self_pairs_idx32 on one upload of (sample, i, j, pair offsets); ii / jj are absolute
    item positions."""
    t = L.torch()
    L.device()
    if n_items >= 2 ** 31:
        raise ValueError("indexed pairs address at most 2^31 - 1 items")
    n_shards = len(pair_off) - 1
    sd, id_, jd, pd = L.to_device_many([flat, ii.astype(np.int32), jj.astype(np.int32),
                                        pair_off])
    max_pairs = int(np.diff(pair_off).max()) if n_shards else 0
    work = L.empty((max(1, int(L.lib().tw_self_pairs_idx_work_bytes(n_shards, max_pairs)) // 8),),
                   t.int64)
    ken = kernel == "kendall"
    out = L.empty((n_shards, 5 if ken else 1), t.int64 if ken else t.float64)
    L.call("tw_self_pairs_idx32", sd, id_, jd, pd, n_shards, max_pairs, code, _CODES[kernel],
           work, out, L.stream_handle())
    host = out.cpu().numpy()
    return host.view(np.uint64) if ken else host


def _values(raw, pairs, kernel):
    """Per-shard values on the host from the device's sums / integers."""
    if kernel == "kendall":
        return [_tau_a(row, p) for row, p in zip(raw, pairs)]
    return [_float_mean(row[0], p) for row, p in zip(raw, pairs)]


# ------------------------------------------------------------------------------- estimators
def Un(S, kernel="gini", algo=None):
    """The complete one-sample U-statistic: the mean of h over all pairs i < j."""
    assert kernel in _KERNELS
    algo = _check_algo(kernel, algo)
    flat, n, code = _items(S, kernel)
    _need_pairs(n)
    raw = _launch_complete(flat, np.array([0, n], dtype=np.int64), code, kernel, algo)
    return _values(raw, [_pairs(n)], kernel)[0]


def kendall_counts(S, algo=None):
    """(C, D, Tx, Ty, Txy) over all pairs of the (n, 2) sample, as Python ints."""
    algo = _check_algo("kendall", algo)
    flat, n, code = _items(S, "kendall")
    _need_pairs(n)
    raw = _launch_complete(flat, np.array([0, n], dtype=np.int64), code, "kendall", algo)
    return tuple(int(v) for v in raw[0])


def kendall_tau_b(S, algo=None):
    """(C - D) / (sqrt(P - Tx) * sqrt(P - Ty)); NaN when a factor is 0 (one coordinate is
    constant)."""
    c, d, tx, ty, _ = kendall_counts(S, algo)
    p = _pairs(np.asarray(S).shape[0])
    fx, fy = math.sqrt(float(p - tx)), math.sqrt(float(p - ty))
    if fx == 0.0 or fy == 0.0:
        return np.float64("nan")
    return np.float64((c - d) / (fx * fy))


def UB_indices(S, i, j, kernel):
    """The mean of h over the given index pairs (i[p], j[p])."""
    assert kernel in _KERNELS
    flat, n, code = _items(S, kernel)
    i = _check_index(np.asarray(i), n)
    j = _check_index(np.asarray(j), n)
    if i.shape != j.shape:
        raise ValueError(f"operands could not be broadcast together with shapes "
                         f"{i.shape} {j.shape}")
    i, j = i.reshape(-1), j.reshape(-1)
    if i.size == 0:
        return np.float64("nan")  # the mean of no terms
    off = np.array([0, i.size], dtype=np.int64)
    raw = _launch_indexed(flat, n, i, j, off, code, kernel)
    return _values(raw, [i.size], kernel)[0]


def _draw_pairs(n: int, B: int):
    """B distinct-index pairs, uniform over the ordered pairs i != j of n points:
    i = randint(0, n, B); j = randint(0, n - 1, B); j += (j >= i) — from the global legacy RNG,
    in this order."""
    try:  # the same two calls (values and state) in one native call
        i, j = randint_batch([(0, n, B), (0, n - 1, B)])
    except NotImplementedError:  # the global generator is not the legacy MT19937
        i = np.random.randint(0, n, B)
        j = np.random.randint(0, n - 1, B)
    j = j + (j >= i)
    return i, j


def UB(S, B, kernel="gini"):
    """The incomplete one-sample U-statistic: B pairs drawn with replacement among the pairs
    of distinct points."""
    assert kernel in _KERNELS
    _, n, _ = _items(S, kernel)
    _need_pairs(n)
    i, j = _draw_pairs(n, int(B))
    return UB_indices(S, i, j, kernel)


class _Complete:
    """Tag of a block function made by UnN: every block's Un."""

    def __init__(self, kernel, algo=None):
        self.kernel, self.algo = kernel, _check_algo(kernel, algo)

    def draw(self, k, N):
        return None

    def evaluate(self, flat, code, k, blocks, draws):
        off = np.arange(blocks + 1, dtype=np.int64) * k
        raw = _launch_complete(flat, off, code, self.kernel, self.algo)
        return _values(raw, [_pairs(k)] * blocks, self.kernel)


class _Incomplete:
    """Tag of a block function made by UnNB: every block's UB, the draws in block order (i then
    j for each block)."""

    def __init__(self, B, kernel):
        self.B, self.kernel = int(B), kernel

    def draw(self, k, N):
        try:  # the 2N calls of the N blocks, in their order, in one native call
            d = randint_batch([(0, k, self.B), (0, k - 1, self.B)] * N)
        except NotImplementedError:  # the global generator is not the legacy MT19937
            return [_draw_pairs(k, self.B) for _ in range(N)]
        return [(d[2 * b], d[2 * b + 1] + (d[2 * b + 1] >= d[2 * b])) for b in range(N)]

    def evaluate(self, flat, code, k, blocks, draws):
        if self.B == 0:
            return [np.float64("nan")] * blocks
        ii = np.concatenate([d[0] + b * k for b, d in enumerate(draws)])
        jj = np.concatenate([d[1] + b * k for b, d in enumerate(draws)])
        off = np.arange(blocks + 1, dtype=np.int64) * self.B
        raw = _launch_indexed(flat, blocks * k, ii, jj, off, code, self.kernel)
        return _values(raw, [self.B] * blocks, self.kernel)


def _block_fn(spec, fn):
    fn._tw_self_block = spec
    return fn


def _block_size(S, N) -> int:
    if not isinstance(S, np.ndarray):
        raise TypeError("UN shuffles the caller's NumPy array in place")
    k = int(S.shape[0] / N)
    _need_pairs(k, "block")
    return k


def _run(S, N, spec, T):
    """np.mean([UN(S, N, f_block) for _ in range(T)]) for a tagged f_block: the T host halves
    (in-place shuffle, the block draws) in order, then all T x N blocks in one launch on
    snapshots of the shuffled sample."""
    k = _block_size(S, N)
    _items(S, spec.kernel)  # shape / dtype errors before the RNG or the array is touched
    snaps, draws = [], []
    for t in range(T):
        np.random.shuffle(S)  # in place; rows are the items of an (n, 2) sample
        flat, _, code = _items(S, spec.kernel)
        w = flat.shape[0] // S.shape[0]
        used = flat[:N * k * w]
        snaps.append(used if t + 1 == T else used.copy())
        draws += spec.draw(k, N) or []
    if not snaps:
        return np.mean([])
    flat = snaps[0] if T == 1 else np.concatenate(snaps)
    vals = spec.evaluate(flat, code, k, T * N, draws)
    return np.mean([np.mean(vals[t * N:(t + 1) * N]) for t in range(T)])


def UN(S, N, f_block):
    """Shuffles S in place, cuts N blocks of k = int(n / N) points (the remainder is left out)
    and averages f_block over them.  Block functions made by this module (Un, and the closures
    of UnN / UnNB) are evaluated in one launch; any other callable is called block by block."""
    spec = getattr(f_block, "_tw_self_block", None)
    if spec is not None:
        return _run(S, N, spec, 1)
    k = _block_size(S, N)
    np.random.shuffle(S)
    return np.mean([f_block(S[b * k:(b + 1) * k]) for b in range(N)])


Un._tw_self_block = _Complete("gini")  # UN(S, N, Un): Un's default kernel on every block


def _complete_block(kernel, algo=None):
    def fun_block(s):
        return Un(s, kernel=kernel, algo=algo)
    return _block_fn(_Complete(kernel, algo), fun_block)


def _incomplete_block(B, kernel):
    def fun_block(s):
        return UB(s, B, kernel=kernel)
    return _block_fn(_Incomplete(B, kernel), fun_block)


def UnN(S, N, kernel="gini", algo=None):
    """Block-wise complete one-sample U-statistic."""
    assert kernel in _KERNELS
    return UN(S, N, _complete_block(kernel, algo))


def UnNB(S, N, B, kernel="gini"):
    """Block-wise incomplete one-sample U-statistic."""
    assert kernel in _KERNELS
    return UN(S, N, _incomplete_block(B, kernel))


def UnNT(S, N, T, kernel="gini", algo=None):
    """Reshuffled block-wise complete U-statistic: np.mean of T UnN calls, the T x N blocks in
    one launch."""
    assert kernel in _KERNELS
    return _run(S, N, _Complete(kernel, algo), T)


def UnNBT(S, N, B, T, kernel="gini"):
    """Reshuffled block-wise incomplete U-statistic: np.mean of T UnNB calls, the T x N blocks
    in one launch."""
    assert kernel in _KERNELS
    return _run(S, N, _Incomplete(B, kernel), T)
