"""Exact quantiles of pairwise distances on MI355X, and the median-heuristic bandwidth of the
Gaussian kernel (an extension; the reference has none): sigma = median ||w_i - w_j|| over the pairs
of a sample, which tuplewise.mmd, tuplewise.hsic and tuplewise.hsic_perm accept as sigma="median".

The pair sets of X (n, d) and Z (m, d), float64 and C-contiguous (a 1-D array is d = 1), 1 <= d <=
64, fewer than 2^31 rows, every entry finite, at least one pair (anything else is a ValueError
before any device work):

    pairs="within"  the M = n (n - 1) / 2 pairs i < j of X; Z must be None
    pairs="cross"   the M = n m pairs (x_i, z_k)
    pairs="pooled"  "within" on the pooled sample [X; Z], formed here

D is the squared Euclidean distance of tuplewise.triplets in its arithmetic order (acc = 0.0; for c
in 0..d-1: t = a_c - b_c; acc = acc + t * t, never fused), by the same device functions as
everywhere else.  Order statistics are EXACT: for finite rows D is a non-negative double (+inf by
overflow at most, never NaN or -0), so its 64-bit pattern orders like an unsigned integer and the
k-th smallest D is found by a radix select over integer histograms (csrc/distselect.hip, DESIGN.md
§4.16) — bit for bit np.sort of the same distances, with no tolerance.  Nothing of size O(M) is
stored: a pass over the pairs leaves one histogram of the next digit_bits bits of the keys that
share a target's prefix; the host narrows every target rank to its digit and, once the candidates
of all targets fit the gather capacity, has them appended to one key buffer and finishes on it.
Square roots and the mean of the two middle distances are NumPy's, on the host.

No function here draws from or touches NumPy's global RNG.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from .triplets import _rows

MAX_D = 64
KEY_BITS = 63             # bit 63 of a key is 0
DIGIT_BITS = 11           # tw_dist_select_digit_bits()
MAX_GROUPS = 8            # tw_dist_select_max_groups(): prefix groups (targets) per pass
GATHER_CAP = 1 << 20      # keys (8 MiB): candidates at or below it are gathered
_PAIRS = ("within", "cross", "pooled")


# ------------------------------------------------------------------ host select logic (no device)
def _digit_at(bits_done: int, digit_bits: int = DIGIT_BITS):
    """(shift, width) of the digit that follows bits_done resolved bits of the 63-bit key."""
    width = min(digit_bits, KEY_BITS - bits_done)
    return KEY_BITS - bits_done - width, width


def _group(prefixes):
    """(groups, inverse): the distinct prefixes, ascending, and every target's group — targets
    that share a prefix share a group."""
    return np.unique(np.asarray(prefixes, dtype=np.uint64), return_inverse=True)


def _narrow(hist, inverse, prefixes, ranks, width: int):
    """One pass's narrowing.  hist[g] is the digit histogram of the keys under group g, target t
    has rank ranks[t] among the keys under prefixes[t] (group inverse[t]).  Returns the prefixes
    extended by each target's digit, the ranks inside the new prefixes and the new candidate
    counts."""
    hist = np.asarray(hist, dtype=np.uint64)
    new_p = np.empty(len(ranks), dtype=np.uint64)
    new_r = np.empty(len(ranks), dtype=np.int64)
    counts = np.empty(len(ranks), dtype=np.int64)
    for t in range(len(ranks)):
        cum = np.cumsum(hist[inverse[t]][:1 << width].astype(np.int64))
        r = int(ranks[t])
        if not 0 <= r < int(cum[-1]):
            raise RuntimeError(f"rank {r} outside its group's {int(cum[-1])} keys: the histogram "
                               f"does not match the pairs")
        digit = int(np.searchsorted(cum, r, side="right"))
        new_p[t] = (int(prefixes[t]) << width) | digit
        new_r[t] = r - (int(cum[digit - 1]) if digit else 0)
        counts[t] = int(hist[inverse[t]][digit])
    return new_p, new_r, counts


def _candidates(prefixes, counts) -> int:
    """The keys under the distinct prefixes: what a gather of these groups would append."""
    _, first = np.unique(np.asarray(prefixes, dtype=np.uint64), return_index=True)
    return int(np.asarray(counts, dtype=np.int64)[first].sum())


def _gather_now(candidates: int, cap: int) -> bool:
    """cap = 0 never gathers; a cap at or above the pair count gathers at once."""
    return 0 < candidates <= cap


def _select_chunk(ranks, M: int, source, cap: int, digit_bits: int):
    """The keys of at most MAX_GROUPS ranks.  source.hist(groups, bits, shift, width, buffer)
    gives the (len(groups), >= 2^width) digit histogram of the keys under the groups (prefixes of
    `bits` bits), over the pairs (buffer None) or over a gathered buffer; source.gather(groups,
    bits, count) returns such a buffer."""
    prefixes = np.zeros(len(ranks), dtype=np.uint64)
    r = np.asarray(ranks, dtype=np.int64).copy()
    bits, buffer = 0, None
    if _gather_now(M, cap):
        buffer = source.gather(np.zeros(1, dtype=np.uint64), 0, M)
    while bits < KEY_BITS:
        shift, width = _digit_at(bits, digit_bits)
        groups, inverse = _group(prefixes)
        hist = source.hist(groups, bits, shift, width, buffer)
        prefixes, r, counts = _narrow(hist, inverse, prefixes, r, width)
        bits += width
        if buffer is None and bits < KEY_BITS:
            total = _candidates(prefixes, counts)
            if _gather_now(total, cap):
                buffer = source.gather(_group(prefixes)[0], bits, total)
    return prefixes


def _select(ranks, M: int, source, cap: int = GATHER_CAP, digit_bits: int = DIGIT_BITS):
    """The uint64 keys of the given 0-based ranks among M keys, MAX_GROUPS distinct ranks at a
    time."""
    ranks = np.asarray(ranks, dtype=np.int64).reshape(-1)
    uniq, inverse = np.unique(ranks, return_inverse=True)
    keys = np.empty(len(uniq), dtype=np.uint64)
    for s in range(0, len(uniq), MAX_GROUPS):
        keys[s:s + MAX_GROUPS] = _select_chunk(uniq[s:s + MAX_GROUPS], M, source, cap, digit_bits)
    return keys[inverse.reshape(-1)]


# ------------------------------------------------------------------------------ host checks
def _pair_count(n: int, m: int, pairs: str) -> int:
    if pairs == "within":
        return n * (n - 1) // 2
    if pairs == "cross":
        return n * m
    return (n + m) * (n + m - 1) // 2


def _check_finite(A, name):
    if not np.isfinite(A).all():
        raise ValueError(f"{name} has a non-finite entry: distance quantiles need finite rows")


def _check(X, Z, pairs):
    """(A, B, pair set id, M) or a ValueError, before anything touches a device: A (and B for
    "cross") as the device reads them; "pooled" is "within" on the concatenation."""
    if pairs not in _PAIRS:
        raise ValueError(f"pairs={pairs!r} is not one of {list(_PAIRS)}")
    Xf = _rows(X, "X")
    if pairs == "within":
        if Z is not None:
            raise ValueError("pairs='within' takes one sample: Z must be None")
        Zf = None
    else:
        if Z is None:
            raise ValueError(f"pairs={pairs!r} needs Z")
        Zf = _rows(Z, "Z")
        if Zf.shape[1] != Xf.shape[1]:
            raise ValueError(f"X has {Xf.shape[1]} coordinates and Z has {Zf.shape[1]}")
    d = Xf.shape[1]
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d = {d} is outside [1, {MAX_D}]")
    n, m = Xf.shape[0], 0 if Zf is None else Zf.shape[0]
    if (n + m if pairs == "pooled" else max(n, m)) >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows")
    M = _pair_count(n, m, pairs)
    if M < 1:
        raise ValueError(f"pairs={pairs!r} of {n} and {m} row(s): there is no pair")
    _check_finite(Xf, "X")
    if Zf is not None:
        _check_finite(Zf, "Z")
    if pairs == "pooled":
        return np.concatenate([Xf, Zf]), None, L.TW_DIST_WITHIN, M
    return Xf, Zf, (L.TW_DIST_WITHIN if pairs == "within" else L.TW_DIST_CROSS), M


def _check_ranks(ranks, M: int):
    if ranks is None:
        raise ValueError("ranks is required")
    r = np.asarray(ranks)
    if r.size == 0:
        return np.empty(r.shape, dtype=np.int64)
    if r.dtype == np.bool_ or r.dtype.kind not in "iu":
        raise ValueError(f"ranks must be integers, not {r.dtype}")
    if r.size and (int(r.min()) < 0 or int(r.max()) >= M):
        raise ValueError(f"ranks must lie in [0, {M})")
    return r.astype(np.int64)


def _check_cap(cap):
    if cap is None:
        return GATHER_CAP
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0:
        raise ValueError(f"_gather_cap = {cap!r} must be an int >= 0")
    return int(cap)


# ------------------------------------------------------------------------------ device glue
def _host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


class _DeviceSource:
    """The select's passes on the device: one upload of the rows, then per pass one launch and one
    read of the histogram.  launches / reads count the native calls and the host reads."""

    def __init__(self, A, B, pid):
        t = L.torch()
        L.device()  # no HIP device: the package's RuntimeError, before any native call
        lib = L.lib()
        if (int(lib.tw_dist_select_digit_bits()) != DIGIT_BITS
                or int(lib.tw_dist_select_max_groups()) != MAX_GROUPS):
            raise L.TuplewiseError("tuplewise.bandwidth: the library's digit width or group count "
                                   "differs from this module's")
        self.pid, self.d, self.n = pid, A.shape[1], A.shape[0]
        if B is None:
            self.xd, self.zd, self.m = L.to_device(A.reshape(-1)), None, 0
        else:
            self.xd, self.zd = L.to_device_many([A.reshape(-1), B.reshape(-1)])
            self.m = B.shape[0]
        self.bins = 1 << DIGIT_BITS
        self.hist_d = L.empty((MAX_GROUPS * self.bins,), t.int64)
        self.count_d = L.empty((2,), t.int64)
        self.launches = self.reads = 0

    @staticmethod
    def _groups(groups, bits):
        pre = np.ascontiguousarray(groups, dtype=np.uint64)
        return pre, np.full(len(pre), bits, dtype=np.int32)

    def hist(self, groups, bits, shift, width, buffer):
        pre, pb = self._groups(groups, bits)
        if buffer is None:
            L.call("tw_dist_hist", self.xd, self.n, self.zd, self.m, self.d, self.pid,
                   _host_ptr(pre), _host_ptr(pb), len(pre), shift, width, self.hist_d,
                   L.stream_handle())
        else:
            L.call("tw_keys_hist", buffer, buffer.numel(), _host_ptr(pre), _host_ptr(pb),
                   len(pre), shift, width, self.hist_d, L.stream_handle())
        self.launches += 1
        self.reads += 1
        h = self.hist_d[:len(pre) * self.bins].cpu().numpy().view(np.uint64)
        return h.reshape(len(pre), self.bins)

    def gather(self, groups, bits, count):
        pre, pb = self._groups(groups, bits)
        keys = L.empty((count,), L.torch().int64)
        L.call("tw_dist_gather", self.xd, self.n, self.zd, self.m, self.d, self.pid,
               _host_ptr(pre), _host_ptr(pb), len(pre), keys, count, self.count_d,
               L.stream_handle())
        self.launches += 1
        self.reads += 1
        got = self.count_d.cpu().numpy()
        if int(got[0]) != count or int(got[1]) != 0:
            raise L.TuplewiseError(f"tuplewise.bandwidth: the gather appended {int(got[0])} keys "
                                   f"where the histograms counted {count}")
        return keys


def _order_keys(A, B, pid, M, ranks, cap):
    """The uint64 keys (bit patterns of D) of the ranks, on the device."""
    if ranks.size == 0:
        return np.empty(0, dtype=np.uint64)
    return _select(ranks, M, _DeviceSource(A, B, pid), cap)


# ------------------------------------------------------------------------------- public surface
def order_statistics(X, Z=None, ranks=None, pairs="within", *, _gather_cap=None):
    """The ranks-th smallest squared distances of the pair set, a float64 array of ranks' shape:
    ranks are 0-based integers in [0, M), any count, duplicates allowed.  Exact (np.sort of the
    same distances, bit for bit).  _gather_cap (private, for the tests): 0 never gathers, a value
    >= M gathers at once, None is the default capacity."""
    A, B, pid, M = _check(X, Z, pairs)
    r = _check_ranks(ranks, M)
    cap = _check_cap(_gather_cap)
    keys = _order_keys(A, B, pid, M, r.reshape(-1), cap)
    return keys.view(np.float64).reshape(r.shape)


def _median_of(A, B, pid, M, cap=GATHER_CAP):
    D = _order_keys(A, B, pid, M, np.array([(M - 1) // 2, M // 2], dtype=np.int64),
                    cap).view(np.float64)
    return (np.sqrt(D[0]) + np.sqrt(D[1])) / 2.0


def median_distance(X, Z=None, pairs="within", *, _gather_cap=None):
    """The median Euclidean distance over the pair set, (sqrt(D_(lo)) + sqrt(D_(hi))) / 2.0 with
    lo = (M - 1) // 2 and hi = M // 2: np.median(np.sqrt(D)) bit for bit."""
    A, B, pid, M = _check(X, Z, pairs)
    return np.float64(_median_of(A, B, pid, M, _check_cap(_gather_cap)))


def quantile_distances(X, Z=None, q=None, pairs="within", method="lower", *, _gather_cap=None):
    """sqrt of the order statistic at floor (method="lower") or ceil ("higher") of q (M - 1), q in
    [0, 1], a float64 array of q's shape: np.quantile(np.sqrt(D), q, method=method).  A ladder of
    bandwidths in one call."""
    if method not in ("lower", "higher"):
        raise ValueError(f"method={method!r} is not 'lower' or 'higher'")
    A, B, pid, M = _check(X, Z, pairs)
    if q is None:
        raise ValueError("q is required")
    try:
        qa = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"q={q!r} is not numeric") from None
    if qa.size and not (np.all(qa >= 0.0) and np.all(qa <= 1.0)):  # (a NaN fails both)
        raise ValueError("q must lie in [0, 1]")
    pos = qa * (M - 1)
    idx = (np.floor(pos) if method == "lower" else np.ceil(pos)).astype(np.int64)
    idx = np.clip(idx, 0, M - 1)
    cap = _check_cap(_gather_cap)
    D = _order_keys(A, B, pid, M, idx.reshape(-1), cap).view(np.float64)
    return np.sqrt(D).reshape(qa.shape)


def _median_sigma(A, B, pairs, what):
    """sigma="median" of the kernel modules: the median distance of already checked rows, a Python
    float, or a ValueError for non-finite rows and for a median of 0."""
    A, B, pid, M = _check(A, B, pairs)
    s = float(_median_of(A, B, pid, M))
    if s == 0.0:
        raise ValueError(f"sigma='median': the median distance of {what} is 0 (at least half of "
                         f"the pairs coincide); give a numeric sigma")
    return s
