"""Two-sample triplet U-statistics of degree (2,1) on MI355X (an extension; the reference has
none): an anchor x_i, a point x_j of its own class (j != i) and a point z_k of the other class,

    h(x_i, x_j, z_k) = 1{D(x_i, z_k) > D(x_i, x_j)}

the triplet statistic of metric learning and ranking.  X is (n, d) and Z is (m, d), float64 and
C-contiguous (a 1-D array is d = 1), 1 <= d <= 64, n >= 2, m >= 1; anything else is a ValueError
before any device work or RNG draw.

D(a, b) is the squared Euclidean distance in ONE arithmetic order, so that counts are exact and
reproducible: acc = 0.0; for c in 0..d-1: t = a_c - b_c; acc = acc + t * t — ascending
coordinates, multiply and add separate (no FMA).  Per anchor i of a block,

    gt_i = #{(j, k): j != i, D(x_i, z_k) > D(x_i, x_j)},    eq_i likewise with ==

by IEEE comparisons of doubles (a NaN distance counts for neither; duplicated points tie at 0).
mode="gt" counts gt, mode="half" counts 2 gt + eq in half-units; the block value is the exact
integer total over n (n - 1) m (twice that for "half"), one correctly rounded division.

For a fixed anchor the count over (j, k) is a two-sample count between two rows of distances, so
the complete statistic is csrc/triplets.hip's tw_triplet_rows (it writes the rows) followed by
the package's exact pair count with one anchor per shard.  Drawn triplets go
through tw_triplet_idx32.  The estimators mirror compute_stats.py:95-123 for the proportional
partition without replacement: the host owns the shuffles and the draws (NumPy's global legacy
RNG, in NumPy's order), the device the arithmetic.
"""
from __future__ import annotations

import numpy as np

from . import _engine as E
from . import _lib as L
from .compute_stats import _check_index
from .numpy_rng import randint_batch

_PREDS = {"gt": L.TW_PRED_GT, "half": L.TW_PRED_HALF}
MAX_D = 64
# the two row workspaces of one batch of anchors stay under this many bytes (a batch holds at
# least one anchor, whatever its rows take)
ROWS_BYTES = 1 << 30


# ------------------------------------------------------------------------------ host checks
def _rows(A, name):
    """The sample as the device reads it, (rows, d) float64 C-contiguous — a view, never a copy
    of an ndarray."""
    A = np.asarray(A)
    if A.dtype != np.float64:
        raise ValueError(f"{name} must be float64, not {A.dtype}")
    if A.ndim not in (1, 2):
        raise ValueError(f"{name} must be (rows, d) or 1-D, not shape {A.shape}")
    if not A.flags.c_contiguous:
        raise ValueError(f"{name} must be C-contiguous")
    return A.reshape(-1, 1) if A.ndim == 1 else A


def _check(X, Z, mode):
    """(Xf, Zf) or a ValueError, before anything touches a device or the RNG."""
    if mode not in _PREDS:
        raise ValueError(f"mode={mode!r} is not one of {list(_PREDS)}")
    Xf, Zf = _rows(X, "X"), _rows(Z, "Z")
    d = Xf.shape[1]
    if Zf.shape[1] != d:
        raise ValueError(f"X has {d} coordinates and Z has {Zf.shape[1]}")
    if not 1 <= d <= MAX_D:
        raise ValueError(f"d = {d} is outside [1, {MAX_D}]")
    if Xf.shape[0] < 2:
        raise ValueError(f"X has {Xf.shape[0]} row(s): a triplet needs two points of the "
                         f"anchor's class")
    if Zf.shape[0] < 1:
        raise ValueError("Z has no rows: a triplet needs a point of the other class")
    if max(Xf.shape[0], Zf.shape[0]) >= 2 ** 31:
        raise ValueError("at most 2^31 - 1 rows per sample")
    return Xf, Zf


def _check_algo(algo, mode):
    """algo= as given (None: "auto"); pick_algo's own ValueError for anything unknown."""
    algo = "auto" if algo is None else algo
    E.pick_algo(algo, 1, 1, mode)
    return algo


def _triplets(n: int, m: int) -> int:
    return n * (n - 1) * m


def _value(count: int, triplets: int, mode: str) -> np.float64:
    """count / triplets (half-units: / 2 triplets) from exact integers, rounded once."""
    if triplets == 0:
        return np.float64("nan")  # the mean of no terms
    return np.float64(int(count) / int(triplets * (2 if mode == "half" else 1)))


def _total(counts, bound: int) -> int:
    """The exact sum of uint64 counts whose sum is at most `bound`."""
    if bound < 2 ** 64:
        return int(counts.sum(dtype=np.uint64))
    return int(counts.astype(object).sum())


def batch_edges(row_elems, cap_bytes: int):
    """Consecutive anchor ranges [(a0, a1), ...] covering every anchor once: each range's rows
    (row_elems[a] doubles for anchor a) take at most cap_bytes, except that a range always holds
    at least one anchor."""
    row_elems = np.asarray(row_elems, dtype=np.int64)
    csum = np.concatenate([[0], np.cumsum(row_elems)]) * 8
    edges, a0, n = [], 0, len(row_elems)
    while a0 < n:
        a1 = int(np.searchsorted(csum, csum[a0] + int(cap_bytes), side="right")) - 1
        a1 = min(max(a1, a0 + 1), n)
        edges.append((a0, a1))
        a0 = a1
    return edges


# ------------------------------------------------------------------------------ device glue
class _Batches:
    """The resident state of one complete count: the blocks b = rows [bxo[b], bxo[b + 1]) of Xf
    against rows [bzo[b], bzo[b + 1]) of Zf, their anchors cut into batches whose two row
    workspaces stay under ROWS_BYTES.  The inputs and every batch's row offsets (each batch's
    start at 0 in the shared workspaces) go up in one copy."""

    def __init__(self, Xf, Zf, bxo, bzo, mode, algo):
        t = L.torch()
        L.device()  # no HIP device: the package's RuntimeError, before any native call
        self.bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
        nb, mb = np.diff(self.bxo), np.diff(bzo)
        self.d, self.pred = Xf.shape[1], _PREDS[mode]
        self.max_n, self.max_m = int(nb.max()), int(mb.max())
        self.algo = E.pick_algo(algo, self.max_m, self.max_n - 1, mode)
        other_len, own_len = np.repeat(mb, nb), np.repeat(nb - 1, nb)
        self.edges = batch_edges(other_len + own_len, ROWS_BYTES)
        oo = [np.concatenate([[0], np.cumsum(other_len[a0:a1])]) for a0, a1 in self.edges]
        wo = [np.concatenate([[0], np.cumsum(own_len[a0:a1])]) for a0, a1 in self.edges]
        self.x, self.z, self.bx, self.bz, self.oo, self.wo = L.to_device_many(
            [Xf.reshape(-1), Zf.reshape(-1), self.bxo, bzo, np.concatenate(oo).astype(np.int64),
             np.concatenate(wo).astype(np.int64)])
        self.pos = np.concatenate([[0], np.cumsum([a1 - a0 + 1 for a0, a1 in self.edges])])
        self.row_elems = [int(o[-1]) + int(w[-1]) for o, w in zip(oo, wo)]  # written per batch
        self.other = L.empty((max(1, max(int(o[-1]) for o in oo)),), t.float64)
        self.own = L.empty((max(1, max(int(w[-1]) for w in wo)),), t.float64)

    def _offsets(self, q):
        p0, p1 = int(self.pos[q]), int(self.pos[q + 1])
        return self.oo[p0:p1], self.wo[p0:p1]

    def rows(self, q):
        """Batch q's tw_triplet_rows launch."""
        a0, a1 = (int(self.bxo[0]) + a for a in self.edges[q])
        oq, wq = self._offsets(q)
        first = int(np.searchsorted(self.bxo, a0, side="right")) - 1
        last = int(np.searchsorted(self.bxo, a1 - 1, side="right")) - 1
        L.call("tw_triplet_rows", self.x, self.z, self.d, self.bx, self.bz, first,
               last - first + 1, a0, a1, self.max_n, self.max_m, oq, wq, self.other, self.own,
               L.stream_handle())

    def count(self, q):
        """Batch q's exact pair count, one anchor per shard: the "other" row on the x side, the
        "own" row on the z side.  Returns the int64 device tensor."""
        oq, wq = self._offsets(q)
        a0, a1 = self.edges[q]
        return E.count_launch(self.other, oq, self.own, wq, a1 - a0, self.max_m, self.max_n - 1,
                              L.TW_F64, self.pred, self.algo)

    def run(self):
        """Every batch's rows and count in order; the per-anchor counts come back in one copy."""
        outs = []
        for q in range(len(self.edges)):
            self.rows(q)
            outs.append(self.count(q))
        out = outs[0] if len(outs) == 1 else L.torch().cat(outs)
        return out.cpu().numpy().view(np.uint64)


def _count_blocks(Xf, Zf, bxo, bzo, mode, algo):
    """The per-anchor counts (uint64, on the host) of every anchor of the given blocks."""
    return _Batches(Xf, Zf, bxo, bzo, mode, algo).run()


def _count_indexed(Xf, Zf, ii, jj, kk, trip_off, mode):
    """tw_triplet_idx32 on one upload: the per-shard uint64 counts of the given triplets
    (absolute rows)."""
    t = L.torch()
    L.device()
    n_shards = len(trip_off) - 1
    xd, zd, id_, jd, kd, od = L.to_device_many(
        [Xf.reshape(-1), Zf.reshape(-1), ii.astype(np.int32), jj.astype(np.int32),
         kk.astype(np.int32), np.asarray(trip_off, dtype=np.int64)])
    max_t = int(np.diff(trip_off).max()) if n_shards else 0
    work = L.empty((max(1, int(L.lib().tw_triplet_idx_work_bytes(n_shards, max_t)) // 8),),
                   t.int64)
    out = L.empty((n_shards,), t.int64)
    L.call("tw_triplet_idx32", xd, zd, Xf.shape[1], id_, jd, kd, od, n_shards, max_t,
           _PREDS[mode], work, out, L.stream_handle())
    return out.cpu().numpy().view(np.uint64)


# ------------------------------------------------------------------------------- estimators
def triplet_counts(X, Z, mode="gt", algo=None):
    """The uint64 array of per-anchor counts: gt_i, or 2 gt_i + eq_i for mode="half".
    algo: "pairs", "sorted" or None / "auto" (the pair count's own choice)."""
    Xf, Zf = _check(X, Z, mode)
    algo = _check_algo(algo, mode)
    return _count_blocks(Xf, Zf, [0, Xf.shape[0]], [0, Zf.shape[0]], mode, algo)


def Un(X, Z, mode="gt", algo=None):
    """The complete triplet U-statistic: the mean of h over all n (n - 1) m triplets."""
    Xf, Zf = _check(X, Z, mode)
    n, m = Xf.shape[0], Zf.shape[0]
    counts = triplet_counts(Xf, Zf, mode, algo)
    return _value(_total(counts, 2 * _triplets(n, m)), _triplets(n, m), mode)


def UB_indices(X, Z, i, j, k, mode="gt"):
    """The mean of h over the given triplets (x_i[p], x_j[p], z_k[p])."""
    Xf, Zf = _check(X, Z, mode)
    i = _check_index(np.asarray(i), Xf.shape[0])
    j = _check_index(np.asarray(j), Xf.shape[0])
    k = _check_index(np.asarray(k), Zf.shape[0])
    if not i.shape == j.shape == k.shape:
        raise ValueError(f"operands could not be broadcast together with shapes "
                         f"{i.shape} {j.shape} {k.shape}")
    i, j, k = i.reshape(-1), j.reshape(-1), k.reshape(-1)
    if i.size == 0:
        return np.float64("nan")  # the mean of no terms
    count = _count_indexed(Xf, Zf, i, j, k, [0, i.size], mode)[0]
    return _value(int(count), i.size, mode)


def _draw_triplets(n: int, m: int, B: int):
    """B triplets, uniform over i != j and k: i = randint(0, n, B); j = randint(0, n - 1, B);
    j += (j >= i); k = randint(0, m, B) — from the global legacy RNG, in this order."""
    try:  # the same three calls (values and state) in one native call
        i, j, k = randint_batch([(0, n, B), (0, n - 1, B), (0, m, B)])
    except NotImplementedError:  # the global generator is not the legacy MT19937
        i = np.random.randint(0, n, B)
        j = np.random.randint(0, n - 1, B)
        k = np.random.randint(0, m, B)
    return i, j + (j >= i), k


def UB(X, Z, B, mode="gt"):
    """The incomplete triplet U-statistic: B triplets drawn with replacement."""
    Xf, Zf = _check(X, Z, mode)
    i, j, k = _draw_triplets(Xf.shape[0], Zf.shape[0], int(B))
    return UB_indices(Xf, Zf, i, j, k, mode)


class _Complete:
    """Tag of a block function made by UnN: every block's Un, all blocks through the same
    batches."""

    def __init__(self, mode, algo=None):
        self.mode, self.algo = mode, _check_algo(algo, mode)

    def evaluate(self, Xf, Zf, k, kz, N):
        counts = _count_blocks(Xf[:N * k], Zf[:N * kz], np.arange(N + 1) * k,
                               np.arange(N + 1) * kz, self.mode, self.algo)
        trip = _triplets(k, kz)
        return [_value(_total(c, 2 * trip), trip, self.mode) for c in counts.reshape(N, k)]


class _Incomplete:
    """Tag of a block function made by UnNB: every block's UB, the draws in block order (i, j,
    k for each block), all blocks in one tw_triplet_idx32 launch."""

    def __init__(self, B, mode):
        self.B, self.mode = int(B), mode

    def evaluate(self, Xf, Zf, k, kz, N):
        B = self.B
        try:  # the 3N calls of the N blocks, in their order, in one native call
            d = randint_batch([(0, k, B), (0, k - 1, B), (0, kz, B)] * N)
            draws = [(d[3 * b], d[3 * b + 1] + (d[3 * b + 1] >= d[3 * b]), d[3 * b + 2])
                     for b in range(N)]
        except NotImplementedError:  # the global generator is not the legacy MT19937
            draws = [_draw_triplets(k, kz, B) for _ in range(N)]
        if B == 0:
            return [np.float64("nan")] * N
        ii = np.concatenate([t[0] + b * k for b, t in enumerate(draws)])
        jj = np.concatenate([t[1] + b * k for b, t in enumerate(draws)])
        kk = np.concatenate([t[2] + b * kz for b, t in enumerate(draws)])
        counts = _count_indexed(Xf[:N * k], Zf[:N * kz], ii, jj, kk, np.arange(N + 1) * B,
                                self.mode)
        return [_value(int(c), B, self.mode) for c in counts]


def _block_fn(spec, fn):
    fn._tw_triplet_block = spec
    return fn


def UN(X, Z, N, f_block, sampling_type="prop-SWOR"):
    """Shuffles X, then Z, in place (rows), cuts N blocks of k = int(n / N) rows of X and
    kz = int(m / N) rows of Z (the remainders are left out) and averages f_block(x, z) over
    them.  Block functions made by this module (Un, and the closures of UnN / UnNB) are
    evaluated together on the device; any other callable is called block by block."""
    if sampling_type != "prop-SWOR":
        raise ValueError(f"sampling_type={sampling_type!r}: only the proportional partition "
                         f"without replacement ('prop-SWOR') is offered for triplets; 'SWOR' and "
                         f"'prop-SWR' are out of scope (DESIGN.md §4.10)")
    if not isinstance(X, np.ndarray) or not isinstance(Z, np.ndarray):
        raise ValueError("UN shuffles the caller's NumPy arrays in place")
    spec = getattr(f_block, "_tw_triplet_block", None)
    Xf, Zf = _check(X, Z, "gt")
    k, kz = int(Xf.shape[0] / N), int(Zf.shape[0] / N)
    if k < 2 or kz < 1:
        raise ValueError(f"N = {N} blocks of {k} row(s) of X and {kz} of Z: a block needs at "
                         f"least 2 rows of X and 1 of Z")
    np.random.shuffle(X)
    np.random.shuffle(Z)
    if spec is not None:
        return np.mean(spec.evaluate(Xf, Zf, k, kz, N))  # Xf / Zf view the shuffled arrays
    return np.mean([f_block(X[b * k:(b + 1) * k], Z[b * kz:(b + 1) * kz]) for b in range(N)])


Un._tw_triplet_block = _Complete("gt")  # UN(X, Z, N, Un): Un's defaults on every block


def UnN(X, Z, N, sampling_type="prop-SWOR", mode="gt", algo=None):
    """Block-wise complete triplet U-statistic."""

    def fun_block(x, z):
        return Un(x, z, mode=mode, algo=algo)

    _check(X, Z, mode)
    return UN(X, Z, N, _block_fn(_Complete(mode, algo), fun_block), sampling_type)


def UnNB(X, Z, N, B, sampling_type="prop-SWOR", mode="gt"):
    """Block-wise incomplete triplet U-statistic."""

    def fun_block(x, z):
        return UB(x, z, B, mode=mode)

    _check(X, Z, mode)
    return UN(X, Z, N, _block_fn(_Incomplete(B, mode), fun_block), sampling_type)


def UnNT(X, Z, N, T, sampling_type="prop-SWOR", mode="gt", algo=None):
    """Reshuffled block-wise complete triplet U-statistic."""
    return np.mean([UnN(X, Z, N, sampling_type, mode, algo) for _ in range(T)])


def UnNBT(X, Z, N, B, T, sampling_type="prop-SWOR", mode="gt"):
    """Reshuffled block-wise incomplete triplet U-statistic."""
    return np.mean([UnNB(X, Z, N, B, sampling_type, mode) for _ in range(T)])
