"""Triplet metric learning on MI355X (an extension; the reference has none): a linear map L of
shape (p, d) learnt under the triplet hinge by SGD on reshuffled shards, with the trade-off
knobs of the reference's learning_process (make_exps.py:96-141: the number of blocks N, the
triplets B drawn per block, the reshuffle period), and judged by the triplet statistic of
tuplewise.triplets on the projected samples.

X is (n, d) and Z is (m, d), float64 and C-contiguous, 1 <= d <= 64; Lmap is (p, d), float64 and
C-contiguous, 1 <= p <= 64 (p <= d is not required).  A triplet is (i, j, k): rows i != j of X
and a row k of Z.  With a = x_i - x_j, b = x_i - z_k, u = L a and v = L b,

    S = margin + |u|^2 - |v|^2,    loss = max(S, 0),    G_t = 1{S > 0} 2 (u a^T - v b^T)

A shard's loss and gradient are the means over its triplets, a step's gradient the mean over
shards plus reg L; "SGD": delta = lr g, "momentum": delta = 0.9 delta + lr g; then L = L - delta.

Arithmetic: the gradient and the loss carry no bit contract (they are
deterministic from run to run: no atomics, partials added in a fixed order); project() is
bit-exact — acc = 0.0; for c in 0..d-1: acc = acc + L[r, c] * A[row, c], multiply and add
separate, a NaN written as np.nan — so every statistic evaluated on projected samples is an
exact count; the update is bit-exact given the gradient.

The host owns the permutations and the draws (NumPy's global legacy RNG, in the order written in
learning_process), the device the arithmetic: csrc/triplet_grad.hip.  Every argument error is a
ValueError before any device work or RNG draw.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib as L
from . import triplets as T
from .numpy_rng import Session

MAX_DIM = 64
OPTIMS = ("SGD", "momentum")
# triplets drawn and uploaded at once (a reshuffle period is cut into such chunks of whole steps)
CHUNK_TRIPLETS = 1 << 22


# ------------------------------------------------------------------------------ host checks
def _check_map(Lmap, d):
    """Lmap as the device reads it, (p, d) float64 C-contiguous, or a ValueError."""
    if not isinstance(Lmap, np.ndarray):
        raise ValueError("Lmap must be a NumPy array of shape (p, d)")
    if Lmap.dtype != np.float64:
        raise ValueError(f"Lmap must be float64, not {Lmap.dtype}")
    if Lmap.ndim != 2:
        raise ValueError(f"Lmap must be (p, d), not shape {Lmap.shape}")
    if not Lmap.flags.c_contiguous:
        raise ValueError("Lmap must be C-contiguous")
    p = Lmap.shape[0]
    if not 1 <= p <= MAX_DIM:
        raise ValueError(f"p = {p} is outside [1, {MAX_DIM}]")
    if Lmap.shape[1] != d:
        raise ValueError(f"Lmap has {Lmap.shape[1]} columns and the samples {d} coordinates")
    return Lmap


def _check_rows(A, name):
    """A sample to project: (rows, d) float64 C-contiguous, 1 <= d <= 64 (any number of rows)."""
    Af = T._rows(A, name)
    if not 1 <= Af.shape[1] <= MAX_DIM:
        raise ValueError(f"d = {Af.shape[1]} is outside [1, {MAX_DIM}]")
    return Af


def _check_rows_index(ind, n, name):
    """A 1-D integer array of rows in [0, n), as int64."""
    ind = np.asarray(ind)
    if ind.dtype.kind not in "iu" or ind.ndim != 1:
        raise ValueError(f"{name} must be a 1-D integer array")
    if ind.size and (int(ind.min()) < 0 or int(ind.max()) >= n):
        raise ValueError(f"{name} has a row outside [0, {n})")
    return ind.astype(np.int64, copy=False)


def _check_triplets(i, j, k, n, m):
    i, j, k = (_check_rows_index(i, n, "i"), _check_rows_index(j, n, "j"),
               _check_rows_index(k, m, "k"))
    if not i.shape == j.shape == k.shape:
        raise ValueError(f"i, j and k have {i.size}, {j.size} and {k.size} entries")
    if np.any(i == j):
        raise ValueError("a triplet with i == j")
    return i, j, k


def _check_trip_off(trip_off, T_):
    if trip_off is None:
        return np.array([0, T_], dtype=np.int64)
    off = np.asarray(trip_off)
    if off.dtype.kind not in "iu" or off.ndim != 1 or off.size < 1:
        raise ValueError("trip_off must be a 1-D integer array of n_shards + 1 offsets")
    off = off.astype(np.int64, copy=False)
    if off[0] != 0 or off[-1] != T_ or np.any(np.diff(off) < 0):
        raise ValueError(f"trip_off must rise from 0 to the {T_} triplets given")
    return off


# ------------------------------------------------------------------------------ device glue
class _Grad:
    """tw_triplet_grad's outputs and work buffer for launches of n_shards shards of at most
    max_t triplets."""

    def __init__(self, n_shards, max_t, d, p):
        t = L.torch()
        self.n_shards, self.max_t, self.d, self.p = int(n_shards), int(max_t), int(d), int(p)
        nbytes = int(L.lib().tw_triplet_grad_work_bytes(self.n_shards, self.max_t, d, p))
        self.work = L.empty((max(1, nbytes // 8),), t.int64)
        self.G = L.empty((p * d,), t.float64)
        self.loss = L.empty((max(1, self.n_shards),), t.float64)
        self.active = L.empty((max(1, self.n_shards),), t.int64)

    def launch(self, xd, zd, Ld, i, j, k, off, margin, want_grad, stream):
        L.call("tw_triplet_grad", xd, zd, self.d, Ld, self.p, i, j, k, off, self.n_shards,
               self.max_t, float(margin), int(want_grad), self.work, self.G, self.loss,
               self.active, stream)


def _loss_of(shard_loss, sizes):
    """The mean of the non-empty shards' mean losses (no shard: nan, the mean of no terms)."""
    keep = sizes > 0
    return np.float64(np.mean(shard_loss[keep])) if keep.any() else np.float64("nan")


def _surrogate(Xf, Zf, Lmap, i, j, k, margin):
    """The mean hinge over the given triplets (one shard), without the gradient."""
    xd, zd, ld, id_, jd, kd, od = L.to_device_many(
        [Xf.reshape(-1), Zf.reshape(-1), Lmap.reshape(-1), i.astype(np.int32),
         j.astype(np.int32), k.astype(np.int32), np.array([0, i.size], dtype=np.int64)])
    g = _Grad(1, i.size, Xf.shape[1], Lmap.shape[0])
    g.launch(xd, zd, ld, id_, jd, kd, od, margin, 0, L.stream_handle())
    return np.float64(g.loss.cpu().numpy()[0])


# --------------------------------------------------------------------------------- the API
def project(A, Lmap):
    """A Lmap^T, (rows, p), in the bit-exact order of the module's docstring."""
    Af = _check_rows(A, "A")
    Lmap = _check_map(Lmap, Af.shape[1])
    rows, p = Af.shape[0], Lmap.shape[0]
    L.device()
    if rows == 0:
        return np.empty((0, p))
    ad, ld = L.to_device_many([Af.reshape(-1), Lmap.reshape(-1)])
    out = L.empty((rows * p,), L.torch().float64)
    L.call("tw_triplet_project", ad, rows, Af.shape[1], ld, p, out, L.stream_handle())
    return out.cpu().numpy().reshape(rows, p)


def loss_grad(X, Z, Lmap, i, j, k, margin=1.0, trip_off=None):
    """(loss, G, active) of the given triplets: shard s holds triplets [trip_off[s],
    trip_off[s + 1]) (None: one shard); loss and G (p, d) are the means over non-empty shards of
    the shard means, active the uint64 counts of S > 0 per shard."""
    Xf, Zf = T._check(X, Z, "gt")
    Lmap = _check_map(Lmap, Xf.shape[1])
    i, j, k = _check_triplets(i, j, k, Xf.shape[0], Zf.shape[0])
    off = _check_trip_off(trip_off, i.size)
    margin = float(margin)
    if margin != margin:
        raise ValueError("margin is NaN")
    L.device()
    sizes = np.diff(off)
    xd, zd, ld, id_, jd, kd, od = L.to_device_many(
        [Xf.reshape(-1), Zf.reshape(-1), Lmap.reshape(-1), i.astype(np.int32),
         j.astype(np.int32), k.astype(np.int32), off])
    g = _Grad(len(sizes), int(sizes.max()) if len(sizes) else 0, Xf.shape[1], Lmap.shape[0])
    g.launch(xd, zd, ld, id_, jd, kd, od, margin, 1, L.stream_handle())
    ns = len(sizes)
    return (_loss_of(g.loss.cpu().numpy()[:ns], sizes), g.G.cpu().numpy().reshape(Lmap.shape),
            g.active.cpu().numpy()[:ns].view(np.uint64))


def _plan(X, Z, p_learn, optim_type):
    """Everything learning_process reads, checked: a dict, or a ValueError before any device
    work or RNG draw."""
    if optim_type not in OPTIMS:
        raise ValueError(f"optim_type={optim_type!r} is not one of {list(OPTIMS)}")
    Xf, Zf = T._check(X, Z, "gt")
    try:
        need = {key: p_learn[key] for key in ("n_it", "N", "B", "margin", "reg", "learning_rate",
                                              "reshuffle_mod", "eval_mod", "L_init")}
    except KeyError as e:
        raise ValueError(f"p_learn has no {e.args[0]!r}") from None
    ints = {}
    for key, least in (("n_it", 0), ("N", 1), ("B", 1), ("reshuffle_mod", 1), ("eval_mod", 1)):
        v = need[key]
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < least:
            raise ValueError(f"p_learn[{key!r}] = {v!r} must be an integer >= {least}")
        ints[key] = int(v)
    n_monitor = p_learn.get("n_monitor", 0)
    if not isinstance(n_monitor, (int, np.integer)) or n_monitor < 0:
        raise ValueError(f"p_learn['n_monitor'] = {n_monitor!r} must be an integer >= 0")
    floats = {}
    for key in ("margin", "reg", "learning_rate"):
        try:
            floats[key] = float(need[key])
        except (TypeError, ValueError):
            raise ValueError(f"p_learn[{key!r}] = {need[key]!r} is not a number") from None
        if floats[key] != floats[key]:
            raise ValueError(f"p_learn[{key!r}] is NaN")
    L0 = _check_map(need["L_init"], Xf.shape[1])
    k, kz = int(Xf.shape[0] / ints["N"]), int(Zf.shape[0] / ints["N"])
    if k < 2 or kz < 1:
        raise ValueError(f"N = {ints['N']} blocks of {k} row(s) of X and {kz} of Z: a block "
                         f"needs at least 2 rows of X and 1 of Z")
    test = _check_test(p_learn, Xf.shape[1])
    return dict(ints, **floats, Xf=Xf, Zf=Zf, L0=L0, k=k, kz=kz, test=test,
                n_monitor=int(n_monitor), momentum=int(optim_type == "momentum"))


def _check_test(p_learn, d):
    """(test_X, test_Z) as the device reads them, or None when neither is given."""
    tx, tz = p_learn.get("test_X"), p_learn.get("test_Z")
    if tx is None and tz is None:
        return None
    if tx is None or tz is None:
        raise ValueError("p_learn has one of test_X and test_Z without the other")
    txf, tzf = T._check(tx, tz, "gt")
    if txf.shape[1] != d:
        raise ValueError(f"the test samples have {txf.shape[1]} coordinates, the map {d}")
    return txf, tzf


def _period_draws(S, N, B, k, kz):
    """The draws of S consecutive steps, every block's (i, j, q) in order: three int64 arrays of
    shape (S, N, B), block-relative, j already moved past i."""
    try:  # the 3 N S calls in their order, in one native call into one flat array
        with Session() as rng:
            flat = rng.randint_flat(np.zeros(3 * N * S, dtype=np.int64),
                                    np.tile(np.array([k, k - 1, kz], dtype=np.int64), N * S),
                                    np.full(3 * N * S, B, dtype=np.int64))
        dr = flat.reshape(S, N, 3, B)
    except NotImplementedError:  # the global generator is not the legacy MT19937
        dr = np.empty((S, N, 3, B), dtype=np.int64)
        for s in range(S):
            for b in range(N):
                dr[s, b, 0] = np.random.randint(0, k, B)
                dr[s, b, 1] = np.random.randint(0, k - 1, B)
                dr[s, b, 2] = np.random.randint(0, kz, B)
    i, j, q = dr[:, :, 0], dr[:, :, 1], dr[:, :, 2]
    return i, j + (j >= i), q


def learning_process(X, Z, p_learn, optim_type="momentum"):
    """SGD on the triplet hinge over reshuffled shards; returns the final Lmap (p, d).

    Keys read from p_learn: n_it, N, B, margin, reg, learning_rate, reshuffle_mod, eval_mod,
    L_init; optional: test_X, test_Z, n_monitor (0), test_complete (False).  RNG order (the
    global legacy np.random): the train monitor triplets (n_monitor > 0), then the test ones
    (test sets given), as triplets._draw_triplets draws them; then, for it in range(n_it): at
    it % reshuffle_mod == 0, px = permutation(n) and pz = permutation(m) — block b holds rows
    px[b k : (b + 1) k] and pz[b kz : (b + 1) kz], k = int(n / N), kz = int(m / N), the
    remainders left out for that period; at it % eval_mod == 0 an evaluation_step (it draws
    nothing); then every block's draws in order, i = randint(0, k, B), j = randint(0, k - 1, B),
    j += (j >= i), q = randint(0, kz, B).  X, Z and L_init are never modified.

    X, Z, L and delta stay on the device for the whole run; a step is the gradient launch, its
    reduction and the update, and nothing is copied back or waited for between steps outside
    the evaluations.  The draws of up to a reshuffle period go up in one copy."""
    P = _plan(X, Z, p_learn, optim_type)
    Xf, Zf, N, B, k, kz = P["Xf"], P["Zf"], P["N"], P["B"], P["k"], P["kz"]
    n, m, d, p = Xf.shape[0], Zf.shape[0], Xf.shape[1], P["L0"].shape[0]
    L.device()
    t = L.torch()
    p_learn["train_X"], p_learn["train_Z"] = Xf, Zf
    p_learn.pop("train_monitor", None)  # (an earlier run's)
    p_learn.pop("test_monitor", None)
    if P["n_monitor"] > 0:
        p_learn["train_monitor"] = T._draw_triplets(n, m, P["n_monitor"])
        if P["test"] is not None:
            p_learn["test_monitor"] = T._draw_triplets(P["test"][0].shape[0],
                                                       P["test"][1].shape[0], P["n_monitor"])
    xd, zd, Ld, off = L.to_device_many([Xf.reshape(-1), Zf.reshape(-1), P["L0"].reshape(-1),
                                        np.arange(N + 1, dtype=np.int64) * B])
    delta = t.zeros((p * d,), dtype=t.float64, device=xd.device)
    grad = _Grad(N, B, d, p)
    step_bytes = 4 * N * B
    chunk_steps = max(1, CHUNK_TRIPLETS // (N * B))
    bx, bz = (np.arange(N) * k)[None, :, None], (np.arange(N) * kz)[None, :, None]
    it, n_it = 0, P["n_it"]
    px = pz = None
    while it < n_it:
        if it % P["reshuffle_mod"] == 0:
            px = np.random.permutation(n)
            pz = np.random.permutation(m)
        if it % P["eval_mod"] == 0:  # (before the chunk's draws: an evaluation draws nothing)
            evaluation_step(it, Ld.cpu().numpy().reshape(p, d), p_learn)
        until = min(n_it, (it // P["reshuffle_mod"] + 1) * P["reshuffle_mod"], it + chunk_steps)
        S = until - it
        i, j, q = _period_draws(S, N, B, k, kz)
        (idx,) = L.to_device_many(
            [np.stack([px[bx + i], px[bx + j], pz[bz + q]], axis=1).astype(np.int32)], pinned=True)
        base = idx.data_ptr()  # (S, 3, N, B) int32; idx stays referenced through the chunk
        stream = L.stream_handle()
        for s in range(S):
            if s and (it + s) % P["eval_mod"] == 0:
                evaluation_step(it + s, Ld.cpu().numpy().reshape(p, d), p_learn)
            at = base + 3 * s * step_bytes
            grad.launch(xd, zd, Ld, ctypes.c_void_p(at), ctypes.c_void_p(at + step_bytes),
                        ctypes.c_void_p(at + 2 * step_bytes), off, P["margin"], 1, stream)
            L.call("tw_triplet_sgd_update", grad.G, Ld, delta, p * d, P["reg"],
                   P["learning_rate"], P["momentum"], stream)
        it = until
    return Ld.cpu().numpy().reshape(p, d)


def evaluation_step(it, Lmap, p_learn):
    """Appends to lists in p_learn (made when missing); draws nothing.  "iter": it.  With
    p_learn["train_monitor"] = (i, j, k) on p_learn["train_X"] / ["train_Z"] (learning_process
    sets them): "train_loss", the mean hinge over those triplets plus reg |L|_F^2 / 2, and
    "train_stat", triplets.UB_indices on the projected samples over the same triplets.  With
    "test_monitor" on "test_X" / "test_Z": "test_loss" and "test_stat" likewise.  With
    "test_complete" and the test samples: "test_stat_complete", triplets.Un of the projected
    test samples (algo="sorted").  Entries whose inputs are absent are not appended."""
    sets = []
    for name in ("train", "test"):
        A, Bz = p_learn.get(name + "_X"), p_learn.get(name + "_Z")
        if A is None or Bz is None:
            sets.append(None)
            continue
        Af, Bf = T._check(A, Bz, "gt")
        sets.append((Af, Bf))
    d = next((s[0].shape[1] for s in sets if s is not None), None)
    if d is None:
        if not isinstance(Lmap, np.ndarray) or Lmap.ndim != 2:
            raise ValueError("Lmap must be a NumPy array of shape (p, d)")
        d = Lmap.shape[1]
    Lmap = _check_map(Lmap, d)
    if any(s is not None and s[0].shape[1] != d for s in sets):
        raise ValueError("the train and test samples differ in their number of coordinates")
    mons = []
    for name, s in zip(("train", "test"), sets):
        mon = p_learn.get(name + "_monitor")
        mons.append(None if mon is None or s is None else
                    _check_triplets(*mon, s[0].shape[0], s[1].shape[0]))
    margin, reg = float(p_learn["margin"]), float(p_learn["reg"])
    penalty = reg * float(np.sum(Lmap * Lmap)) / 2
    p_learn.setdefault("iter", []).append(it)
    for name, s, mon in zip(("train", "test"), sets, mons):
        if mon is None or mon[0].size == 0:
            continue
        PA, PB = project(s[0], Lmap), project(s[1], Lmap)
        p_learn.setdefault(name + "_loss", []).append(
            np.float64(_surrogate(s[0], s[1], Lmap, *mon, margin) + penalty))
        p_learn.setdefault(name + "_stat", []).append(T.UB_indices(PA, PB, *mon))
    if p_learn.get("test_complete", False) and sets[1] is not None:
        p_learn.setdefault("test_stat_complete", []).append(
            T.Un(project(sets[1][0], Lmap), project(sets[1][1], Lmap), algo="sorted"))
