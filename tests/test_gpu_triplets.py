"""tuplewise.triplets on the device against the NumPy oracle of tests/test_triplets_cpu.py: the
distance rows bit for bit (the test that catches an FMA or another summation order), per-anchor
counts exactly with both count algorithms and under forced batching, the indexed kernel on
hand-made triplets, and the estimators' values, in-place shuffles and RNG consumption exactly."""
import functools

import numpy as np
import pytest

from test_triplets_cpu import (MODES, data, o_counts, o_dist_pairs, o_dist_rows, o_own_rows, o_UB,
                               o_UB_indices, o_Un, o_UnN, o_UnNB, o_UnNBT, o_UnNT, same_state)

pytestmark = pytest.mark.gpu

# (d, n, m) with n and m as functions of the point-tile edge P: every d of {1, 2, 3, 8, 17, 37,
# 64}, every n of {2, 3, 65, P-1, P, P+1, 2P+3} and every m of {1, 5, P+1} appears
SHAPES = {
    "d1-n2-m1": (1, lambda P: 2, lambda P: 1),
    "d2-n3-m5": (2, lambda P: 3, lambda P: 5),
    "d3-n65-mP+1": (3, lambda P: 65, lambda P: P + 1),
    "d8-nP-1-m5": (8, lambda P: P - 1, lambda P: 5),
    "d17-nP-m1": (17, lambda P: P, lambda P: 1),
    "d37-nP+1-mP+1": (37, lambda P: P + 1, lambda P: P + 1),
    "d64-n2P+3-m5": (64, lambda P: 2 * P + 3, lambda P: 5),
    "d64-n65-mP+1": (64, lambda P: 65, lambda P: P + 1),
    "d8-n2P+3-mP+1": (8, lambda P: 2 * P + 3, lambda P: P + 1),
}
GUARD = 64  # sentinel entries behind each workspace: nothing may be written there


@pytest.fixture(scope="module")
def tr(gpu):
    import tuplewise.triplets as m
    return m


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_triplet_rows_tile())


@functools.lru_cache(maxsize=None)
def case(shape, P, kind):
    """One data set of a shape and its reference (computed once, shared, never modified):
    X, Z, the other rows, the own rows, the "gt" and "half" counts per anchor."""
    d, fn, fm = SHAPES[shape]
    n, m = fn(P), fm(P)
    X, Z = data(kind, n, m, d, 1000 * d + n + m)
    return X, Z, o_dist_rows(X, Z), o_own_rows(X), o_counts(X, Z, "gt"), o_counts(X, Z, "half")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def raw_rows(tw, X, Z, bxo, bzo, a_begin, a_end, blk_first=None, blk_count=None):
    """tw_triplet_rows called directly on blocks (bxo, bzo) for anchors [a_begin, a_end): the
    per-anchor lists of "other" and "own" rows, read back from sentinel-filled workspaces."""
    import torch
    L = tw._lib
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb, mb = np.diff(bxo), np.diff(bzo)
    blk = np.searchsorted(bxo, np.arange(a_begin, a_end), side="right") - 1
    oo = np.concatenate([[0], np.cumsum(mb[blk])]).astype(np.int64)
    wo = np.concatenate([[0], np.cumsum(nb[blk] - 1)]).astype(np.int64)
    xd, zd, bxd, bzd, ood, wod = (L.to_device(np.ascontiguousarray(a).reshape(-1))
                                  for a in (X, Z, bxo, bzo, oo, wo))
    other = torch.full((int(oo[-1]) + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    own = torch.full((int(wo[-1]) + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    first = int(blk[0]) if blk_first is None else blk_first
    count = int(blk[-1]) - first + 1 if blk_count is None else blk_count
    L.call("tw_triplet_rows", xd, zd, X.shape[1], bxd, bzd, first, count, a_begin, a_end,
           int(nb.max()), int(mb.max()), ood, wod, other, own, L.stream_handle())
    other, own = other.cpu().numpy(), own.cpu().numpy()
    assert np.all(other[oo[-1]:] == -7.0) and np.all(own[wo[-1]:] == -7.0)
    return ([other[oo[q]:oo[q + 1]] for q in range(a_end - a_begin)],
            [own[wo[q]:wo[q + 1]] for q in range(a_end - a_begin)])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_rows_bit_for_bit(tw, gpu, tile, shape):
    X, Z, want_other, want_own = case(shape, tile, "nan")[:4]
    n, m = X.shape[0], Z.shape[0]
    other, own = raw_rows(tw, X, Z, [0, n], [0, m], 0, n)
    assert np.isnan(want_other).any() and np.isnan(want_own).any()  # NaN positions included
    assert np.array_equal(bits(np.concatenate(other)), bits(want_other))
    assert np.array_equal(bits(np.concatenate(own)), bits(want_own))


def test_rows_of_a_range_inside_mixed_blocks(tw, gpu, tile):
    nx, nz = [2, tile + 3, 5, 64], [3, 5, tile + 1, 1]
    bxo, bzo = np.concatenate([[0], np.cumsum(nx)]), np.concatenate([[0], np.cumsum(nz)])
    X, Z = data("nan", int(bxo[-1]), int(bzo[-1]), 5, 77)
    want_other, want_own = [], []
    for b in range(4):
        xb, zb = X[bxo[b]:bxo[b + 1]], Z[bzo[b]:bzo[b + 1]]
        want_other += list(o_dist_rows(xb, zb))
        want_own += list(o_own_rows(xb))
    # the range starts and ends in the middle of a block: blocks 0..3, 1..3 and 1 alone
    every = dict(blk_first=0, blk_count=4)  # naming more blocks than the range touches
    for a_begin, a_end, extra in ((1, int(bxo[3]) + 30, {}), (2 + tile // 2, int(bxo[4]) - 1, {}),
                                  (7, tile - 20, {}), (7, tile - 20, every)):
        other, own = raw_rows(tw, X, Z, bxo, bzo, a_begin, a_end, **extra)
        for q, a in enumerate(range(a_begin, a_end)):
            assert np.array_equal(bits(other[q]), bits(want_other[a])), (a_begin, a)
            assert np.array_equal(bits(own[q]), bits(want_own[a])), (a_begin, a)


@pytest.mark.parametrize("kind", ["nan", "ties"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_counts_exact(tr, tile, shape, kind):
    X, Z = case(shape, tile, kind)[:2]
    for mode, want in zip(MODES, case(shape, tile, kind)[4:]):
        if kind == "ties" and mode == "half" and X.shape[0] > 3:
            assert (want > 2 * case(shape, tile, kind)[4]).any()  # ties are really exercised
        got = {algo: tr.triplet_counts(X, Z, mode, algo) for algo in ("pairs", "sorted", None)}
        for algo, g in got.items():
            assert g.dtype == np.uint64 and np.array_equal(g, want), (mode, algo)
        assert tr.Un(X, Z, mode) == o_Un(X, Z, mode)


@pytest.mark.parametrize("mode", MODES)
def test_counts_unchanged_by_batching(tr, monkeypatch, mode):
    X, Z = data("ties", 65, 5, 3, 5)
    want = o_counts(X, Z, mode)
    row = 8 * (5 + 64)  # one anchor's two rows
    assert [a1 - a0 for a0, a1 in tr.batch_edges([5 + 64] * 65, 30 * row)] == [30, 30, 5]
    for cap in (30 * row, 30 * row + 7, row, 1):  # 3 batches with a ragged last one; 65 of one
        monkeypatch.setattr(tr, "ROWS_BYTES", cap)
        for algo in ("pairs", "sorted"):
            assert np.array_equal(tr.triplet_counts(X, Z, mode, algo), want), (cap, algo)
    # the blocks of one UnN straddle the batches
    Xs, Zs = data("nan", 70, 31, 4, 6)
    Xo, Zo = Xs.copy(), Zs.copy()
    monkeypatch.setattr(tr, "ROWS_BYTES", 8 * (10 + 22) * 9)
    np.random.seed(3)
    got = tr.UnN(Xs, Zs, 3, mode=mode)
    np.random.seed(3)
    assert got == o_UnN(Xo, Zo, 3, mode) and np.array_equal(bits(Xs), bits(Xo))


def raw_idx(tw, X, Z, i, j, k, off, mode):
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns = len(off) - 1
    max_t = int(np.diff(off).max())
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    id_, jd, kd = (L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, k))
    od = L.to_device(off)
    work = L.empty((L.lib().tw_triplet_idx_work_bytes(ns, max_t) // 8,), torch.int64)
    out = torch.full((ns,), -7, dtype=torch.int64, device=xd.device)
    pred = {"gt": L.TW_PRED_GT, "half": L.TW_PRED_HALF}[mode]
    L.call("tw_triplet_idx32", xd, zd, X.shape[1], id_, jd, kd, od, ns, max_t, pred, work, out,
           L.stream_handle())
    return out.cpu().numpy().view(np.uint64)


def o_idx_count(X, Z, i, j, k, mode):
    other, own = o_dist_pairs(X[i], Z[k]), o_dist_pairs(X[i], X[j])
    with np.errstate(invalid="ignore"):
        gt, eq = int(np.sum(other > own)), int(np.sum(other == own))
    return gt if mode == "gt" else 2 * gt + eq


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind,d", [("ties", 2), ("nan", 37)])
def test_indexed(tw, tr, kind, d, mode):
    n, m = 40, 23
    X, Z = data(kind, n, m, d, 1)
    # hand-made: j adjacent to i on both sides, repeated triplets, the last rows, negative
    # indices as NumPy reads them
    i = np.array([0, 1, 5, 5, 5, 39, 38, 13, 13, -1, 0])
    j = np.array([1, 0, 4, 6, 6, 38, 39, 12, 14, 0, -1])
    k = np.array([0, 22, 3, 3, 3, 22, 0, 11, 11, -1, -23])
    got = tr.UB_indices(X, Z, i, j, k, mode)
    assert isinstance(got, np.float64) and got == o_UB_indices(X, Z, i, j, k, mode)
    assert tr.UB_indices(X, Z, i.reshape(-1, 1), j.reshape(-1, 1), k.reshape(-1, 1), mode) == got
    none = np.zeros(0, dtype=np.int64)
    assert np.isnan(tr.UB_indices(X, Z, none, none, none, mode))
    # raw, shards of mixed sizes: a single triplet, none, more than one block's worth, a few
    rng = np.random.RandomState(4)
    sizes = [1, 0, 2500, 11, 0]
    off = np.concatenate([[0], np.cumsum(sizes)])
    T = int(off[-1])
    ri, rk = rng.randint(0, n, T), rng.randint(0, m, T)
    rj = rng.randint(0, n - 1, T)
    rj += rj >= ri
    ri[-11:], rj[-11:], rk[-11:] = i % n, j % n, k % m
    got = raw_idx(tw, X, Z, ri, rj, rk, off, mode)
    want = [o_idx_count(X, Z, ri[a:b], rj[a:b], rk[a:b], mode) for a, b in zip(off, off[1:])]
    assert [int(g) for g in got] == want and want[2] > 0
    for s in (0, 2, 3):  # a shard's count is the same alone as beside others
        a, b = off[s], off[s + 1]
        alone = raw_idx(tw, X, Z, ri[a:b], rj[a:b], rk[a:b], [0, b - a], mode)
        assert int(alone[0]) == want[s]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["gauss", "ties"])
def test_estimators(tr, kind, mode):
    n, m, d, N, B, T = 1000, 700, 5, 7, 500, 3
    X0, Z0 = data(kind, n, m, d, 21)
    runs = [("Un", lambda X, Z: tr.Un(X, Z, mode), lambda X, Z: o_Un(X, Z, mode)),
            ("UB", lambda X, Z: tr.UB(X, Z, B, mode), lambda X, Z: o_UB(X, Z, B, mode)),
            ("UnN", lambda X, Z: tr.UnN(X, Z, N, mode=mode), lambda X, Z: o_UnN(X, Z, N, mode)),
            ("UnNB", lambda X, Z: tr.UnNB(X, Z, N, B, mode=mode),
             lambda X, Z: o_UnNB(X, Z, N, B, mode)),
            ("UnNT", lambda X, Z: tr.UnNT(X, Z, N, T, mode=mode),
             lambda X, Z: o_UnNT(X, Z, N, T, mode)),
            ("UnNBT", lambda X, Z: tr.UnNBT(X, Z, N, B, T, mode=mode),
             lambda X, Z: o_UnNBT(X, Z, N, B, T, mode))]
    for seed, (name, f, o) in enumerate(runs):
        X, Z, Xo, Zo = X0.copy(), Z0.copy(), X0.copy(), Z0.copy()
        np.random.seed(100 + seed)
        got = f(X, Z)
        state = np.random.get_state()
        np.random.seed(100 + seed)
        want = o(Xo, Zo)
        assert isinstance(got, np.float64) and got == want, (name, got, want)
        assert 0.0 < got < 1.0
        assert np.array_equal(X, Xo) and np.array_equal(Z, Zo), name
        assert same_state(state, np.random.get_state()), name
    # UN with a callable of the caller's own goes block by block, the same partition
    X, Z, Xo, Zo = X0.copy(), Z0.copy(), X0.copy(), Z0.copy()
    np.random.seed(9)
    got = tr.UN(X, Z, N, lambda x, z: tr.Un(x, z, mode))
    np.random.seed(9)
    assert got == o_UnN(Xo, Zo, N, mode) and np.array_equal(X, Xo)


def test_one_dimensional_samples(tr):
    rng = np.random.RandomState(8)
    X, Z = rng.normal(size=300), rng.normal(0.5, 1.0, size=130)
    assert np.array_equal(tr.triplet_counts(X, Z), o_counts(X, Z, "gt"))
    Xo, Zo = X.copy(), Z.copy()
    np.random.seed(1)
    got = tr.UnNB(X, Z, 4, 50, mode="half")
    np.random.seed(1)
    assert got == o_UnNB(Xo, Zo, 4, 50, "half") and np.array_equal(X, Xo)
