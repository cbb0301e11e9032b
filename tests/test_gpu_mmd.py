"""tuplewise.mmd on the device against the NumPy oracle of tests/test_mmd_cpu.py: the three
component sums of tw_mmd_sums at rtol 1e-12 (one block, mixed block sizes in one launch, offsets
that do not start at 0, sentinels behind the outputs), the exact properties (run-to-run bits, a
block alone and beside others, duplicated rows, NaN placement), the indexed kernel on hand-made
quadruples, and the estimators' values, in-place shuffles and RNG consumption.

Tolerances: the distances and c * D are bit-identical on both sides, exp is within an ulp or so of
NumPy's, sqrt is exact and the terms are non-negative, so the component sums agree to the
package's rtol 1e-12 for float sums whatever the order of summation.  The statistic cancels, so
values are compared at atol = 1e-12 * (|2 Sxx / (n (n - 1))| + |2 Szz / (m (m - 1))| +
|2 Sxz / (n m)|), the indexed ones at 1e-12 * (s0 + s1 + s2 + s3) / B, both from the oracle."""
import functools
import math

import numpy as np
import pytest

from test_mmd_cpu import (KERNELS, o_components, o_draw, o_idx_sums, o_sign, o_UB_indices,
                          o_UB_scale, o_Un, o_Un_scale, o_UN)
from test_triplets_cpu import same_state

pytestmark = pytest.mark.gpu

RTOL = 1e-12
# (d, n, m) with n and m as functions of the tile edge P: every d of {1, 2, 3, 8, 17, 37, 64},
# every n of {2, 3, 65, P-1, P, P+1, 2P+3} and every m of {2, 5, P+1} appears
SHAPES = {
    "d1-n2-m2": (1, lambda P: 2, lambda P: 2),
    "d2-n3-m5": (2, lambda P: 3, lambda P: 5),
    "d3-n65-mP+1": (3, lambda P: 65, lambda P: P + 1),
    "d8-nP-1-m5": (8, lambda P: P - 1, lambda P: 5),
    "d17-nP-m2": (17, lambda P: P, lambda P: 2),
    "d37-nP+1-mP+1": (37, lambda P: P + 1, lambda P: P + 1),
    "d64-n2P+3-m5": (64, lambda P: 2 * P + 3, lambda P: 5),
    "d64-n65-mP+1": (64, lambda P: 65, lambda P: P + 1),
    "d8-n2P+3-mP+1": (8, lambda P: 2 * P + 3, lambda P: P + 1),
}
GUARD = 64  # sentinel entries behind d_out and d_work: nothing may be written there


@pytest.fixture(scope="module")
def mm(gpu):
    import tuplewise.mmd as m
    return m


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_mmd_tile())


def sigma_of(kernel, d):
    return math.sqrt(d) if kernel == "gaussian" else None


def coef(tw, kernel, d):
    if kernel == "gaussian":
        s = sigma_of(kernel, d)
        return tw._lib.TW_MMD_GAUSSIAN, -1.0 / (2.0 * s * s)
    return tw._lib.TW_MMD_ENERGY, 0.0


def mmd_data(kind, n, m, d, seed):
    """"gauss": standard normal X, Z shifted by 0.2; "ties": the same with duplicated rows inside
    X, inside Z and across them; "nan": one NaN coordinate in X; "nanz": one in Z."""
    rng = np.random.RandomState(seed)
    X, Z = rng.normal(size=(n, d)), rng.normal(0.2, 1.0, size=(m, d))
    if kind == "ties":
        X[n - 1] = X[0]
        Z[m - 1] = Z[0]
        if n > 2 and m > 2:
            X[n // 2], Z[m // 2] = X[0], X[0]
    if kind == "nan":
        X[n // 3, d // 2] = np.nan
    if kind == "nanz":
        Z[m // 3, d // 2] = np.nan
    return X, Z


@functools.lru_cache(maxsize=None)
def case(shape, P, kind, kernel):
    """One data set of a shape and its reference (computed once, shared, never modified)."""
    d, fn, fm = SHAPES[shape]
    n, m = fn(P), fm(P)
    X, Z = mmd_data(kind, n, m, d, 1000 * d + n + m)
    return X, Z, o_components(X, Z, kernel, sigma_of(kernel, d))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


def raw_sums(tw, X, Z, bxo, bzo, kernel):
    """tw_mmd_sums called directly on blocks (bxo, bzo): the (n_blocks, 3) sums, read back from
    sentinel-filled d_out and d_work."""
    import torch
    L = tw._lib
    bxo, bzo = np.asarray(bxo, dtype=np.int64), np.asarray(bzo, dtype=np.int64)
    nb = len(bxo) - 1
    max_n, max_m = int(np.diff(bxo).max()), int(np.diff(bzo).max())
    kid, c = coef(tw, kernel, X.shape[1])
    xd, zd, bxd, bzd = (L.to_device(np.ascontiguousarray(a).reshape(-1)) for a in (X, Z, bxo, bzo))
    nwork = int(L.lib().tw_mmd_work_bytes(nb, max_n, max_m)) // 8
    work = torch.full((nwork + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    out = torch.full((3 * nb + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    L.call("tw_mmd_sums", xd, zd, X.shape[1], bxd, bzd, nb, max_n, max_m, kid, c, work, out,
           L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(-7.0)) and np.all(bits(out[3 * nb:]) == bits(-7.0))
    return out[:3 * nb].reshape(nb, 3)


def close(got, want, what=None):
    """rtol 1e-12, NaN exactly where the oracle has NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    print(what, "got", got.tolist(), "want", want.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, got, want)
    ok = ~np.isnan(want)
    assert np.all(np.abs(got[ok] - want[ok]) <= RTOL * np.abs(want[ok])), (what, got, want)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_components_one_block(tw, mm, tile, shape, kernel):
    X, Z, want = case(shape, tile, "gauss", kernel)
    n, m = X.shape[0], Z.shape[0]
    got = raw_sums(tw, X, Z, [0, n], [0, m], kernel)
    close(got[0], want, shape)
    assert np.array_equal(bits(raw_sums(tw, X, Z, [0, n], [0, m], kernel)), bits(got))  # same bits
    pub = mm.components(X, Z, kernel, sigma_of(kernel, X.shape[1]))
    assert all(isinstance(v, np.float64) for v in pub) and np.array_equal(bits(pub), bits(got))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind", ["ties", "nan", "nanz"])
@pytest.mark.parametrize("shape", ["d2-n3-m5", "d37-nP+1-mP+1", "d8-n2P+3-mP+1"])
def test_components_ties_and_nan(tw, tile, shape, kind, kernel):
    X, Z, want = case(shape, tile, kind, kernel)
    if kind == "nan":
        assert np.isnan(want[0]) and not np.isnan(want[1]) and np.isnan(want[2])
    if kind == "nanz":
        assert not np.isnan(want[0]) and np.isnan(want[1]) and np.isnan(want[2])
    close(raw_sums(tw, X, Z, [0, X.shape[0]], [0, Z.shape[0]], kernel)[0], want, (shape, kind))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("d", [1, 8, 17, 64])
def test_duplicated_rows_are_exact(tw, d, kernel):
    """Two equal rows: D = 0 exactly, so the Gaussian term is exactly 1 and the energy term
    exactly 0 — Sxx and Szz are that one term."""
    rng = np.random.RandomState(d)
    X, Z = np.repeat(rng.normal(size=(1, d)), 2, axis=0), np.repeat(rng.normal(size=(1, d)), 2, axis=0)
    got = raw_sums(tw, X, Z, [0, 2], [0, 2], kernel)[0]
    one = 1.0 if kernel == "gaussian" else 0.0
    assert np.array_equal(bits(got[:2]), bits([one, one])), got
    close(got, o_components(X, Z, kernel, sigma_of(kernel, d)))


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_blocks_in_one_launch(tw, tile, kernel):
    P, d = tile, 5
    nx, nz = [2, P + 1, 65, 2 * P + 3], [2, 5, P + 1, 3]
    want = None
    for gx, gz in ((0, 0), (7, 3)):  # the partition at 0, then behind a leading gap of rows
        bxo, bzo = gx + np.concatenate([[0], np.cumsum(nx)]), gz + np.concatenate([[0], np.cumsum(nz)])
        X, Z = mmd_data("gauss", int(bxo[-1]) - gx, int(bzo[-1]) - gz, d, 77)
        if want is None:
            want = [o_components(X[a:b], Z[e:f], kernel, sigma_of(kernel, d))
                    for a, b, e, f in zip(bxo, bxo[1:], bzo, bzo[1:])]
        X = np.concatenate([np.full((gx, d), 1e3), X])  # rows no block owns: far away, so a
        Z = np.concatenate([np.full((gz, d), -1e3), Z])  # block-relative offset shows in the sums
        got = raw_sums(tw, X, Z, bxo, bzo, kernel)
        for b in range(4):
            close(got[b], want[b], (gx, b))
        assert np.array_equal(bits(raw_sums(tw, X, Z, bxo, bzo, kernel)), bits(got))
        for b in range(4):  # a block alone in a launch: the same bits as beside the others
            alone = raw_sums(tw, X, Z, bxo[b:b + 2], bzo[b:b + 2], kernel)
            assert np.array_equal(bits(alone[0]), bits(got[b])), (gx, b)
        if gx == 0:
            first = got
        else:  # and the same bits wherever the partition starts
            assert np.array_equal(bits(got), bits(first))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("shape", ["d3-n65-mP+1", "d17-nP-m2", "d64-n2P+3-m5"])
def test_same_sample_twice(tw, tile, shape, kernel):
    """Z = X.copy(): the rectangle holds every unordered pair twice and the n pairs (i, i)."""
    X = case(shape, tile, "gauss", kernel)[0]
    n = X.shape[0]
    sxx, szz, sxz = raw_sums(tw, X, X.copy(), [0, n], [0, n], kernel)[0]
    g0 = 1.0 if kernel == "gaussian" else 0.0
    print(shape, kernel, sxx, szz, sxz)
    assert abs(sxx - szz) <= RTOL * sxx  # (the two triangles are grouped into workgroups apart)
    assert abs(sxz - (2.0 * sxx + n * g0)) <= RTOL * abs(2.0 * sxx + n * g0)


def raw_idx(tw, X, Z, i, j, k, l, off, kernel):  # noqa: E741
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns = len(off) - 1
    max_q = int(np.diff(off).max())
    kid, c = coef(tw, kernel, X.shape[1])
    xd, zd = L.to_device(X.reshape(-1)), L.to_device(Z.reshape(-1))
    id_, jd, kd, ld = (L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, k, l))
    od = L.to_device(off)
    nwork = int(L.lib().tw_mmd_idx_work_bytes(ns, max_q)) // 8
    work = torch.full((nwork + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    out = torch.full((4 * ns + GUARD,), -7.0, dtype=torch.float64, device=xd.device)
    L.call("tw_mmd_idx32", xd, zd, X.shape[1], id_, jd, kd, ld, od, ns, max_q, kid, c, work, out,
           L.stream_handle())
    work, out = work.cpu().numpy(), out.cpu().numpy()
    assert np.all(bits(work[nwork:]) == bits(-7.0)) and np.all(bits(out[4 * ns:]) == bits(-7.0))
    return out[:4 * ns].reshape(ns, 4)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("kind,d", [("ties", 2), ("gauss", 37), ("nan", 8)])
def test_indexed(tw, mm, kind, d, kernel):
    n, m = 40, 23
    X, Z = mmd_data(kind, n, m, d, 1)
    sigma = sigma_of(kernel, d)
    # hand-made: neighbours on both sides, repeated quadruples, the last rows, negative indices
    # as NumPy reads them
    i = np.array([0, 1, 5, 5, 5, 39, 38, 13, 13, -1, 0])
    j = np.array([1, 0, 4, 6, 6, 38, 39, 12, 14, 0, -1])
    k = np.array([0, 22, 3, 3, 3, 22, 0, 11, 11, -1, -23])
    l = np.array([1, 21, 4, 2, 2, 0, 22, 12, 10, 0, -1])  # noqa: E741
    if kind != "nan":
        got = mm.UB_indices(X, Z, i, j, k, l, kernel, sigma)
        want = o_UB_indices(X, Z, i, j, k, l, kernel, sigma)
        tol = RTOL * o_UB_scale(X, Z, i, j, k, l, kernel, sigma)
        print(kind, kernel, got, want, tol)
        assert isinstance(got, np.float64) and abs(got - want) <= tol
        col = [a.reshape(-1, 1) for a in (i, j, k, l)]
        assert mm.UB_indices(X, Z, *col, kernel, sigma) == got
    none = np.zeros(0, dtype=np.int64)
    assert np.isnan(mm.UB_indices(X, Z, none, none, none, none, kernel, sigma))
    # raw, shards of mixed sizes: none, one, a few, one past a wave's quadruples, one past two
    # workgroups' worth (4 quadruples per lane, 256 lanes)
    rng = np.random.RandomState(4)
    sizes = [0, 1, 3, 257, 4 * 256 * 2 + 1, 0, 11]
    off = np.concatenate([[0], np.cumsum(sizes)])
    T = int(off[-1])
    ri, rk = rng.randint(0, n, T), rng.randint(0, m, T)
    rj, rl = rng.randint(0, n - 1, T), rng.randint(0, m - 1, T)
    rj += rj >= ri
    rl += rl >= rk
    ri[-11:], rj[-11:], rk[-11:], rl[-11:] = i % n, j % n, k % m, l % m
    got = raw_idx(tw, X, Z, ri, rj, rk, rl, off, kernel)
    for s, (a, b) in enumerate(zip(off, off[1:])):
        if a == b:
            assert np.array_equal(bits(got[s]), bits(np.zeros(4))), s  # an empty shard: zeros
        else:
            close(got[s], o_idx_sums(X, Z, ri[a:b], rj[a:b], rk[a:b], rl[a:b], kernel, sigma), s)
    assert np.array_equal(bits(raw_idx(tw, X, Z, ri, rj, rk, rl, off, kernel)), bits(got))
    for s in (1, 3, 4):  # a shard's sums are the same bits alone as beside others
        a, b = off[s], off[s + 1]
        alone = raw_idx(tw, X, Z, ri[a:b], rj[a:b], rk[a:b], rl[a:b], [0, b - a], kernel)
        assert np.array_equal(bits(alone[0]), bits(got[s])), s


# ---- the estimators: the oracle's value with the magnitude its tolerance is taken from
def ref_Un(X, Z, kernel, sigma):
    return o_Un(X, Z, kernel, sigma), o_Un_scale(X, Z, kernel, sigma)


def ref_UB(X, Z, B, kernel, sigma):
    i, j, k, l = o_draw(X.shape[0], Z.shape[0], B)  # noqa: E741
    return (o_UB_indices(X, Z, i, j, k, l, kernel, sigma),
            o_UB_scale(X, Z, i, j, k, l, kernel, sigma))


def ref_blocks(X, Z, N, T, block):
    """T rounds of o_UN over `block` (value, scale): the value and the mean scale."""
    scales = []

    def f(x, z):
        v, s = block(x, z)
        scales.append(s)
        return v

    value = np.mean([o_UN(X, Z, N, f) for _ in range(T)])
    return value, float(np.mean(scales))


@pytest.mark.parametrize("kernel", KERNELS)
def test_estimators(mm, kernel):
    n, m, d, N, B, T = 103, 57, 5, 4, 500, 3
    X0, Z0 = mmd_data("gauss", n, m, d, 21)
    sg = sigma_of(kernel, d)
    kw = dict(kernel=kernel, sigma=sg)

    def un(x, z):
        return ref_Un(x, z, kernel, sg)

    def ub(b):
        return lambda x, z: ref_UB(x, z, b, kernel, sg)

    runs = [("Un", lambda X, Z: mm.Un(X, Z, **kw), un),
            ("UB", lambda X, Z: mm.UB(X, Z, 1000, **kw), ub(1000)),
            ("UnN", lambda X, Z: mm.UnN(X, Z, N, **kw), lambda X, Z: ref_blocks(X, Z, N, 1, un)),
            ("UnNB", lambda X, Z: mm.UnNB(X, Z, N, B, **kw),
             lambda X, Z: ref_blocks(X, Z, N, 1, ub(B))),
            ("UnNT", lambda X, Z: mm.UnNT(X, Z, N, T, **kw),
             lambda X, Z: ref_blocks(X, Z, N, T, un)),
            ("UnNBT", lambda X, Z: mm.UnNBT(X, Z, N, B, T, **kw),
             lambda X, Z: ref_blocks(X, Z, N, T, ub(B))),
            # UN with Un itself (its arguments bound) and with a callable of the caller's own go
            # block by block, the same partition
            ("UN(Un)", lambda X, Z: mm.UN(X, Z, N, functools.partial(mm.Un, **kw)),
             lambda X, Z: ref_blocks(X, Z, N, 1, un)),
            ("UN(callable)", lambda X, Z: mm.UN(X, Z, N, lambda x, z: float(x[0, 0] - z[-1, 1])),
             lambda X, Z: (o_UN(X, Z, N, lambda x, z: float(x[0, 0] - z[-1, 1])), 0.0))]
    for seed, (name, f, o) in enumerate(runs):
        X, Z, Xo, Zo = X0.copy(), Z0.copy(), X0.copy(), Z0.copy()
        np.random.seed(100 + seed)
        got = f(X, Z)
        state = np.random.get_state()
        np.random.seed(100 + seed)
        want, scale = o(Xo, Zo)
        print(name, kernel, got, want, RTOL * scale)
        assert isinstance(got, np.float64) and abs(got - want) <= RTOL * scale, (name, got, want)
        assert np.array_equal(bits(X), bits(Xo)) and np.array_equal(bits(Z), bits(Zo)), name
        assert same_state(state, np.random.get_state()), name
    # the sign convention: both statistics are positive for samples this far apart
    Xs, Zs = mmd_data("gauss", 200, 150, 3, 5)
    Zs += 1.0
    assert mm.Un(Xs, Zs, **(dict(kernel=kernel, sigma=sigma_of(kernel, 3)))) > 0.0
    assert o_sign(kernel) == (1.0 if kernel == "gaussian" else -1.0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_dimensional_samples(mm, kernel):
    rng = np.random.RandomState(8)
    X, Z = rng.normal(size=300), rng.normal(0.5, 1.0, size=130)
    sg = sigma_of(kernel, 1)
    got = mm.Un(X, Z, kernel, sg)
    want, scale = ref_Un(X, Z, kernel, sg)
    assert abs(got - want) <= RTOL * scale
    Xo, Zo = X.copy(), Z.copy()
    np.random.seed(1)
    got = mm.UnNB(X, Z, 4, 50, kernel=kernel, sigma=sg)
    np.random.seed(1)
    want, scale = ref_blocks(Xo, Zo, 4, 1, lambda x, z: ref_UB(x, z, 50, kernel, sg))
    assert abs(got - want) <= RTOL * scale and np.array_equal(X, Xo) and np.array_equal(Z, Zo)
