"""tw_triplet_grad at every one of its 32 kernel forms, at the hinge's edge, over many shards, and
learning_process across chunk cuts.

The form a call reaches (csrc/triplet_grad.hip: the d gates of tw_triplet_grad pick DP,
tg_launch_p picks PP, want_grad picks GRAD; G = 64 / PP triplets lie side by side in a wave and a
workgroup of 4 waves takes g = 4 G triplets per pass, 128 = tw_triplet_grad_tile() per slice):

    d in      DP  |  p in      PP   G   g
    [1, 8]     8  |  [1, 8]     8   8  32
    [9, 16]   16  |  [9, 16]   16   4  16
    [17, 32]  32  |  [17, 32]  32   2   8
    [33, 64]  64  |  [33, 64]  64   1   4

FORMS below holds the 16 (DP, PP) pairs; shapes_of gives each pair its upper edge (d, p) =
(DP, PP) and its lower edge (DP / 2 + 1, PP / 2 + 1) — 1 at 8 —, i.e. d in {8, 1}, {16, 9},
{32, 17}, {64, 33} and p likewise: both ends of the gate's interval in the table, so both reach
k_triplet_grad<DP, PP, .>.  Every case runs with want_grad = 1 (GRAD = true) and 0 (GRAD = false):
16 pairs x 2 = the 32 forms, each at triplets {1, g - 1, g, g + 1, tile - 1, tile + 1,
2 tile + 3}: a lone triplet, a last pass one short of, equal to and one over the workgroup's g, and
one, two and three slices.  The many-shard cases sit at (17, 16) -> <32, 16> and (9, 33) ->
<16, 64>, the NaN case at (16, 9) -> <16, 16>.

Real-valued data is compared with the NumPy oracle within the project's bound for unpinned
gradients, 1e-12 max(1, max|want|).  Integer data (X, Z in [-3, 3], L in [-2, 2])
makes every product, fma, butterfly, partial and shard sum an exact integer far below 2^53, so
G and the loss are one integer divided once by the shard's triplets: the kernel must give the
correctly rounded quotient bit for bit, whatever its order of addition, and the margin can be
placed so that some S is 0 exactly — the strict S > 0 then shows in the counts and in every bit.
"""
import functools
from fractions import Fraction

import numpy as np
import pytest

from test_triplets_cpu import same_state
from test_triplet_learning_cpu import (draw, make, o_hinge, o_learning_process, o_loss_grad,
                                       o_shard)
from test_triplet_learning_gpu import (TOL, bits, close, raw_grad, tile, tl,  # noqa: F401
                                       trajectory_data)

pytestmark = pytest.mark.gpu

N_ROWS, M_ROWS = 50, 40
PADS = (8, 16, 32, 64)
FORMS = [(DP, PP) for DP in PADS for PP in PADS]
SHARD_COUNTS = [16, 17, 33, 256, 257, 300]  # around kTgRedS = 16 groups and kBlock = 256 shards
SHARD_SHAPES = [(17, 16), (9, 33)]


def shapes_of(DP, PP):
    return [(DP, PP), tuple(1 if P == 8 else P // 2 + 1 for P in (DP, PP))]


def pass_of(PP):
    return 4 * (64 // PP)  # g: the triplets one pass of a workgroup takes


def counts_of(PP, S):
    g = pass_of(PP)
    return [1, g - 1, g, g + 1, S - 1, S + 1, 2 * S + 3]


# ---------------------------------------------------------------- real-valued data and reference
@functools.lru_cache(maxsize=None)
def real_case(d, p, T):
    """Data with no triplet near S = 0 (a condition on the oracle alone: the first seed of a fixed
    sequence that meets it) and its reference, computed once and never modified."""
    for seed in range(1000 * d + 10 * p, 1000 * d + 10 * p + 50):
        X, Z, Lm = make(N_ROWS, M_ROWS, d, p, seed)
        i, j, k = draw(np.random.RandomState(seed + T), N_ROWS, M_ROWS, T)
        ref = o_loss_grad(X, Z, Lm, i, j, k, 1.0)
        if ref[3] > 1e-6:
            return X, Z, Lm, i, j, k, ref
    raise AssertionError("no seed keeps every triplet away from S = 0")


# -------------------------------------------------------------------- integer data and reference
def int_data(d, p, seed):
    rng = np.random.RandomState(seed)
    return (rng.randint(-3, 4, size=(N_ROWS, d)), rng.randint(-3, 4, size=(M_ROWS, d)),
            rng.randint(-2, 3, size=(p, d)))


def int_hinge(Xi, Zi, Li, i, j, k):
    """(S at margin 0, a, b, u, v) in int64."""
    a, b = Xi[i] - Xi[j], Xi[i] - Zi[k]
    u, v = a @ Li.T, b @ Li.T
    return np.sum(u * u, axis=1) - np.sum(v * v, axis=1), a, b, u, v


def quotients(num, den):
    """The correctly rounded num / den, elementwise, from exact rationals."""
    num = np.asarray(num)
    out = np.array([float(Fraction(int(v), int(den))) for v in num.reshape(-1)], dtype=np.float64)
    return out.reshape(num.shape)


def int_reference(Xi, Zi, Li, i, j, k, margin):
    """(loss, G, active, S) of one shard from int64 sums and one exact division each."""
    S0, a, b, u, v = int_hinge(Xi, Zi, Li, i, j, k)
    S = S0 + int(margin)
    act = S > 0  # strict
    Gn = 2 * (u[act].T @ a[act] - v[act].T @ b[act])
    assert max(np.abs(Gn).max(initial=0), np.abs(S).max()) * len(S) < 1 << 52
    return quotients(S[act].sum(), len(S))[()], quotients(Gn, len(S)), int(act.sum()), S


@functools.lru_cache(maxsize=None)
def int_case(d, p, T):
    """Integer data whose lower median of S at margin 0 has triplets on both sides of it (T > 1;
    a condition on the reference alone: the first seed of a fixed sequence that meets it), with
    the margins to run: minus that median, so that S == 0 exactly there; for T = 1 also the
    margin + 1, which makes the one triplet active."""
    for seed in range(7000 + 100 * d + p, 7000 + 100 * d + p + 200):
        Xi, Zi, Li = int_data(d, p, seed)
        i, j, k = draw(np.random.RandomState(seed + T), N_ROWS, M_ROWS, T)
        S0 = int_hinge(Xi, Zi, Li, i, j, k)[0]
        margin = -int(np.sort(S0)[(T - 1) // 2])
        S = S0 + margin
        if T == 1 and Li.any():
            return Xi, Zi, Li, i, j, k, (margin, margin + 1)
        if T > 1 and (S > 0).any() and (S < 0).any():
            return Xi, Zi, Li, i, j, k, (margin,)
    raise AssertionError("no seed puts triplets on both sides of S = 0")


def as_f64(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.float64) for a in arrays)


# ------------------------------------------------------------ 1. the form matrix, real-valued
@pytest.mark.parametrize("DP,PP", FORMS)
def test_every_form_against_oracle(tw, tile, DP, PP):
    worst_G = worst_loss = 0.0
    for d, p in shapes_of(DP, PP):
        for T in counts_of(PP, tile):
            X, Z, Lm, i, j, k, (loss_o, G_o, act_o, low) = real_case(d, p, T)
            assert low > 1e-6  # no activity flip can excuse a difference
            G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], 1.0)  # (checks the sentinels)
            dG, dl = np.abs(G - G_o).max(), abs(loss[0] - loss_o)
            worst_G, worst_loss = max(worst_G, dG), max(worst_loss, dl)
            print(f"<{DP},{PP}> d={d} p={p} T={T}: max|G - G_o| = {dG:.3g} (max|G_o| = "
                  f"{np.abs(G_o).max():.3g}), |loss - loss_o| = {dl:.3g} (loss_o = {loss_o:.3g}), "
                  f"active {act[0]} of {T}")
            assert act[0] == act_o[0], (d, p, T)
            assert close(G, G_o) and close(loss[0], loss_o), (d, p, T)
            G0, loss0, act0 = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], 1.0, want_grad=0)
            assert np.all(G0 == -7.0), (d, p, T)  # d_G keeps its sentinels
            assert act0[0] == act_o[0], (d, p, T)
            assert bits(loss0)[0] == bits(loss)[0], (d, p, T)  # the gradient call's loss
    print(f"<{DP},{PP}> worst: max|G - G_o| = {worst_G:.3g}, |loss - loss_o| = {worst_loss:.3g}")


# ------------------------------------------- 2. integer data: bit equality and the S = 0 edge
@pytest.mark.parametrize("DP,PP", FORMS)
def test_every_form_exact_on_integers(tw, tile, DP, PP):
    for d, p in shapes_of(DP, PP):
        for T in counts_of(PP, tile):
            Xi, Zi, Li, i, j, k, margins = int_case(d, p, T)
            X, Z, Lm = as_f64(Xi, Zi, Li)
            for n, margin in enumerate(margins):
                loss_r, G_r, act_r, S = int_reference(Xi, Zi, Li, i, j, k, margin)
                zeros, above, below = int((S == 0).sum()), int((S > 0).sum()), int((S < 0).sum())
                if n == 0:
                    assert zeros >= 1  # a triplet sits on the hinge's edge
                    assert T == 1 or (above >= 1 and below >= 1)
                # the float oracle equals the rational reference on such data (no device involved)
                loss_o, G_o, act_o, _ = o_loss_grad(X, Z, Lm, i, j, k, float(margin))
                assert loss_o == loss_r and np.array_equal(G_o, G_r) and act_o[0] == act_r
                G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], float(margin))
                wrong = int((bits(G) != bits(G_r)).sum())
                print(f"<{DP},{PP}> d={d} p={p} T={T} margin={margin}: S == 0 at {zeros}, > 0 at "
                      f"{above}, < 0 at {below}; active {act[0]}; entries of G off {wrong}, "
                      f"max|G - G_r| = {np.abs(G - G_r).max():.3g}, loss {loss[0]!r} for "
                      f"{loss_r!r}")
                assert act[0] == act_r == above, (d, p, T, margin)  # S == 0 is not active
                # bit for bit, and so +0.0 wherever the reference is 0
                assert np.array_equal(bits(G), bits(G_r)), (d, p, T, margin)
                assert bits(loss)[0] == bits(loss_r)[0], (d, p, T, margin)
                G0, loss0, act0 = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], float(margin),
                                           want_grad=0)
                assert np.all(G0 == -7.0) and act0[0] == act_r, (d, p, T, margin)
                assert bits(loss0)[0] == bits(loss_r)[0], (d, p, T, margin)


# --------------------------------------------------------------------------- 3. many shards
def placements(ns):
    """(index of the one large shard, indices kept empty): first, last and index 16 in turn."""
    spots = [0, ns - 1] + ([16] if ns > 17 else [])
    return [(big, [s for s in spots if s != big]) for big in spots]


@functools.lru_cache(maxsize=None)
def mixed_case(ns, d, p, S, big, empty):
    """Shard sizes from {0, 1, g + 1} with the one shard of S + 3 triplets at `big` and the shards
    `empty` empty; no triplet near S = 0 (the first seed of a fixed sequence that meets it)."""
    g = pass_of(16 if p <= 16 else 64)
    for seed in range(1000 * ns + 10 * big, 1000 * ns + 10 * big + 10):
        rng = np.random.RandomState(seed)
        X, Z, Lm = make(N_ROWS, M_ROWS, d, p, seed)
        sizes = rng.choice([0, 1, g + 1], size=ns)
        sizes[list(empty)] = 0
        sizes[big] = S + 3
        off = np.concatenate([[0], np.cumsum(sizes)])
        i, j, k = draw(rng, N_ROWS, M_ROWS, int(off[-1]))
        ref = o_loss_grad(X, Z, Lm, i, j, k, 1.0, off)
        if ref[3] > 1e-6 and (sizes == 1).any() and (sizes == g + 1).any():
            return X, Z, Lm, i, j, k, off, ref
    raise AssertionError("no seed keeps every triplet away from S = 0")


@pytest.mark.parametrize("d,p", SHARD_SHAPES)
@pytest.mark.parametrize("ns", SHARD_COUNTS)
def test_many_mixed_shards_against_oracle(tw, tile, ns, d, p):
    """One shard of tile + 3 triplets makes every shard own two partial slots, and all the others
    write at most the first: the work buffer's sentinel reads as a NaN, so a slot read without
    having been written shows in G or in that shard's loss."""
    worst_G = worst_loss = 0.0
    for big, empty in placements(ns):
        X, Z, Lm, i, j, k, off, (_, G_o, act_o, low) = mixed_case(ns, d, p, tile, big,
                                                                 tuple(empty))
        sizes = np.diff(off)
        assert low > 1e-6 and (sizes == 0).any() and sizes.max() == sizes[big] == tile + 3
        G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, off, 1.0)
        assert np.array_equal(act, act_o), (ns, big)
        dG = np.abs(G - G_o).max()
        worst_G = max(worst_G, dG)
        assert close(G, G_o), (ns, big, dG)
        for s in range(ns):
            a, b = off[s], off[s + 1]
            if a == b:
                assert bits(loss)[s] == 0 and act[s] == 0, (ns, big, s)  # an empty shard: +0.0
                continue
            want = o_shard(X, Z, Lm, i[a:b], j[a:b], k[a:b], 1.0)[0]  # the shard alone
            worst_loss = max(worst_loss, abs(loss[s] - want))
            assert abs(loss[s] - want) <= TOL * max(1.0, abs(want)), (ns, big, s)
        G0, loss0, act0 = raw_grad(tw, X, Z, Lm, i, j, k, off, 1.0, want_grad=0)
        assert np.all(G0 == -7.0) and np.array_equal(act0, act_o)
        assert np.array_equal(bits(loss0), bits(loss)), (ns, big)
    print(f"shards={ns} d={d} p={p}: worst max|G - G_o| = {worst_G:.3g}, worst shard "
          f"|loss - loss_o| = {worst_loss:.3g} (bound {TOL:g} max(1, |want|))")


@pytest.mark.parametrize("d,p", SHARD_SHAPES)
@pytest.mark.parametrize("ns", SHARD_COUNTS)
def test_many_shards_exact_on_integers(tw, tile, ns, d, p):
    """Shard sizes that are powers of two, and a power of two of non-empty shards: every quotient
    is exact (a dyadic rational of few bits), so G and every loss are the same in any order."""
    assert tile == 128  # 256 triplets: two slices, the others one
    rng = np.random.RandomState(50 * ns + d)
    Xi, Zi, Li = int_data(d, p, 900 + ns + d)
    full = 1 << ((ns - 1).bit_length() - 1)  # the largest power of two below ns
    sizes = np.zeros(ns, dtype=np.int64)
    where = rng.permutation(ns)[:full]
    sizes[where] = rng.choice([1, 2, 64, 256], size=full, p=[0.45, 0.4, 0.1, 0.05])
    sizes[where[0]], sizes[where[1]] = 256, 64
    if ns > 16:  # shard 16, the first one a thread group takes second, is not empty
        sizes[16], sizes[where[2]] = sizes[where[2]], sizes[16]
    nz = int((sizes > 0).sum())
    assert nz & (nz - 1) == 0 and nz < ns and set(sizes) <= {0, 1, 2, 64, 256}
    off = np.concatenate([[0], np.cumsum(sizes)])
    i, j, k = draw(rng, N_ROWS, M_ROWS, int(off[-1]))
    S0, a, b, u, v = int_hinge(Xi, Zi, Li, i, j, k)
    margin = -int(np.sort(S0)[(len(S0) - 1) // 2])
    S = S0 + margin
    assert (S == 0).any() and (S > 0).any() and (S < 0).any()
    # G = sum_s (sum_t G_t) / size_s / nz = sum_t (256 / size_s) G_t / (256 nz), in int64
    weight = np.repeat(256 // np.maximum(sizes, 1), sizes) * (S > 0)
    Gn = 2 * ((u * weight[:, None]).T @ a - (v * weight[:, None]).T @ b)
    assert np.abs(Gn).max() < 1 << 52
    G_r = quotients(Gn, 256 * nz)
    assert all(Fraction(float(x)) == Fraction(int(n_), 256 * nz)
               for x, n_ in zip(G_r.reshape(-1), Gn.reshape(-1)))  # exact, not merely rounded
    loss_r = np.zeros(ns)
    act_r = np.zeros(ns, dtype=np.uint64)
    for s in range(ns):
        Ss = S[off[s]:off[s + 1]]
        if len(Ss):
            loss_r[s] = quotients(Ss[Ss > 0].sum(), len(Ss))
            act_r[s] = (Ss > 0).sum()
    X, Z, Lm = as_f64(Xi, Zi, Li)
    G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, off, float(margin))
    wrong = int((bits(G) != bits(G_r)).sum())
    print(f"shards={ns} ({nz} non-empty) d={d} p={p} triplets={off[-1]}: entries of G off {wrong}, "
          f"max|G - G_r| = {np.abs(G - G_r).max():.3g}, shard losses off "
          f"{int((bits(loss) != bits(loss_r)).sum())}")
    assert np.array_equal(act, act_r)
    assert np.array_equal(bits(G), bits(G_r))
    assert np.array_equal(bits(loss), bits(loss_r))


# ------------------------------------------------ 4. chunked periods and the draw fallback
CUT_KEYS = ("iter", "train_loss", "test_loss", "train_stat", "test_stat", "test_stat_complete")


def cut_p_learn():
    """The small trajectory of test_trajectory with periods of 10 steps and an evaluation every
    4: with 3 steps per chunk a period is cut 3 + 3 + 3 + 1, the evaluations at 0, 16 and 20 fall
    on a chunk's first step, those at 4, 8, 12 and 24 inside one, and n_it = 27 ends inside a
    period and inside a chunk."""
    X, Z, tX, tZ, L0 = trajectory_data()
    return X, Z, {"n_it": 27, "N": 4, "B": 16, "margin": 1.0, "reg": 0.01, "learning_rate": 0.01,
                  "reshuffle_mod": 10, "eval_mod": 4, "L_init": L0, "n_monitor": 32,
                  "test_X": tX, "test_Z": tZ, "test_complete": True}


def run_cut(tl, optim):
    X, Z, pl = cut_p_learn()
    np.random.seed(70)
    Lg = tl.learning_process(X, Z, pl, optim)
    return Lg, pl, np.random.get_state()


def same_run(one, two):
    (La, pa, sa), (Lb, pb, sb) = one, two
    assert np.array_equal(bits(La), bits(Lb))
    assert pa["iter"] == pb["iter"] == list(range(0, 27, 4))
    for key in CUT_KEYS[1:]:
        assert len(pa[key]) == len(pb[key]) == 7, key
        assert np.array_equal(bits(pa[key]), bits(pb[key])), key
    for key in ("train_monitor", "test_monitor"):
        assert all(np.array_equal(a, b) for a, b in zip(pa[key], pb[key])), key
    assert same_state(sa, sb)


@pytest.mark.parametrize("optim", ["SGD", "momentum"])
def test_chunk_cuts_change_nothing(tl, monkeypatch, optim):
    whole = run_cut(tl, optim)
    X, Z, po = cut_p_learn()
    np.random.seed(70)
    Lo, low = o_learning_process(X, Z, po, optim)
    state_o = np.random.get_state()
    assert low > 1e-6  # over every training triplet of the oracle's run
    print(optim, "unchunked max|L - L_o| =", np.abs(whole[0] - Lo).max(), "oracle min|S| =", low)
    assert np.abs(whole[0] - Lo).max() <= 1e-10 and same_state(whole[2], state_o)
    assert whole[1]["iter"] == po["iter"]
    for key in ("train_loss", "test_loss"):
        assert np.abs(np.array(whole[1][key]) - np.array(po[key])).max() <= 1e-10, key

    periods = []  # the steps each call of _period_draws is asked for
    inner = tl._period_draws

    def recording(S, *rest):
        periods.append(S)
        return inner(S, *rest)

    monkeypatch.setattr(tl, "_period_draws", recording)
    for steps, want in ((3, [3, 3, 3, 1] * 2 + [3, 3, 1]), (1, [1] * 27)):
        monkeypatch.setattr(tl, "CHUNK_TRIPLETS", steps * 4 * 16)
        del periods[:]
        cut = run_cut(tl, optim)
        assert periods == want  # the cuts are where this test means them to be
        same_run(cut, whole)
    monkeypatch.setattr(tl, "CHUNK_TRIPLETS", 1 << 22)
    del periods[:]
    run_cut(tl, optim)
    assert periods == [10, 10, 7]


@pytest.mark.parametrize("optim", ["SGD", "momentum"])
def test_draws_without_the_native_session(tl, monkeypatch, optim):
    whole = run_cut(tl, optim)
    refused = []

    class NoSession:
        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def randint_flat(self, *args, **kwargs):
            refused.append(1)
            raise NotImplementedError("not the legacy MT19937")

    monkeypatch.setattr(tl, "Session", NoSession)
    fallback = run_cut(tl, optim)
    assert len(refused) == 3  # one per period: every draw came from np.random.randint
    same_run(fallback, whole)


# ------------------------------------------------------------ 5. NaN coordinates in the gradient
def test_nan_rows_are_inactive(tw, tile):
    d, p, T = 16, 9, 2 * tile + 3  # <16, 16>: four triplets side by side in a wave
    X, Z, Lm = make(N_ROWS, M_ROWS, d, p, 81)
    X, Z = X.copy(), Z.copy()
    bad_x, bad_z = [3, 17, 49], [0, 22]
    X[3, 0], X[17, 15], X[49, 7], Z[0, 5], Z[22, 15] = (np.nan,) * 5
    X[17, 2] = np.nan
    rng = np.random.RandomState(82)
    good_x = np.setdiff1d(np.arange(N_ROWS), bad_x)
    good_z = np.setdiff1d(np.arange(M_ROWS), bad_z)
    i, k = rng.choice(good_x, T), rng.choice(good_z, T)
    j = rng.choice(good_x, T)
    j = np.where(j == i, good_x[(np.searchsorted(good_x, j) + 1) % len(good_x)], j)
    # every 7th triplet touches a NaN row: as i, as j, as k in turn (and some in two places)
    hit = np.arange(0, T, 7)
    for n, t in enumerate(hit):
        if n % 3 == 0:
            i[t] = bad_x[(n // 3) % 3]
        elif n % 3 == 1:
            j[t] = bad_x[(n // 3) % 3]
        else:
            k[t] = bad_z[(n // 3) % 2]
    i[hit[-1]], k[hit[-1]] = bad_x[0], bad_z[1]
    assert not np.any(i == j)
    touched = np.isin(i, bad_x) | np.isin(j, bad_x) | np.isin(k, bad_z)
    assert np.array_equal(np.flatnonzero(touched), hit) and len(hit) < T // 6
    assert np.isin(i, bad_x).sum() >= 3 and np.isin(j, bad_x).sum() >= 3
    assert np.isin(k, bad_z).sum() >= 3
    with np.errstate(invalid="ignore"):
        S = o_hinge(X, Z, Lm, i, j, k, 1.0)[0]
        loss_o, G_o, act_o, _ = o_loss_grad(X, Z, Lm, i, j, k, 1.0)
    assert np.array_equal(np.isnan(S), touched) and np.abs(S[~touched]).min() > 1e-6
    assert act_o[0] == (S > 0).sum() and np.isfinite(G_o).all() and np.isfinite(loss_o)
    G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], 1.0)
    print("NaN rows: max|G - G_o| =", np.abs(G - G_o).max(), "|loss - loss_o| =",
          abs(loss[0] - loss_o), "active", act[0], "of", T, "with", len(hit), "NaN triplets")
    assert act[0] == act_o[0]
    assert np.isfinite(G).all() and np.isfinite(loss[0])
    assert close(G, G_o) and close(loss[0], loss_o)
    G0, loss0, act0 = raw_grad(tw, X, Z, Lm, i, j, k, [0, T], 1.0, want_grad=0)
    assert np.all(G0 == -7.0) and act0[0] == act_o[0] and bits(loss0)[0] == bits(loss)[0]
