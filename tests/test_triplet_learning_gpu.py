"""tuplewise.triplet_learning on the device against the NumPy oracle of
tests/test_triplet_learning_cpu.py: the projection bit for bit, the loss and the gradient within
the project's bound for unpinned gradients at d, p in {1, 3, 8, 17, 33, 64} — the
DP, PP in {8, 32, 64} forms of k_triplet_grad, 7 of the 16 pairs with the gradient and 4 without;
tests/test_triplet_learning_gpu_forms.py runs all 32 — and around the slice of triplets one
workgroup takes, the counts of active triplets exactly, the update bit for bit, and whole
trajectories with their evaluations, RNG consumption and untouched inputs."""
import functools

import numpy as np
import pytest

from test_triplets_cpu import same_state
from test_triplet_learning_cpu import (draw, make, o_learning_process, o_loss_grad, o_project,
                                       o_update)

pytestmark = pytest.mark.gpu

GUARD = 64  # sentinel entries behind each output and the work buffer: nothing may be written there
TOL = 1e-12  # the project's bound for gradients without a bit contract
N_ROWS, M_ROWS = 50, 40

PROJECT_SHAPES = [(1, 1), (3, 2), (8, 8), (17, 5), (37, 64), (64, 64), (5, 17)]
PROJECT_ROWS = [1, 63, 64, 65, 513]

# (d, p, triplets as a function of the slice): d and p each cover {1, 3, 8, 17, 33, 64} and the
# triplets {1, 63, 64, 65, slice - 1, slice, slice + 1, 2 slice + 3}
GRAD_CASES = {
    "d1-p1-t1": (1, 1, lambda s: 1),
    "d3-p64-t63": (3, 64, lambda s: 63),
    "d8-p8-t64": (8, 8, lambda s: 64),
    "d17-p3-t65": (17, 3, lambda s: 65),
    "d33-p17-tS-1": (33, 17, lambda s: s - 1),
    "d64-p64-tS": (64, 64, lambda s: s),
    "d64-p1-tS+1": (64, 1, lambda s: s + 1),
    "d1-p33-t2S+3": (1, 33, lambda s: 2 * s + 3),
    "d64-p8-t2S+3": (64, 8, lambda s: 2 * s + 3),
    "d8-p64-tS+1": (8, 64, lambda s: s + 1),
    "d33-p33-t65": (33, 33, lambda s: 65),
    "d17-p33-tS": (17, 33, lambda s: s),
}


@pytest.fixture(scope="module")
def tl(gpu):
    import tuplewise.triplet_learning as m
    return m


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_triplet_grad_tile())


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1).view(np.uint64)


@functools.lru_cache(maxsize=None)
def grad_case(name, S):
    """One case's data and reference (computed once, shared, never modified)."""
    d, p, ft = GRAD_CASES[name]
    T = ft(S)
    X, Z, Lm = make(N_ROWS, M_ROWS, d, p, 100 * d + p)
    i, j, k = draw(np.random.RandomState(T + d), N_ROWS, M_ROWS, T)
    return X, Z, Lm, i, j, k, o_loss_grad(X, Z, Lm, i, j, k, 1.0)


def close(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return np.abs(got - want).max() <= TOL * max(1.0, np.abs(want).max())


def raw_grad(tw, X, Z, Lm, i, j, k, off, margin, want_grad=1):
    """tw_triplet_grad called directly on sentinel-filled outputs with GUARD entries behind each:
    (G, loss, active), G with its sentinels when want_grad = 0."""
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns, (p, d) = len(off) - 1, Lm.shape
    max_t = int(np.diff(off).max())
    xd, zd, ld, od = (L.to_device(np.ascontiguousarray(a).reshape(-1)) for a in (X, Z, Lm, off))
    id_, jd, kd = (L.to_device(np.asarray(a, dtype=np.int32)) for a in (i, j, k))
    wn = int(L.lib().tw_triplet_grad_work_bytes(ns, max_t, d, p)) // 8
    dev = xd.device
    work = torch.full((wn + GUARD,), -7, dtype=torch.int64, device=dev)
    G = torch.full((p * d + GUARD,), -7.0, dtype=torch.float64, device=dev)
    loss = torch.full((ns + GUARD,), -7.0, dtype=torch.float64, device=dev)
    act = torch.full((ns + GUARD,), -7, dtype=torch.int64, device=dev)
    L.call("tw_triplet_grad", xd, zd, d, ld, p, id_, jd, kd, od, ns, max_t, float(margin),
           want_grad, work, G, loss, act, L.stream_handle())
    work, G, loss, act = work.cpu().numpy(), G.cpu().numpy(), loss.cpu().numpy(), act.cpu().numpy()
    assert np.all(work[wn:] == -7) and np.all(G[p * d:] == -7.0)
    assert np.all(loss[ns:] == -7.0) and np.all(act[ns:] == -7)
    return G[:p * d].reshape(p, d), loss[:ns], act[:ns].view(np.uint64)


# ------------------------------------------------------------------------------- projection
@pytest.mark.parametrize("d,p", PROJECT_SHAPES)
def test_project_bit_for_bit(tl, d, p):
    rng = np.random.RandomState(10 * d + p)
    Lm = rng.normal(size=(p, d))
    for rows in PROJECT_ROWS:
        A = rng.normal(size=(rows, d))
        got = tl.project(A, Lm)
        assert got.shape == (rows, p) and got.dtype == np.float64
        assert np.array_equal(bits(got), bits(o_project(A, Lm))), rows
    assert tl.project(np.zeros((0, d)), Lm).shape == (0, p)


def test_project_nan_and_inf_rows(tl):
    rng = np.random.RandomState(2)
    A, Lm = rng.normal(size=(65, 17)), rng.normal(size=(5, 17))
    A[3, 4], A[64, 16] = np.nan, np.nan
    A[10, 0], A[11, 7] = np.inf, -np.inf
    A[12, 2], A[12, 9] = np.inf, -np.inf  # inf - inf somewhere along the sum
    want = o_project(A, Lm)
    assert np.isnan(want[3]).all() and np.isinf(want[10]).all() and np.isnan(want[12]).any()
    assert np.array_equal(bits(tl.project(A, Lm)), bits(want))


# --------------------------------------------------------------------- loss and gradient
@pytest.mark.parametrize("name", list(GRAD_CASES))
def test_loss_grad_against_oracle(tl, tile, name):
    X, Z, Lm, i, j, k, (loss_o, G_o, act_o, low) = grad_case(name, tile)
    assert low > 1e-6  # no activity flip can excuse a difference
    loss, G, act = tl.loss_grad(X, Z, Lm, i, j, k, 1.0)
    print(name, "max|G - G_o| =", np.abs(G - G_o).max(), "max|G_o| =", np.abs(G_o).max(),
          "|loss - loss_o| =", abs(loss - loss_o), "loss_o =", loss_o)
    assert G.shape == Lm.shape and act.dtype == np.uint64 and isinstance(loss, np.float64)
    assert np.array_equal(act, act_o)
    assert close(G, G_o) and close(loss, loss_o)


def test_loss_grad_mixed_shards(tw, tl, tile):
    sizes = [1, 0, 65, tile + 3]
    off = np.concatenate([[0], np.cumsum(sizes)])
    X, Z, Lm = make(N_ROWS, M_ROWS, 17, 8, 12)
    i, j, k = draw(np.random.RandomState(13), N_ROWS, M_ROWS, int(off[-1]))
    loss_o, G_o, act_o, low = o_loss_grad(X, Z, Lm, i, j, k, 1.0, off)
    assert low > 1e-6
    loss, G, act = tl.loss_grad(X, Z, Lm, i, j, k, 1.0, trip_off=off)
    assert np.array_equal(act, act_o) and act[1] == 0
    assert close(G, G_o) and close(loss, loss_o)
    # raw: the same bits, the empty shard's loss 0, nothing written behind the buffers
    G_r, loss_r, act_r = raw_grad(tw, X, Z, Lm, i, j, k, off, 1.0)
    assert np.array_equal(bits(G_r), bits(G)) and np.array_equal(act_r, act_o)
    assert loss_r[1] == 0.0
    for s in (0, 2, 3):  # a shard's loss is the same alone as beside others
        a, b = off[s], off[s + 1]
        want = o_loss_grad(X, Z, Lm, i[a:b], j[a:b], k[a:b], 1.0)[0]
        assert abs(loss_r[s] - want) <= TOL * max(1.0, abs(want))
    # every shard empty (the index arrays are not read): a zero gradient
    G_e, loss_e, act_e = raw_grad(tw, X, Z, Lm, i[:1], j[:1], k[:1], [0, 0, 0], 1.0)
    assert not bits(G_e).any() and not loss_e.any() and not act_e.any()


@pytest.mark.parametrize("name", ["d17-p3-t65", "d64-p8-t2S+3", "d8-p64-tS+1"])
def test_margins_far_from_the_data(tw, tl, tile, name):
    X, Z, Lm, i, j, k, _ = grad_case(name, tile)
    loss, G, act = tl.loss_grad(X, Z, Lm, i, j, k, -1e9)
    assert not bits(G).any() and bits(loss)[0] == 0 and act[0] == 0  # all +0.0
    loss_o, G_o, act_o, _ = o_loss_grad(X, Z, Lm, i, j, k, 1e9)
    loss, G, act = tl.loss_grad(X, Z, Lm, i, j, k, 1e9)
    assert act[0] == len(i) == act_o[0]
    assert close(G, G_o) and close(loss, loss_o)


def test_repeated_anchor(tl, tile):
    X, Z, Lm = make(N_ROWS, M_ROWS, 8, 8, 21)
    T = tile + 1
    rng = np.random.RandomState(22)
    i = np.full(T, 7)
    j = rng.randint(0, N_ROWS - 1, T)
    j += j >= i
    k = rng.randint(0, M_ROWS, T)
    loss_o, G_o, act_o, low = o_loss_grad(X, Z, Lm, i, j, k, 1.0)
    assert low > 1e-6
    loss, G, act = tl.loss_grad(X, Z, Lm, i, j, k, 1.0)
    assert np.array_equal(act, act_o) and close(G, G_o) and close(loss, loss_o)


@pytest.mark.parametrize("name", ["d3-p64-t63", "d64-p64-tS", "d64-p8-t2S+3"])
def test_without_gradient_and_guards(tw, tile, name):
    X, Z, Lm, i, j, k, (loss_o, G_o, act_o, _) = grad_case(name, tile)
    G, loss, act = raw_grad(tw, X, Z, Lm, i, j, k, [0, len(i)], 1.0, want_grad=0)
    assert np.all(G == -7.0)  # the sentinels: d_G is left untouched
    assert act[0] == act_o[0] and close(loss[0], loss_o)
    G1, loss1, act1 = raw_grad(tw, X, Z, Lm, i, j, k, [0, len(i)], 1.0)
    assert close(G1, G_o) and act1[0] == act_o[0]
    assert bits(loss1)[0] == bits(loss)[0]  # the surrogate is the gradient call's loss


@pytest.mark.parametrize("name", ["d64-p64-tS", "d64-p8-t2S+3", "d1-p33-t2S+3"])
def test_deterministic(tl, tile, name):
    X, Z, Lm, i, j, k, _ = grad_case(name, tile)
    off = [0, len(i) // 3, len(i)]
    first = tl.loss_grad(X, Z, Lm, i, j, k, 1.0, trip_off=off)
    again = tl.loss_grad(X, Z, Lm, i, j, k, 1.0, trip_off=off)
    assert np.array_equal(bits(first[1]), bits(again[1]))
    assert bits(first[0])[0] == bits(again[0])[0] and np.array_equal(first[2], again[2])


# ---------------------------------------------------------------------------------- update
@pytest.mark.parametrize("optim", ["SGD", "momentum"])
def test_update_bit_for_bit(tw, optim):
    import torch
    L = tw._lib
    rng = np.random.RandomState(31)
    p, d, reg, lr = 5, 17, 0.05, 0.3
    Lm, grads = rng.normal(size=(p, d)), [rng.normal(size=(p, d)) for _ in range(2)]
    grads[1][0, 0], grads[1][1, 1] = 0.0, -0.0
    ld = L.to_device(Lm.reshape(-1))
    delta = torch.zeros(p * d + GUARD, dtype=torch.float64, device=ld.device)
    delta[p * d:] = -7.0
    Lo, do = Lm.copy(), 0
    for G in grads:  # two consecutive steps: the second one reads the first one's delta
        gd = L.to_device(G.reshape(-1))
        L.call("tw_triplet_sgd_update", gd, ld, delta, p * d, reg, lr, int(optim == "momentum"),
               L.stream_handle())
        Lo, do = o_update(Lo, do, G, reg, lr, optim)
        assert np.array_equal(bits(ld.cpu().numpy()), bits(Lo))
        assert np.array_equal(bits(delta.cpu().numpy()[:p * d]), bits(do))
    assert np.all(delta.cpu().numpy()[p * d:] == -7.0)


# ------------------------------------------------------------------------------ trajectory
def trajectory_data():
    rng = np.random.RandomState(41)
    n, m, d, p = 40, 36, 5, 3
    X, Z = rng.normal(size=(n, d)), rng.normal(0.5, 1.0, size=(m, d))
    tX, tZ = rng.normal(size=(30, d)), rng.normal(0.5, 1.0, size=(25, d))
    return X, Z, tX, tZ, rng.normal(size=(p, d)) / np.sqrt(d)


def trajectory_p_learn(tX, tZ, L0):
    return {"n_it": 80, "N": 4, "B": 16, "margin": 1.0, "reg": 0.01, "learning_rate": 0.01,
            "reshuffle_mod": 10, "eval_mod": 20, "L_init": L0, "n_monitor": 32, "test_X": tX,
            "test_Z": tZ, "test_complete": True}


@functools.lru_cache(maxsize=None)
def trajectory_oracle(optim):
    X, Z, tX, tZ, L0 = trajectory_data()
    po = trajectory_p_learn(tX, tZ, L0)
    np.random.seed(50)
    Lo, low = o_learning_process(X, Z, po, optim)
    return Lo, low, po, np.random.get_state()


@pytest.mark.parametrize("optim", ["SGD", "momentum"])
def test_trajectory(tl, monkeypatch, optim):
    import tuplewise.triplets as tr
    X, Z, tX, tZ, L0 = trajectory_data()
    keep = [a.copy() for a in (X, Z, tX, tZ, L0)]
    Lo, low, po, state_o = trajectory_oracle(optim)
    assert low > 1e-6  # over every training triplet of the oracle's run
    maps, inner = [], tl.evaluation_step

    def recording(it, Lmap, p_learn):
        maps.append(Lmap.copy())
        inner(it, Lmap, p_learn)

    monkeypatch.setattr(tl, "evaluation_step", recording)
    pl = trajectory_p_learn(tX, tZ, L0)
    np.random.seed(50)
    Lg = tl.learning_process(X, Z, pl, optim)
    assert same_state(np.random.get_state(), state_o)
    print(optim, "max|L - L_o| =", np.abs(Lg - Lo).max(), "oracle min|S| =", low)
    assert Lg.shape == L0.shape and np.abs(Lg - Lo).max() <= 1e-10
    for a, b in zip((X, Z, tX, tZ, L0), keep):
        assert np.array_equal(bits(a), bits(b))
    assert pl["iter"] == po["iter"] == [0, 20, 40, 60] and len(maps) == 4
    for key in ("train_loss", "test_loss"):
        assert len(pl[key]) == 4
        assert np.abs(np.array(pl[key]) - np.array(po[key])).max() <= 1e-10, key
    nt, mt = tX.shape[0], tZ.shape[0]
    for key, terms in (("train_stat", 32), ("test_stat", 32),
                       ("test_stat_complete", nt * (nt - 1) * mt)):
        assert len(pl[key]) == 4
        assert np.abs(np.array(pl[key]) - np.array(po[key])).max() <= 1.0 / terms + 1e-15, key
    assert len(set(po["train_stat"])) > 1  # the statistic moves along the run
    for e, Lm in enumerate(maps):  # exact counts on the module's own projection
        PX, PZ, PtX, PtZ = (tl.project(A, Lm) for A in (X, Z, tX, tZ))
        assert pl["train_stat"][e] == tr.UB_indices(PX, PZ, *pl["train_monitor"])
        assert pl["test_stat"][e] == tr.UB_indices(PtX, PtZ, *pl["test_monitor"])
        assert pl["test_stat_complete"][e] == tr.Un(PtX, PtZ, algo="sorted")


def test_trajectory_across_kernel_paths(tl):
    rng = np.random.RandomState(61)
    n, m, d, p = 100, 50, 64, 8
    X, Z = rng.normal(size=(n, d)), rng.normal(0.5, 1.0, size=(m, d))
    L0 = rng.normal(size=(p, d)) / np.sqrt(d)
    keep = [a.copy() for a in (X, Z, L0)]

    def p_learn():
        return {"n_it": 6, "N": 3, "B": 65, "margin": 1.0, "reg": 0.01, "learning_rate": 0.01,
                "reshuffle_mod": 2, "eval_mod": 100, "L_init": L0}

    for optim in ("SGD", "momentum"):
        po, pl = p_learn(), p_learn()
        np.random.seed(62)
        Lo, low = o_learning_process(X, Z, po, optim)
        state_o = np.random.get_state()
        assert low > 1e-6
        np.random.seed(62)
        Lg = tl.learning_process(X, Z, pl, optim)
        assert same_state(np.random.get_state(), state_o)
        print(optim, "max|L - L_o| =", np.abs(Lg - Lo).max(), "oracle min|S| =", low)
        assert np.abs(Lg - Lo).max() <= 1e-10
        assert pl["iter"] == po["iter"] == [0]  # (nothing to monitor: no other entry)
        assert not any(key.endswith(("_loss", "_stat", "_complete")) for key in pl)
    for a, b in zip((X, Z, L0), keep):
        assert np.array_equal(bits(a), bits(b))
