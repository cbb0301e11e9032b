"""The float pair sums (k_pair_sum, k_pair_sum_idx) and the fused evaluation (k_eval_pairs) of
csrc/pairsum.hip against math.fsum over the float64 terms, formed exactly as the kernels form
them: x*z, abs(x - z), max((z - x) + margin, 0), logaddexp(0, (z - x) + margin).

Tolerance, from the kernels' constants — never relative to the result (the prod sums cancel):

    |sum - fsum(terms)| <= chain * 2^-53 * sum |terms|

chain = the longest accumulation path a term can take:
  all pairs: min(nz, 2048) (the z chunk a lane walks) + 4 (its R accumulators) + 8 (wave and
             block trees) + ceil(per / 64) (k_reduce_partials' lane loop) + 6 (its tree), per =
             tw_pair_sum_work_per_shard of the launch;
  indexed:   the same with 8 (kSumPPT pairs per lane) in place of the chunk.
The logistic kernel adds 4 * 2^-52 * sum |terms|: the 4 ulp test_device_sigmoid_accuracy
grants the device exp.  Inputs are unit-scale Gaussians, and every case checks on the host that
the median |term| is at least 100 times its tolerance, so one dropped or doubled term fails —
the median over the non-zero terms: the hinge is 0 on more than half of the pairs at margins
<= 0, and a dropped zero changes no sum."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KERNELS = ["prod", "gini", "hinge", "logistic"]
SIZES = [(1, 1), (1024, 2048), (1025, 2049), (1, 4097), (2048, 1), (0, 10), (10, 0),
         (3000, 100)]
PAIR_COUNTS = [1, 2047, 2048, 2049, 6000, 0]


def _code(kern):
    from tuplewise import _lib as L
    return {"prod": L.TW_KERN_PROD, "gini": L.TW_KERN_GINI, "hinge": L.TW_KERN_HINGE,
            "logistic": L.TW_KERN_LOGISTIC}[kern]


def _terms(kern, x, z, margin):
    """The float64 terms as the kernels form them (x, z broadcast)."""
    with np.errstate(invalid="ignore", over="ignore"):
        if kern == "prod":
            return x * z
        if kern == "gini":
            return np.abs(x - z)
        if kern == "hinge":
            return np.maximum((z - x) + margin, 0)
        return np.logaddexp(0, (z - x) + margin)


def _chain(first, per):
    return first + 4 + 8 + -(-per // 64) + 6


def _frac(err, tol):
    """err as a fraction of its tolerance (a shard of zero terms has tolerance 0)."""
    return err / tol if tol > 0 else (0.0 if err == 0 else np.inf)


def _bar(kern, terms, chain):
    """(tolerance, fsum) of one sum; checks that a single term stands out of the tolerance."""
    a = np.abs(terms.ravel())
    s = float(a.sum())
    tol = chain * 2.0 ** -53 * s + (4 * 2.0 ** -52 * s if kern == "logistic" else 0.0)
    nz = a[a > 0]
    if nz.size:
        assert np.median(nz) >= 100 * tol, (kern, np.median(nz), tol)
    return tol, math.fsum(terms.ravel().tolist())


@pytest.fixture(scope="module")
def shards():
    rng = np.random.RandomState(20)
    xs = [rng.normal(0.1, 1, nx) for nx, _ in SIZES]
    zs = [rng.normal(0, 1, nz) for _, nz in SIZES]
    return xs, zs


@pytest.fixture(scope="module")
def shards_dev(gpu, shards):
    from tuplewise import _engine as E, _lib as L
    return E.Shards.from_blocks(shards[0], shards[1], L.TW_F64)


@pytest.mark.parametrize("margin", [1.0, 0.0, -0.5])
@pytest.mark.parametrize("kern", KERNELS)
def test_all_pairs_sum_within_chain_bound(gpu, shards, shards_dev, kern, margin):
    """k_pair_sum over one launch of ragged shards — one pair, exactly one x tile and one z
    chunk, one more than each, three z chunks under one x, two x tiles over one z, both empty
    kinds, three x tiles: every kernel at margins 1, 0 and -0.5 within the chain bound of the
    fsum reference; empty shards exactly 0.0."""
    from tuplewise import _engine as E, _lib as L
    xs, zs = shards
    got = E.pair_sum_complete_dev(shards_dev, _code(kern), margin, "pairs").cpu().numpy()
    per = int(L.lib().tw_pair_sum_work_per_shard(max(nx for nx, _ in SIZES),
                                                 max(nz for _, nz in SIZES)))
    assert per == 9
    worst = 0.0
    for s, (x, z) in enumerate(zip(xs, zs)):
        if len(x) == 0 or len(z) == 0:
            assert got[s] == 0.0 and not np.signbit(got[s])
            continue
        tol, want = _bar(kern, _terms(kern, x[:, None], z[None, :], margin),
                         _chain(min(len(z), 2048), per))
        worst = max(worst, _frac(abs(got[s] - want), tol))
        assert abs(got[s] - want) <= tol, (SIZES[s], got[s], want, tol)
    print(f"all pairs {kern} margin {margin}: max error = {worst:.3g} of the bar")


def _nonfinite_cases():
    inf, nan = np.inf, np.nan
    base_x, base_z = np.array([0.5, -1.0, 2.0]), np.array([1.0, 0.25, -3.0, 4.0])
    # the case list of test_hinge_sorted_nonfinite (tests/test_gpu_parity.py)
    cases = [([], []), ([nan], []), ([], [nan]), ([], [inf]), ([-inf], []), ([inf], []),
             ([], [-inf]), ([inf], [inf]), ([-inf], [-inf]), ([inf], [-inf]), ([-inf], [inf])]
    xs = [np.concatenate([base_x, np.array(a, dtype=np.float64)]) for a, _ in cases]
    zs = [np.concatenate([base_z, np.array(b, dtype=np.float64)]) for _, b in cases]
    xs.append(np.array([inf, inf]))
    zs.append(np.array([1.0, 2.0]))
    # the padded-lane mask: one valid x beside 1023 lanes holding 0.0 (0 * inf = NaN must not
    # leak into the prod sum), and 1025 x — the second tile has one valid lane — against
    # z = -inf and NaN.  Quarter-integer values: every finite sum is exact in any order.
    mixed = (np.arange(1025) % 17) * 0.25 - 2.0
    pos = (np.arange(1025) % 17 + 1) * 0.25
    for x, extra in (([0.5], [inf]), ([-0.5], [inf]), (mixed, [-inf]), (pos, [-inf]),
                     (mixed, [nan]), (pos, [-inf, nan])):
        xs.append(np.asarray(x, dtype=np.float64))
        zs.append(np.concatenate([base_z, np.array(extra)]))
    return xs, zs


@pytest.mark.parametrize("kern", KERNELS)
def test_all_pairs_nonfinite(gpu, kern):
    """NaN / +-inf operands, every kernel, against NumPy's elementwise terms then summed:
    array-equal, NaN-aware.  The finite shards hold quarter-integers, so prod, gini and hinge
    sums are exact in any order and must match to the bit; a finite logistic sum (irrational
    terms through the device exp, which is granted 4 ulp) is held to the chain bound
    instead, its finiteness still to the bit."""
    from tuplewise import _engine as E, _lib as L
    xs, zs = _nonfinite_cases()
    sh = E.Shards.from_blocks(xs, zs, L.TW_F64)
    per = int(L.lib().tw_pair_sum_work_per_shard(1025, 6))
    for margin in (1.0, 0.0):
        got = E.pair_sum_complete_dev(sh, _code(kern), margin, "pairs").cpu().numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            terms = [_terms(kern, x[:, None], z[None, :], margin) for x, z in zip(xs, zs)]
            want = np.array([t.sum() for t in terms])
        if kern != "logistic":
            np.testing.assert_array_equal(got, want)
            continue
        fin = np.isfinite(want)
        np.testing.assert_array_equal(got[~fin], want[~fin])
        assert np.all(np.isfinite(got[fin]))
        exact = int(np.sum(got[fin] == want[fin]))
        print(f"logistic margin {margin}: {exact} of {int(fin.sum())} finite sums equal "
              f"NumPy's to the bit")
        for s in np.nonzero(fin)[0]:
            a = float(np.abs(terms[s]).sum())
            tol = _chain(min(len(zs[s]), 2048), per) * 2.0 ** -53 * a + 4 * 2.0 ** -52 * a
            assert abs(got[s] - math.fsum(terms[s].ravel().tolist())) <= tol, s


@pytest.mark.parametrize("margin", [1.0, -0.5])
@pytest.mark.parametrize("kern", KERNELS)
def test_indexed_sum_and_fused_count(gpu, kern, margin):
    """k_pair_sum_idx with int64 indices, int32 indices and int32 + the fused #{x > z}: pair
    counts per shard of 1, one block's 2048 less one / exactly / plus one, 6000 (three
    blocks) and 0.  The sum within the chain bound, the three variants' sums the same bits,
    the count NumPy's exactly."""
    import torch
    from tuplewise import _engine as E, _lib as L
    rng = np.random.RandomState(21)
    x, z = rng.normal(0.1, 1, 500), rng.normal(0, 1, 300)
    off = np.concatenate([[0], np.cumsum(PAIR_COUNTS)]).astype(np.int64)
    ix, iz = rng.randint(0, 500, off[-1]), rng.randint(0, 300, off[-1])
    xd, zd = L.to_device(x), L.to_device(z)
    code = _code(kern)
    i64 = (L.to_device(ix, np.int64), L.to_device(iz, np.int64))
    i32 = (L.to_device(ix, np.int32), L.to_device(iz, np.int32))
    cnt = L.empty((len(PAIR_COUNTS),), torch.int64)
    s64 = E.pair_sum_indexed_dev(xd, zd, i64[0], i64[1], off, code, margin).cpu().numpy()
    s32 = E.pair_sum_indexed_dev(xd, zd, i32[0], i32[1], off, code, margin).cpu().numpy()
    s32c = E.pair_sum_indexed_dev(xd, zd, i32[0], i32[1], off, code, margin,
                                  count_out=cnt).cpu().numpy()
    assert np.array_equal(s64, s32) and np.array_equal(s64, s32c)
    per = int(L.lib().tw_pair_sum_idx_work_per_shard(max(PAIR_COUNTS)))
    assert per == 3
    worst = 0.0
    counts = cnt.cpu().numpy()
    for s, n in enumerate(PAIR_COUNTS):
        a, b = x[ix[off[s]:off[s + 1]]], z[iz[off[s]:off[s + 1]]]
        assert counts[s] == int(np.sum(a > b))
        if n == 0:
            assert s64[s] == 0.0
            continue
        tol, want = _bar(kern, _terms(kern, a, b, margin), _chain(8, per))
        worst = max(worst, _frac(abs(s64[s] - want), tol))
        assert abs(s64[s] - want) <= tol, (n, s64[s], want, tol)
    print(f"indexed {kern} margin {margin}: max error = {worst:.3g} of the bar")


def test_indexed_count_nan_pairs(gpu):
    """The fused count over pairs that hold NaN and +-inf scores: NumPy's #{x > z} exactly
    (a NaN compares false), the sums NaN exactly where NumPy's are, the three index variants
    the same bits."""
    import torch
    from tuplewise import _engine as E, _lib as L
    rng = np.random.RandomState(22)
    x, z = rng.normal(0.1, 1, 64), rng.normal(0, 1, 48)
    x[[3, 40]] = [np.nan, np.inf]
    z[[5, 17, 30]] = [np.nan, -np.inf, np.inf]
    counts = [2049, 300, 0, 4100]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ix, iz = rng.randint(0, 64, off[-1]), rng.randint(0, 48, off[-1])
    xd, zd = L.to_device(x), L.to_device(z)
    i64 = (L.to_device(ix, np.int64), L.to_device(iz, np.int64))
    i32 = (L.to_device(ix, np.int32), L.to_device(iz, np.int32))
    for kern in KERNELS:
        cnt = L.empty((len(counts),), torch.int64)
        s64 = E.pair_sum_indexed_dev(xd, zd, i64[0], i64[1], off, _code(kern), 1.0)
        s32 = E.pair_sum_indexed_dev(xd, zd, i32[0], i32[1], off, _code(kern), 1.0)
        s32c = E.pair_sum_indexed_dev(xd, zd, i32[0], i32[1], off, _code(kern), 1.0,
                                      count_out=cnt)
        s64, s32, s32c = (v.cpu().numpy() for v in (s64, s32, s32c))
        np.testing.assert_array_equal(s64, s32)
        np.testing.assert_array_equal(s64, s32c)
        got = cnt.cpu().numpy()
        for s in range(len(counts)):
            a, b = x[ix[off[s]:off[s + 1]]], z[iz[off[s]:off[s + 1]]]
            with np.errstate(invalid="ignore"):
                assert got[s] == int(np.sum(a > b)), (kern, s)
                want = _terms(kern, a, b, 1.0).sum() if len(a) else 0.0
            assert np.isnan(s64[s]) == np.isnan(want), (kern, s, s64[s], want)
            if not np.isfinite(want):
                np.testing.assert_array_equal(s64[s], want)


# --------------------------------------------------------------------- the fused evaluation
# (d, (test X rows, test Z rows), monitor pairs, loss); (1, 1) with 1 pair is the 2-block grid
EVAL_CASES = [
    (1, (1, 1), 1, "hinge"),
    (10, (1, 1), 1, "logistic"),
    (32, (1, 1), 6000, "hinge"),
    (10, (1, 1), 2049, "logistic"),
    (10, (1024, 2048), 2047, "hinge"),
    (32, (1024, 2048), 2049, "logistic"),
    (10, (1025, 2049), 2049, "hinge"),
    (1, (1025, 2049), 6000, "logistic"),
    (32, (1025, 2049), 1, "hinge"),
    (10, (3000, 100), 1, "logistic"),
    (32, (3000, 100), 2047, "hinge"),
    (1, (3000, 100), 6000, "hinge"),
]


def _eval_problem(d, n, m, n_pairs, seed):
    rng = np.random.RandomState(seed)
    w = rng.normal(0, 1, d) / np.sqrt(d)
    p = {"train_X": rng.normal(0.1, 1, (200, d)), "train_Z": rng.normal(0, 1, (150, d)),
         "test_X": rng.normal(0.1, 1, (n, d)), "test_Z": rng.normal(0, 1, (m, d)),
         "train_mon_pairs": list(zip(rng.randint(0, 200, n_pairs).tolist(),
                                     rng.randint(0, 150, n_pairs).tolist()))}
    return w, p


def _eval_both(lr, monkeypatch, wd, p, loss, margin):
    """_eval_device's four outputs: fused (twice in a row) and separate launches."""
    out = []
    for fused in (True, True, False):
        monkeypatch.setattr(lr, "EVAL_FUSED", fused)
        lr._eval_small.last = None
        res, n_pairs, n_test = lr._eval_device(wd, p, loss, margin, True)
        # the fused path ran exactly when asked for (no quiet fall-back to the launches)
        assert (res.data_ptr() == lr._eval_small.last) == fused
        out.append(res.cpu().numpy().copy())
    return out, n_pairs, n_test


@pytest.mark.parametrize("d,sizes,n_pairs,loss", EVAL_CASES)
def test_fused_evaluation_sizes(gpu, d, sizes, n_pairs, loss, monkeypatch):
    """tw_eval_small around one block of monitor pairs (2048), one x tile (1024) and one z
    chunk (2048) of the test sets, down to the 2-block grid: the four outputs bit-identical to
    the separate launches and across two fused calls in a row (the ticket resets itself); both
    surrogate sums within the chain bound of fsum over the device's own scores; both counts
    NumPy's on those scores."""
    import tuplewise.learning as lr
    from tuplewise import _lib as L
    n, m = sizes
    margin = 1.0
    w, p = _eval_problem(d, n, m, n_pairs, 100 * d + n_pairs % 97)
    wd = L.to_device(w)
    (f1, f2, sep), got_pairs, got_test = _eval_both(lr, monkeypatch, wd, p, loss, margin)
    assert (got_pairs, got_test) == (n_pairs, n * m)
    assert np.array_equal(f1.view(np.uint64), sep.view(np.uint64))
    assert np.array_equal(f1.view(np.uint64), f2.view(np.uint64))
    sx, sz, tx, tz = (lr._scores(lr._dev_f64(p[k]), wd).cpu().numpy()
                      for k in ("train_X", "train_Z", "test_X", "test_Z"))
    mon = np.asarray(p["train_mon_pairs"], dtype=np.int64)
    a, b = sx[mon[:, 0]], sz[mon[:, 1]]
    per_idx = int(L.lib().tw_pair_sum_idx_work_per_shard(n_pairs))
    per = int(L.lib().tw_pair_sum_work_per_shard(n, m))
    tol_m, want_m = _bar(loss, _terms(loss, a, b, margin), _chain(8, per_idx))
    tol_t, want_t = _bar(loss, _terms(loss, tx[:, None], tz[None, :], margin),
                         _chain(min(m, 2048), per))
    print(f"fused evaluation d={d} {sizes} {n_pairs} pairs {loss}: errors = "
          f"{_frac(abs(f1[0] - want_m), tol_m):.3g}, {_frac(abs(f1[2] - want_t), tol_t):.3g} "
          f"of the bar")
    assert abs(f1[0] - want_m) <= tol_m
    assert abs(f1[2] - want_t) <= tol_t
    assert int(f1[1:2].view(np.uint64)[0]) == int(np.sum(a > b))
    assert int(f1[3:4].view(np.uint64)[0]) == int(np.sum(tx[:, None] > tz[None, :]))


def test_fused_evaluation_refuses_wide_rows(gpu):
    """d = 33 is past tw_eval_small's row width: _eval_small returns None (the separate
    launches run)."""
    import tuplewise.learning as lr
    from tuplewise import _lib as L
    w, p = _eval_problem(33, 5, 4, 7, 1)
    assert lr._eval_small(L.to_device(w), p, L.TW_KERN_HINGE, 1.0) is None
    w, p = _eval_problem(32, 5, 4, 7, 1)
    assert lr._eval_small(L.to_device(w), p, L.TW_KERN_HINGE, 1.0) is not None


def test_fused_evaluation_padded_lanes_not_counted(gpu, monkeypatch):
    """Every test z below every test x and below 0, 1025 test x rows: the second x tile holds
    one valid lane beside 1023 padded ones whose 0.0 > z is true — the fused #{x > z} must be
    exactly 1025 * m, as the separate count."""
    import tuplewise.learning as lr
    from tuplewise import _lib as L
    rng = np.random.RandomState(4)
    n, m = 1025, 70
    p = {"train_X": rng.normal(0.1, 1, (20, 1)), "train_Z": rng.normal(0, 1, (20, 1)),
         "test_X": rng.uniform(0.5, 2.0, (n, 1)), "test_Z": rng.uniform(-3.0, -0.5, (m, 1)),
         "train_mon_pairs": [(1, 2), (3, 4), (0, 19)]}
    wd = L.to_device(np.ones(1))
    (f1, f2, sep), _, n_test = _eval_both(lr, monkeypatch, wd, p, "hinge", 1.0)
    assert n_test == n * m
    assert int(f1[3:4].view(np.uint64)[0]) == n * m
    assert np.array_equal(f1.view(np.uint64), sep.view(np.uint64))
    assert np.array_equal(f1.view(np.uint64), f2.view(np.uint64))
