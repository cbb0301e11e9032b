"""tw_pair_moments (csrc/moments.hip) and the API above it against the NumPy oracle pinned in
test_moments_cpu.py.  Bar: the integers are equal — there is no tolerance anywhere; the
derived floats are compared bit for bit where the specification says so (theta, UnN's value)."""
import numpy as np
import pytest

from test_moments_cpu import moments_sorted, point_counts

pytestmark = pytest.mark.gpu

ALGOS = ("pairs", "sorted", "auto")
SIZES = (0, 1, 2, 63, 64, 65, 255, 257, 1023, 1025, 4099)


def _device_moments(xs, zs, half, algo, code=None):
    from tuplewise import _engine as E
    from tuplewise import _lib as L
    if code is None:
        code = L.TW_I64 if np.asarray(xs[0]).dtype.kind == "i" else L.TW_F64
    sh = E.Shards.from_blocks(xs, zs, code)
    got = E.moments_complete(sh, "half" if half else "gt", algo)
    assert got.dtype == np.uint64 and got.shape == (len(xs), 4)
    return [tuple(int(v) for v in row) for row in got]


def _oracle(xs, zs, half):
    return [moments_sorted(x, z, half) for x, z in zip(xs, zs)]


def _check(xs, zs, half, algos=ALGOS):
    want = _oracle(xs, zs, half)
    for algo in algos:
        assert _device_moments(xs, zs, half, algo) == want, algo
    return want


@pytest.mark.parametrize("half", [False, True])
def test_mixed_launch(gpu, half):
    """One launch, block sizes differing inside it: every size of SIZES on each side, a block
    empty on each side, 1 x 4099 and 4099 x 1; heavy ties so that half mode matters."""
    rng = np.random.RandomState(5)
    shapes = [(SIZES[i], SIZES[(i * 4 + 3) % len(SIZES)]) for i in range(len(SIZES))]
    shapes += [(0, 257), (255, 0), (1, 4099), (4099, 1), (4099, 4099), (2, 2)]
    assert {a for a, _ in shapes} >= set(SIZES) and {b for _, b in shapes} >= set(SIZES)
    xs = [rng.normal(size=a).round(1) for a, _ in shapes]
    zs = [rng.normal(size=b).round(1) for _, b in shapes]
    want = _check(xs, zs, half)
    assert want[shapes.index((0, 257))] == (0, 0, 0, 0)
    # the A/B hook itself (process-global), with algo="auto" leaving the choice to it
    from tuplewise import _lib as L
    for k in (1, 2):
        L.call("tw_pair_moments_set_algo", k)
        try:
            assert _device_moments(xs, zs, half, "auto") == want, k
        finally:
            L.call("tw_pair_moments_set_algo", 0)


def _family(kind, rng, n, side):
    if kind == "gauss":
        return rng.normal(size=n)
    if kind == "ties":
        return rng.randint(0, 5, n).astype(np.float64)
    if kind == "equal":
        return np.full(n, -2.25)
    if kind == "edge":
        v = rng.normal(size=n).round(1)
        v[::7] = np.nan
        v[1::9] = 0.0
        v[2::11] = -0.0
        v[3::13] = np.inf
        v[4::17] = -np.inf
        return v
    if kind == "i64_2p53":  # a float compare would merge these
        s = np.where(rng.randint(0, 2, n) == 1, 1, -1).astype(np.int64)
        v = s * np.int64(2 ** 53) + rng.randint(0, 3, n).astype(np.int64)
        v[::29] = np.iinfo(np.int64).max  # its order key is the sort's padding key
        v[1::31] = np.iinfo(np.int64).min
        return v
    if kind == "bernoulli":  # estimation-experiment/main.py:97-101 at epsilon = 0.3
        b = rng.binomial(1, 0.7 if side == "x" else 0.3, n).astype(np.int64)
        return 2 * b if side == "x" else 2 * b - 1
    raise AssertionError(kind)


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("kind", ["gauss", "ties", "equal", "edge", "i64_2p53", "bernoulli"])
def test_input_families(gpu, kind, half):
    """Three blocks in one launch: below one sort chunk, a chunk with padding, two chunks."""
    rng = np.random.RandomState(11)
    shapes = [(300, 257), (1500, 1300), (5000, 4099)]
    xs = [_family(kind, rng, a, "x") for a, _ in shapes]
    zs = [_family(kind, rng, b, "z") for _, b in shapes]
    _check(xs, zs, half, ("pairs", "sorted"))


@pytest.mark.parametrize("half", [False, True])
def test_crossover(gpu, half):
    """Launches exactly at MOMENTS_SORTED_MIN_PAIRS and one element either side of it: auto
    and both forced algorithms give the oracle's integers."""
    from tuplewise import _engine as E
    P = E.MOMENTS_SORTED_MIN_PAIRS
    n0 = 1 << ((P.bit_length() - 1 + 1) // 2)
    m0 = P // n0
    assert n0 * m0 == P and m0 > 1
    rng = np.random.RandomState(2)
    for n, m in ((n0, m0), (n0, m0 - 1), (n0 + 1, m0)):  # at, just below, just above
        x, z = rng.normal(size=n).round(2), rng.normal(size=m).round(2)
        _check([x], [z], half)


@pytest.mark.parametrize("half", [False, True])
def test_large_single_block(gpu, half):
    """70 000 x 90 001: a_i^2 exceeds 2^32 (a 32-bit accumulator would wrap), several staging
    groups of sorted chunks per search.  S equals the existing count."""
    from tuplewise import _engine as E
    from tuplewise import _lib as L
    rng = np.random.RandomState(7)
    x, z = rng.normal(size=70_000), rng.normal(size=90_001)
    z[rng.randint(0, z.size, 900)] = x[rng.randint(0, x.size, 900)]  # 1 % ties
    want = _check([x], [z], half, ("sorted", "pairs"))[0]
    assert int(point_counts(x, z, half)[0].max()) ** 2 > 2 ** 32 and want[1] > 2 ** 32
    count = E.count_complete(E.Shards.from_blocks([x], [z], L.TW_F64), "half" if half else "gt")
    assert int(count[0]) == want[0]


@pytest.mark.parametrize("tie_mode", ["strict", "half"])
@pytest.mark.parametrize("dx,dz", [(np.float64, np.float64), (np.float32, np.float32),
                                   (np.int32, np.int32), (np.int32, np.float32)])
def test_un_var_theta_bits(gpu, tie_mode, dx, dz):
    import tuplewise.estimation as est
    rng = np.random.RandomState(4)
    X = rng.randint(-20, 20, 777).astype(dx)
    Z = rng.randint(-20, 20, 555).astype(dz)
    c = est.Un_var(X, Z, tie_mode=tie_mode)
    want = est.Un(X, Z, tie_mode=tie_mode)
    assert np.float64(c.theta).tobytes() == np.float64(want).tobytes()
    half = tie_mode == "half"
    assert (c.S, c.A2, c.B2, c.Q) == moments_sorted(X.astype(np.float64),
                                                    Z.astype(np.float64), half)
    assert (c.n, c.m, c.unit) == (777, 555, 2 if half else 1)


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("tie_mode", ["strict", "half"])
@pytest.mark.parametrize("sampling", ["prop-SWOR", "SWOR"])
def test_unn_var_matches_unn(gpu, sampling, tie_mode):
    """Value, post-call arrays and np.random state are est.UnN's; blocks are the oracle's
    moments of the shuffled slices.  n = 1000, m = 12, N = 10 makes SWOR draw degenerate
    blocks (k = tau with probability ~0.3 per block)."""
    import tuplewise.estimation as est
    from tuplewise import _blocks as Bk
    rng = np.random.RandomState(9)
    X0, Z0 = rng.normal(size=1000).round(1), rng.normal(0.3, 1, size=12).round(1)
    half = tie_mode == "half"
    X, Z = X0.copy(), Z0.copy()
    np.random.seed(21)
    want = est.UnN(X, Z, 10, sampling, tie_mode=tie_mode)
    state = np.random.get_state()
    Xv, Zv = X0.copy(), Z0.copy()
    np.random.seed(21)
    value, var, blocks = est.UnN_var(Xv, Zv, 10, sampling, tie_mode=tie_mode)
    assert np.float64(value).tobytes() == np.float64(want).tobytes()
    assert np.array_equal(Xv, X) and np.array_equal(Zv, Z)
    assert _same_state(np.random.get_state(), state)
    # the plan again, on scratch copies from the same seed: the slices the blocks were cut at
    np.random.seed(21)
    plan = Bk.plan_un(X0.copy(), Z0.copy(), 10, Bk.BlockSpec(), sampling, "est")
    cut = [p[1] for p in plan if p[0] == "val"]
    if sampling == "SWOR":
        assert len(cut) < len(plan) == 10, "this seed must draw a degenerate block"
    assert len(blocks) == len(cut)
    for c, b in zip(blocks, cut):
        xs, zs = X[b.x[0]:b.x[1]], Z[b.z[0]:b.z[1]]
        assert (c.n, c.m, c.unit) == (len(xs), len(zs), 2 if half else 1)
        assert (c.S, c.A2, c.B2, c.Q) == moments_sorted(xs, zs, half)
    total = sum(c.var_Un for c in blocks) / len(plan) ** 2
    assert var == total or (np.isnan(var) and np.isnan(total))
    with pytest.raises(NotImplementedError):
        est.UnN_var(X0.copy(), Z0.copy(), 10, "prop-SWR", tie_mode=tie_mode)


@pytest.mark.parametrize("tie_mode", ["strict", "half"])
@pytest.mark.parametrize("n,m,N", [(5000, 50, 10), (4096, 4096, 4)])
def test_sharded_sample(gpu, n, m, N, tie_mode):
    import torch
    import tuplewise.estimation as est
    from tuplewise.device import ShardedSample
    rng = np.random.RandomState(n + N)
    X, Z = rng.normal(size=n).round(2), rng.normal(0.2, 1, size=m).round(2)
    half = tie_mode == "half"
    S = ShardedSample(torch.from_numpy(X).cuda(), torch.from_numpy(Z).cuda(), N,
                      tie_mode=tie_mode)
    S.repartition(12345)
    mom = S.local_moments()
    assert mom.dtype == torch.int64 and tuple(mom.shape) == (N, 4) and mom.is_cuda
    got = mom.cpu().numpy().view(np.uint64)
    Xs, Zs = S.X.cpu().numpy(), S.Z.cpu().numpy()
    for s in range(N):
        xs, zs = Xs[S.x_off[s]:S.x_off[s + 1]], Zs[S.z_off[s]:S.z_off[s + 1]]
        assert tuple(int(v) for v in got[s]) == moments_sorted(xs, zs, half), s
    counts = S.local_counts().cpu().numpy().view(np.uint64)
    assert np.array_equal(counts, got[:, 0])
    assert S.Un_var() == est.Un_var(Xs, Zs, tie_mode=tie_mode)


def test_evaluate_device_equals_evaluate(gpu):
    import torch
    from tuplewise import _blocks as Bk
    rng = np.random.RandomState(6)
    X, Z = rng.randint(0, 50, 900).astype(np.int64), rng.randint(0, 50, 700).astype(np.int64)
    blocks = [Bk.Block((0, 400), (0, 300)), Bk.Block((400, 900), (300, 700))]
    spec = Bk.PairMoments("half")
    want = spec.evaluate(X, Z, blocks)
    got = spec.evaluate_device(torch.from_numpy(X).cuda(), torch.from_numpy(Z).cuda(), blocks)
    assert got == want
    assert [(c.S, c.A2, c.B2, c.Q) for c in want] == [
        moments_sorted(X[:400], Z[:300], True), moments_sorted(X[400:], Z[300:], True)]


def test_var_unnt_against_closed_form(gpu):
    """Un_var(...).var_UnNT(10, 4) averaged over 20 Bernoulli samples (RandomState(0),
    n = 5000, m = 50, epsilon = 0.3) within 10 % of Var_Un + 9 sigma_0 / (n m 4).  The NumPy
    oracle alone gives 3.751e-4 against 3.824e-4 here: -1.9 % (seeds 1..3: -3.8, +3.6, +3.0 %)."""
    import tuplewise.estimation as est
    n, m, eps = 5000, 50, 0.3
    rs = np.random.RandomState(0)
    vals = []
    for _ in range(20):
        X = 2 * rs.binomial(1, 1 - eps, n)
        Z = 2 * rs.binomial(1, eps, m) - 1
        vals.append(est.Un_var(X, Z).var_UnNT(10, 4))
    want = est.Var_Un(eps, n, m) + 9 * est.sigma_0(eps) / (n * m * 4)
    print(f"var_UnNT(10, 4): mean {np.mean(vals)!r}, closed form {want!r}")
    assert abs(np.mean(vals) - want) < 0.10 * want
