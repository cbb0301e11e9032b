"""The sorted path of tuplewise.onesample on the device (csrc/selfsorted.hip):
tw_self_sorted's Kendall integers equal the CPU sorted oracle of test_onesample_sorted_cpu.py and
tw_self_pairs on the device, on every input; the sorted Gini sum meets the package's float
pair-sum contract, is exact where the pair sum is an exact integer, and has the same bits
whatever shares its launch.  The raw entry point runs at chunk = 1024 so that chunk boundaries
are reached at sizes a test can afford, and once more at the default chunk."""
import numpy as np
import pytest

from test_gpu_onesample import edge_samples, raw_self_pairs, same_state
from test_onesample_cpu import o_Un, sample
from test_onesample_sorted_cpu import extreme_int64, s_kendall_counts

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-15
EPS = np.finfo(np.float64).eps
C = 1024
SIZES = [2, 3, C - 1, C, C + 1, 2 * C + 1, 3 * C + 5]


@pytest.fixture(scope="module")
def os1(gpu):
    import tuplewise.onesample as m
    return m


def raw_sorted(tw, flat, off, dtype, kern, chunk):
    """tw_self_sorted called directly on scratch full of junk: the per-shard outputs on the
    host.  The device copy of the input must come back unchanged."""
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns = len(off) - 1
    max_n, total = int(np.diff(off).max()), int(off[-1] - off[0])
    flat = np.ascontiguousarray(flat if flat.size else np.zeros(2, flat.dtype))
    sd, od = L.to_device(flat), L.to_device(off)
    need = L.lib().tw_self_sorted_work_bytes(ns, total, max_n, kern, chunk)
    assert need >= 8
    work = torch.full((need // 8,), 0x0123456789ABCDEF, dtype=torch.int64, device=sd.device)
    ken = kern == L.TW_SELF_KENDALL
    out = torch.full((ns, 5 if ken else 1), -7, dtype=torch.int64 if ken else torch.float64,
                     device=sd.device)
    L.call("tw_self_sorted", sd, od, ns, total, max_n, dtype, kern, chunk, work, out,
           L.stream_handle())
    host = out.cpu().numpy()
    assert np.array_equal(sd.cpu().numpy().view(np.uint64), flat.view(np.uint64))
    return host.view(np.uint64) if ken else host


def kendall_both(tw, S, chunks=(C, 0)):
    """The five counters of one (n, 2) sample from tw_self_sorted at every chunk, checked
    against tw_self_pairs on the device."""
    L = tw._lib
    dtype = L.TW_F64 if S.dtype == np.float64 else L.TW_I64
    n = S.shape[0]
    pairs = raw_self_pairs(tw, S.reshape(-1), [0, n], dtype, L.TW_SELF_KENDALL)[0]
    for chunk in chunks:
        got = raw_sorted(tw, S.reshape(-1), [0, n], dtype, L.TW_SELF_KENDALL, chunk)[0]
        assert np.array_equal(got, pairs), (chunk, got, pairs)
    return tuple(int(v) for v in pairs)


def kendall_sample(n, ties, dtype, seed):
    S = sample(n, "kendall", seed, ties)
    if dtype == "int64":  # Gaussian points on a grid of 1e-3 (a few ties), or the values 0..3
        S = np.ascontiguousarray(np.round(S * (1 if ties else 1000)).astype(np.int64))
    return S


# ------------------------------------------------------------------------------ Kendall
@pytest.mark.parametrize("dtype", ["float64", "int64"])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kendall_sizes(tw, gpu, n, ties, dtype):
    S = kendall_sample(n, ties, dtype, 3 * n + ties)
    assert kendall_both(tw, S) == s_kendall_counts(S)


@pytest.mark.parametrize("chunk", [2048, 8192, 16384])
def test_kendall_other_chunks(tw, gpu, chunk):
    """The sort networks of 8 and 16 keys a thread and the opted-in LDS of the largest chunk:
    one chunk and five items."""
    S = kendall_sample(chunk + 5, True, "float64", chunk)
    S[::7, 0] += 0.5
    assert kendall_both(tw, S, chunks=(chunk,)) == s_kendall_counts(S)


def test_mixed_shards_in_one_launch(tw, gpu):
    L = tw._lib
    sizes = [2, 2 * C + 3, 1, 0, C, 5]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    K = sample(int(off[-1]), "kendall", 99, ties=True)
    G = sample(int(off[-1]), "gini", 98)
    for S, kern in ((K, L.TW_SELF_KENDALL), (G, L.TW_SELF_GINI)):
        before = S.copy()
        got = raw_sorted(tw, S.reshape(-1), off, L.TW_F64, kern, C)
        other = raw_sorted(tw, S.reshape(-1), off, L.TW_F64, kern, 0)
        if kern == L.TW_SELF_KENDALL:
            assert np.array_equal(got, other)
        else:  # another chunk is another order of the double-double sum: each within an ulp
            assert np.allclose(got, other, rtol=2 * EPS, atol=0.0)
        for s, n in enumerate(sizes):
            part = S[off[s]:off[s + 1]]
            if n < 2:
                assert not got[s].any(), (s, got[s])  # zeros, and written
                continue
            alone = raw_sorted(tw, part.reshape(-1), [0, n], L.TW_F64, kern, C)
            assert got[s].tobytes() == alone[0].tobytes(), (s, got[s], alone[0])
            if kern == L.TW_SELF_KENDALL:
                assert tuple(int(v) for v in got[s]) == s_kendall_counts(part)
            else:
                pairs = np.float64(n * (n - 1) // 2)
                assert np.isclose(got[s][0] / pairs, o_Un(part, "gini"), rtol=RTOL, atol=ATOL)
        assert np.array_equal(S, before)
    # the same shards at offsets that do not start at 0
    shifted = raw_sorted(tw, K.reshape(-1), off[1:], L.TW_F64, L.TW_SELF_KENDALL, C)
    whole = raw_sorted(tw, K.reshape(-1), off, L.TW_F64, L.TW_SELF_KENDALL, C)
    assert np.array_equal(shifted, whole[1:])


def edge_cases():
    rng = np.random.RandomState(6)
    n = 2 * C + 1
    out = dict(edge_samples())
    out["extreme"] = extreme_int64(n, 2)  # INT64_MAX carries the key of chunk padding
    out["all equal"] = np.full((n, 2), 2.5)
    out["all equal int64"] = np.full((n, 2), np.iinfo(np.int64).max)
    out["constant a"] = np.ascontiguousarray(np.stack([np.ones(n), rng.permutation(n) * 1.0], 1))
    out["constant b"] = np.ascontiguousarray(np.stack([rng.normal(size=n), np.zeros(n)], 1))
    nan_a = sample(n, "kendall", 4, ties=True)
    nan_a[:, 0] = np.nan
    nan_b = sample(n, "kendall", 5)
    nan_b[:, 1] = np.nan
    out["nan a"], out["nan b"] = nan_a, nan_b
    some = sample(n, "kendall", 6, ties=True)  # one NaN here and there, in every chunk
    some[rng.randint(0, n, 40), 0] = np.nan
    some[rng.randint(0, n, 40), 1] = np.nan
    out["some nan"] = some
    zeros = sample(n, "kendall", 7, ties=True) - 1.0
    zeros[zeros == 0.0] *= rng.choice([1.0, -1.0], size=int((zeros == 0.0).sum()))
    out["signed zeros"] = zeros
    return out


@pytest.mark.parametrize("which", ["ties", "nonfinite", "int64", "extreme", "all equal",
                                   "all equal int64", "constant a", "constant b", "nan a",
                                   "nan b", "some nan", "signed zeros"])
def test_kendall_edge_data(tw, gpu, which):
    S = edge_cases()[which]
    n = S.shape[0]
    P = n * (n - 1) // 2
    got = kendall_both(tw, S)
    assert got == s_kendall_counts(S)
    if which.startswith("all equal"):
        assert got == (0, 0, P, P, P)
    if which == "constant a":
        assert got == (0, 0, P, 0, 0)
    if which == "nan a":
        assert got[:3] == (0, 0, 0) and got[4] == 0 and 0 < got[3] < P
    if which == "nan b":
        assert got == (0, 0, 0, 0, 0)
    if which == "signed zeros":
        assert np.signbit(S[S == 0.0]).any() and not np.signbit(S[S == 0.0]).all()


@pytest.mark.parametrize("mirror", [False, True])
def test_counters_above_2_to_32(tw, gpu, mirror):
    n = 100_000
    a = np.random.RandomState(1).permutation(n).astype(np.float64)
    S = np.ascontiguousarray(np.stack([a, a if mirror else -a], axis=1))
    L = tw._lib
    P = n * (n - 1) // 2
    assert P == 4_999_950_000 > 2 ** 32
    for chunk in (C, 0):
        got = raw_sorted(tw, S.reshape(-1), [0, n], L.TW_F64, L.TW_SELF_KENDALL, chunk)[0]
        assert tuple(int(v) for v in got) == ((P, 0, 0, 0, 0) if mirror else (0, P, 0, 0, 0))


def test_kendall_four_points_a_lane(tw, gpu):
    """From 192 tiles of 4096 points on, a lane of the search kernels holds four points: one
    such launch against tw_self_pairs."""
    n = 800_000
    S = sample(n, "kendall", 12)
    S[:, 1] = np.round(S[:, 1], 3)  # ties in b
    got = kendall_both(tw, S, chunks=(0,))
    assert got[0] + got[1] + got[2] + got[3] - got[4] == n * (n - 1) // 2 and got[3] > 0


def test_estimators_give_the_same_value_either_way(os1):
    S0 = sample(3001, "kendall", 31, ties=True)
    for est, args in (("Un", ("kendall",)), ("kendall_tau_b", ()), ("kendall_counts", ()),
                      ("UnN", (7, "kendall")), ("UnNT", (7, 3, "kendall"))):
        res = {}
        for algo in ("pairs", "sorted", "auto"):
            S = S0.copy()
            np.random.seed(17)
            value = getattr(os1, est)(S, *args, algo=algo)
            res[algo] = (value, S, np.random.get_state())
        for algo in ("sorted", "auto"):
            assert type(res[algo][0]) is type(res["pairs"][0])
            assert res[algo][0] == res["pairs"][0], (est, algo)
            assert np.array_equal(res[algo][1], res["pairs"][1])
            assert same_state(res[algo][2], res["pairs"][2])
        if est in ("UnN", "UnNT"):
            assert not np.array_equal(res["sorted"][1], S0)  # shuffled in place
        else:
            assert isinstance(res["sorted"][0], tuple if est == "kendall_counts" else np.float64)
    with pytest.raises(ValueError, match="algo"):
        os1.UnN(S0.copy(), 7, "var", algo="sorted")


def test_auto_takes_the_sorted_path_from_the_threshold(os1, monkeypatch):
    n = os1.SORTED_MIN_N
    S = sample(n, "kendall", 5)
    S[:, 1] = np.round(S[:, 1], 2)
    calls, native = [], os1.L.call
    monkeypatch.setattr(os1.L, "call", lambda name, *a: (calls.append(name), native(name, *a))[1])
    at = os1.kendall_counts(S)  # Kendall's default is "auto"
    below = os1.kendall_counts(S[:n - 1])
    os1.Un(S[:, 0].copy(), "gini")  # Gini's default is "pairs" at any size
    os1.Un(S[:, 0].copy(), "gini", algo="auto")
    assert calls == ["tw_self_sorted", "tw_self_pairs", "tw_self_pairs", "tw_self_sorted"]
    assert at == os1.kendall_counts(S, algo="pairs")
    assert below == os1.kendall_counts(S[:n - 1], algo="sorted")


# ------------------------------------------------------------------------------ Gini
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_gini_sizes(tw, os1, n, ties):
    S = sample(n, "gini", 11 * n + ties, ties)
    before = S.copy()
    want = o_Un(S, "gini")
    got = os1.Un(S, "gini", algo="sorted")
    print(n, ties, got, want, abs(got - want))
    assert isinstance(got, np.float64)
    assert np.isclose(got, want, rtol=RTOL, atol=ATOL), (got, want, abs(got - want))
    L = tw._lib
    raw = raw_sorted(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI, 0)[0][0]
    assert np.float64(raw / np.float64(n * (n - 1) // 2)) == got
    small = raw_sorted(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI, C)[0][0]
    assert abs(small - raw) <= 2 * EPS * abs(raw), (small, raw)  # each within an ulp of the sum
    assert np.array_equal(S, before)
    assert os1.Un(S, "gini") == os1.Un(S, "gini", algo="pairs")  # the default stays all pairs


@pytest.mark.parametrize("n", [3 * C + 5, 2 ** 15])
def test_gini_exact_on_integers(tw, gpu, n):
    """|s| < 2^20 and n <= 2^15: the pair sum is an integer below 2^53, every partial sum of
    either kernel is exact, and the two must agree bit for bit."""
    L = tw._lib
    S = np.random.RandomState(n).randint(-2 ** 20 + 1, 2 ** 20, size=n).astype(np.float64)
    pairs = raw_self_pairs(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI)[0][0]
    for chunk in (C, 0):
        got = raw_sorted(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI, chunk)[0][0]
        assert got == pairs and got == np.floor(got) and 0 < got < 2.0 ** 53, (got, pairs)


@pytest.mark.parametrize("chunk", [2048, 8192, 16384])
def test_gini_other_chunks(tw, gpu, chunk):
    L = tw._lib
    n = chunk + 5
    S = np.random.RandomState(chunk).randint(-1000, 1000, size=n).astype(np.float64)
    pairs = raw_self_pairs(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI)[0][0]
    assert raw_sorted(tw, S, [0, n], L.TW_F64, L.TW_SELF_GINI, chunk)[0][0] == pairs


@pytest.mark.parametrize("extra", [[np.nan], [np.inf], [np.inf, np.inf], [np.inf, -np.inf],
                                   [-np.inf], [-np.inf, -np.inf]])
def test_gini_non_finite(os1, extra):
    S = np.concatenate([sample(C + 50, "gini", 3), extra])
    np.random.RandomState(1).shuffle(S)
    with np.errstate(invalid="ignore"):
        want = o_Un(S, "gini")
    got = os1.Un(S, "gini", algo="sorted")
    assert isinstance(got, np.float64)
    assert (np.isnan(got) and np.isnan(want)) or got == want, (got, want)
    assert not np.isfinite(want)


def test_block_estimators_gini_sorted(os1):
    S0 = sample(3001, "gini", 41)
    a, b = S0.copy(), S0.copy()
    np.random.seed(23)
    got = os1.UnNT(a, 7, 3, "gini", algo="sorted")
    state = np.random.get_state()
    np.random.seed(23)
    want = os1.UnNT(b, 7, 3, "gini", algo="pairs")
    assert same_state(state, np.random.get_state()) and np.array_equal(a, b)
    assert np.isclose(got, want, rtol=RTOL, atol=ATOL), (got, want)


def test_native_refusals_on_the_device(tw, gpu):
    """TW_SELF_VAR, an odd chunk and a shard above 2^31 - 1 items are refused before a launch:
    the output keeps its fill."""
    import torch
    L = tw._lib
    S = L.to_device(np.arange(16.0))
    off = L.to_device(np.array([0, 8], dtype=np.int64))
    work = L.empty((1 << 16,), torch.int64)
    out = torch.full((1, 5), -7, dtype=torch.int64, device=S.device)
    for dtype, kern, chunk, total, max_n in ((L.TW_F64, L.TW_SELF_VAR, 0, 8, 8),
                                             (L.TW_F64, L.TW_SELF_KENDALL, 1000, 8, 8),
                                             (L.TW_F64, L.TW_SELF_KENDALL, 0, 2 ** 31, 2 ** 31)):
        with pytest.raises(ValueError, match="tw_self_sorted"):
            L.call("tw_self_sorted", S, off, 1, total, max_n, dtype, kern, chunk, work, out,
                   L.stream_handle())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
