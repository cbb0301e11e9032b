"""tuplewise.onesample on the device against the NumPy oracle of tests/test_onesample_cpu.py:
Kendall integers and values bit for bit, Gini / var at the package's float pair-sum contract
(rtol 1e-12, atol 1e-15; tests/test_gpu_parity.py), RNG consumption and the in-place shuffle
exactly."""
import numpy as np
import pytest

from test_onesample_cpu import (KERNELS, o_kendall_counts, o_kendall_tau_b, o_pairs_value, o_UB,
                                o_Un, o_UnN, o_UnNB, o_UnNBT, o_UnNT, sample)

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-12, 1e-15

# n as a function of the tile edge T: the diagonal-only case, ragged edges, the first
# off-diagonal tile, a full second row of the triangle
SIZES = {"2": lambda T: 2, "3": lambda T: 3, "63": lambda T: 63, "64": lambda T: 64,
         "65": lambda T: 65, "T-1": lambda T: T - 1, "T": lambda T: T, "T+1": lambda T: T + 1,
         "2T+1": lambda T: 2 * T + 1, "3T+5": lambda T: 3 * T + 5}


@pytest.fixture(scope="module")
def os1(gpu):
    import tuplewise.onesample as m
    return m


@pytest.fixture(scope="module")
def tile(tw, gpu):
    return int(tw._lib.lib().tw_self_pairs_tile())


def same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def check(got, want, kernel):
    if kernel == "kendall":
        assert isinstance(got, np.float64)
        assert got == want or (np.isnan(got) and np.isnan(want)), (got, want)
    else:
        print(kernel, got, want, abs(got - want))
        assert np.isclose(got, want, rtol=RTOL, atol=ATOL), (got, want, abs(got - want))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("size", list(SIZES))
def test_sizes(os1, tile, size, kernel):
    n = SIZES[size](tile)
    S = sample(n, kernel, 7 * n + 1)
    before = S.copy()
    check(os1.Un(S, kernel), o_Un(S, kernel), kernel)
    if kernel == "kendall":
        assert os1.kendall_counts(S) == o_kendall_counts(S)
        got, want = os1.kendall_tau_b(S), o_kendall_tau_b(S)
        assert got == want, (got, want)
        T = sample(n, kernel, n, ties=True)
        assert os1.kendall_counts(T) == o_kendall_counts(T)
        got, want = os1.kendall_tau_b(T), o_kendall_tau_b(T)
        assert got == want or (np.isnan(got) and np.isnan(want)), (got, want)
    assert np.array_equal(S, before)


def raw_self_pairs(tw, flat, off, dtype, kern):
    """tw_self_pairs called directly: the per-shard outputs on the host."""
    import torch
    L = tw._lib
    off = np.asarray(off, dtype=np.int64)
    ns = len(off) - 1
    max_n = int(np.diff(off).max())
    sd = L.to_device(flat if flat.size else np.zeros(2, flat.dtype))
    od = L.to_device(off)
    work = L.empty((L.lib().tw_self_pairs_work_bytes(ns, max_n) // 8,), torch.int64)
    ken = kern == L.TW_SELF_KENDALL
    out = torch.full((ns, 5 if ken else 1), -7, dtype=torch.int64 if ken else torch.float64,
                     device=sd.device)
    L.call("tw_self_pairs", sd, od, ns, max_n, dtype, kern, work, out, L.stream_handle())
    host = out.cpu().numpy()
    return host.view(np.uint64) if ken else host


@pytest.mark.parametrize("kernel", KERNELS)
def test_mixed_shards_in_one_launch(tw, gpu, tile, kernel):
    L = tw._lib
    sizes = [2, 2 * tile + 3, 1, 0, tile, 5]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    S = sample(int(off[-1]), kernel, 99, ties=(kernel == "kendall"))
    w = 2 if kernel == "kendall" else 1
    kern = {"gini": L.TW_SELF_GINI, "var": L.TW_SELF_VAR, "kendall": L.TW_SELF_KENDALL}[kernel]
    got = raw_self_pairs(tw, S.reshape(-1), off, L.TW_F64, kern)
    for s, n in enumerate(sizes):
        part = S[off[s]:off[s + 1]]
        if n < 2:
            assert not got[s].any(), (s, got[s])  # zeros, and written
            continue
        alone = raw_self_pairs(tw, part.reshape(-1), [0, n], L.TW_F64, kern)
        assert np.array_equal(got[s], alone[0]), (s, got[s], alone[0])
        if kernel == "kendall":
            assert tuple(int(v) for v in got[s]) == o_kendall_counts(part)
        else:
            pairs = n * (n - 1) // 2
            check(np.float64(got[s][0] / np.float64(pairs)), o_Un(part, kernel), kernel)
    assert w * off[-1] == S.size


def edge_samples():
    rng = np.random.RandomState(3)
    ties = rng.randint(0, 4, size=(700, 2)).astype(np.float64)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 2.5])
    nonfinite = special[rng.randint(0, len(special), size=(600, 2))]
    big = 2 ** 62 + rng.randint(0, 3, size=(300, 2)).astype(np.int64)  # equal as doubles
    return {"ties": ties, "nonfinite": np.ascontiguousarray(nonfinite), "int64": big}


@pytest.mark.parametrize("which", ["ties", "nonfinite", "int64"])
def test_kendall_edge_data(os1, which):
    S = edge_samples()[which]
    want = o_kendall_counts(S)
    assert os1.kendall_counts(S) == want
    got, ref = os1.kendall_tau_b(S), o_kendall_tau_b(S)
    assert got == ref or (np.isnan(got) and np.isnan(ref))
    check(os1.Un(S, "kendall"), o_Un(S, "kendall"), "kendall")
    if which == "int64":
        pair = np.array([[2 ** 62, 2 ** 62 + 1], [2 ** 62 + 1, 2 ** 62]], dtype=np.int64)
        assert float(pair[0, 0]) == float(pair[0, 1])  # tied once rounded to double ...
        assert os1.kendall_counts(pair) == (0, 1, 0, 0, 0)  # ... ordered as integers
        assert want[2] < 300 * 299 // 2 // 2  # a third of the a-pairs tie, not all of them
    if which == "nonfinite":
        c, d, tx, ty, txy = want
        assert c + d + tx + ty - txy < 600 * 599 // 2  # NaN pairs fall in no class


@pytest.mark.parametrize("kernel", KERNELS)
def test_multi_workgroup(os1, kernel):
    S = sample(5000, kernel, 11)
    check(os1.Un(S, kernel), o_Un(S, kernel), kernel)
    if kernel == "kendall":
        assert os1.kendall_counts(S) == o_kendall_counts(S)


def test_other_dtypes_and_columns(os1):
    S = np.random.RandomState(2).randint(-50, 50, size=(300, 1)).astype(np.int32)
    want = o_Un(np.asarray(S, np.float64), "gini")
    check(os1.Un(S, "gini"), want, "gini")
    check(os1.Un(S[:, 0].astype(np.float32), "var"), o_Un(S, "var"), "var")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("B", [1, 1000])
def test_UB_and_UB_indices(os1, kernel, B):
    S = sample(1000, kernel, 21, ties=(kernel == "kendall"))
    np.random.seed(77 + B)
    i = np.random.randint(0, 1000, B)
    j = np.random.randint(0, 999, B)
    j += (j >= i)
    check(os1.UB_indices(S, i, j, kernel), o_pairs_value(S, i, j, kernel), kernel)
    np.random.seed(77 + B)
    gi, gj = os1._draw_pairs(1000, B)
    assert np.array_equal(gi, i) and np.array_equal(gj, j) and np.all(gi != gj)
    np.random.seed(5 + B)
    got = os1.UB(S, B, kernel)
    mine = np.random.get_state()
    np.random.seed(5 + B)
    want = o_UB(S, B, kernel)
    assert same_state(mine, np.random.get_state())
    check(got, want, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("est", ["UnN", "UnNT", "UnNB", "UnNBT"])
def test_block_estimators(os1, est, kernel):
    n, N, T, B = 1003, 10, 3, 500
    S0 = sample(n, kernel, 31, ties=(kernel == "kendall"))
    mine, ref = S0.copy(), S0.copy()
    args = {"UnN": (N,), "UnNT": (N, T), "UnNB": (N, B), "UnNBT": (N, B, T)}[est]
    oracle = {"UnN": o_UnN, "UnNT": o_UnNT, "UnNB": o_UnNB, "UnNBT": o_UnNBT}[est]
    np.random.seed(13)
    got = getattr(os1, est)(mine, *args, kernel)
    state = np.random.get_state()
    np.random.seed(13)
    want = oracle(ref, *args, kernel)
    assert same_state(state, np.random.get_state())
    assert np.array_equal(mine, ref) and not np.array_equal(mine, S0)  # shuffled in place
    check(got, want, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_untagged_block_function(os1, kernel):
    S0 = sample(1003, kernel, 41)
    a, b, c = S0.copy(), S0.copy(), S0.copy()
    np.random.seed(3)
    tagged = os1.UnN(a, 10, kernel)
    np.random.seed(3)
    plain = os1.UN(b, 10, lambda s: os1.Un(s, kernel))  # no tag: looped over in Python
    assert np.array_equal(a, b)
    assert tagged == plain if kernel == "kendall" else np.isclose(tagged, plain, rtol=RTOL,
                                                                  atol=ATOL)
    if kernel == "gini":  # Un itself carries a tag (its default kernel)
        np.random.seed(3)
        assert os1.UN(c, 10, os1.Un) == tagged


@pytest.mark.parametrize("kernel", KERNELS)
def test_UN_refuses_blocks_of_one_point(os1, kernel):
    S = sample(10, kernel, 51)
    before = S.copy()
    np.random.seed(9)
    state = np.random.get_state()
    for call in (lambda: os1.UnN(S, 10, kernel), lambda: os1.UnNB(S, 6, 4, kernel),
                 lambda: os1.UnNT(S, 7, 2, kernel), lambda: os1.UnNBT(S, 9, 4, 2, kernel),
                 lambda: os1.UN(S, 10, lambda s: 1.0)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(S, before) and same_state(state, np.random.get_state())
