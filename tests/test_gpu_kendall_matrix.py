"""tuplewise.kendall on the GPU: tw_col_ranks and tw_kendall_matrix against the brute-force
oracle of test_kendall_matrix_cpu and against the (n, 2) Kendall of tuplewise.onesample.  All
results are exact integers (or floats formed from them by the same expressions): every
comparison is ==."""
import functools

import numpy as np
import pytest

from test_kendall_matrix_cpu import (o_sign_counts, o_UnN_matrix, o_UnNT_matrix, same_state,
                                     table)

pytestmark = pytest.mark.gpu

SENT16, SENT32, SENT64 = -21846, 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
PAD = 64  # sentinel elements behind every buffer


# ------------------------------------------------------------------------------ raw calls
def raw_ranks(tw, S, off, width, lead=0):
    """tw_col_ranks on rows [off[0], off[-1]) of S (lead: off[0]): the image as an int64 array
    of ranks (the 16-bit bias removed), sentinels behind the image and the work buffer checked."""
    import torch
    L = tw._lib
    lib = L.lib()
    S = np.ascontiguousarray(S)
    p = S.shape[1]
    off = np.asarray(off, np.int64)
    n_shards, total = len(off) - 1, int(off[-1] - off[0])
    max_n = int(np.diff(off).max())
    code = L.TW_F64 if S.dtype == np.float64 else L.TW_I64
    sd, od = L.to_device(S.reshape(-1)), L.to_device(off)
    need = int(lib.tw_col_ranks_work_bytes(n_shards, total, max_n, p))
    assert need >= 8 and need % 8 == 0
    work = torch.full((need // 8 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    if width == 16:
        img = torch.full((total * p + PAD,), SENT16, dtype=torch.int16, device="cuda")
    else:
        img = torch.full((total * p + PAD,), SENT32, dtype=torch.int32, device="cuda")
    L.call("tw_col_ranks", sd, od, n_shards, total, max_n, p, code, width, work, img,
           L.stream_handle())
    torch.cuda.synchronize()
    assert (work[need // 8:] == SENT64).all()
    h = img.cpu().numpy()
    assert (h[total * p:] == (SENT16 if width == 16 else SENT32)).all()
    h = h[:total * p].astype(np.int64)
    return h + 32768 if width == 16 else h


def want_ranks(S, off):
    out = []
    for s in range(len(off) - 1):
        blk = S[off[s]:off[s + 1]]
        for c in range(S.shape[1]):
            col = blk[:, c]
            if col.dtype == np.float64:
                col = col + 0.0  # -0.0 ties with 0.0 either way; searchsorted agrees
            out.append(np.searchsorted(np.sort(col), col, "left"))
    return np.concatenate(out).astype(np.int64) if out else np.zeros(0, np.int64)


def raw_matrix(tw, S, Y, off, width=None):
    """Both native calls on resident rows with sentinels behind M, Ua, Ub and the work buffer.
    Returns (M (shards, p, q), Ua, Ub) int64 on the host."""
    import torch
    import tuplewise.kendall as K
    L = tw._lib
    lib = L.lib()
    off = np.asarray(off, np.int64)
    n_shards, total = len(off) - 1, int(off[-1] - off[0])
    max_n = int(np.diff(off).max())
    width = width or int(lib.tw_kendall_matrix_width(max_n))
    od = L.to_device(off)
    S = np.ascontiguousarray(S)
    p = S.shape[1]
    sd = L.to_device(S.reshape(-1))
    ra = K._ranks_device(sd, od, n_shards, total, max_n, p, K._code(S), width)
    if Y is None:
        rb, q = ra, p
    else:
        Y = np.ascontiguousarray(Y)
        q = Y.shape[1]
        yd = L.to_device(Y.reshape(-1))
        rb = K._ranks_device(yd, od, n_shards, total, max_n, q, K._code(Y), width)
    need = int(lib.tw_kendall_matrix_work_bytes(n_shards, p, q))
    work = torch.full((need // 8 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    M = torch.full((n_shards * p * q + PAD,), SENT64, dtype=torch.int64, device="cuda")
    Ua = torch.full((n_shards * p + PAD,), SENT64, dtype=torch.int64, device="cuda")
    Ub = torch.full((n_shards * q + PAD,), SENT64, dtype=torch.int64, device="cuda")
    L.call("tw_kendall_matrix", ra, p, rb, q, od, n_shards, max_n, width, work, M, Ua, Ub,
           L.stream_handle())
    torch.cuda.synchronize()
    assert (work[need // 8:] == SENT64).all()
    for buf, used in ((M, n_shards * p * q), (Ua, n_shards * p), (Ub, n_shards * q)):
        assert (buf[used:] == SENT64).all()
    return (M[:n_shards * p * q].cpu().numpy().reshape(n_shards, p, q),
            Ua[:n_shards * p].cpu().numpy().reshape(n_shards, p),
            Ub[:n_shards * q].cpu().numpy().reshape(n_shards, q))


class hooks:
    """Tuning hooks set for a with-block and restored to their defaults after it."""

    def __init__(self, tw, **kw):
        self.L, self.kw = tw._lib, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.L.call(f"tw_kendall_matrix_set_{k}", v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.L.call(f"tw_kendall_matrix_set_{k}", 0)


@functools.lru_cache(maxsize=None)
def case(n, p, ties, q=0):
    """(S, Y or None, oracle) computed once and shared; the arrays are never modified."""
    S = table(n, p, 1000 * n + p + ties, ties)
    Y = table(n, q, 77 * n + q + ties, ties) if q else None
    return S, Y, o_sign_counts(S, Y)


def check(counts, want):
    M, Us, Uy, P = want
    assert counts.pairs == P
    assert np.array_equal(counts.M, M)
    assert np.array_equal(counts.Us, Us) and np.array_equal(counts.Uy, Uy)


def tile(tw):
    return int(tw._lib.lib().tw_kendall_matrix_tile())


# ------------------------------------------------------------------------------ tw_col_ranks
def rank_data(n, p, kind, seed):
    rng = np.random.RandomState(seed)
    if kind == "f64":
        return rng.normal(size=(n, p))
    if kind == "ties":
        return rng.randint(0, 6, size=(n, p)).astype(np.float64)
    if kind == "zeros_inf":
        return rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -2.5]), size=(n, p))
    if kind == "i64":
        return rng.randint(-2 ** 62, 2 ** 62, size=(n, p)).astype(np.int64)
    if kind == "i64_ties":
        return rng.randint(0, 6, size=(n, p)).astype(np.int64)
    assert kind == "i64_ends"
    return rng.choice(np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1],
                               dtype=np.int64), size=(n, p))


RANK_KINDS = ["f64", "ties", "zeros_inf", "i64", "i64_ties", "i64_ends"]


def rank_sizes(tw):
    lib = tw._lib.lib()
    big = 16384  # kMaxChunk of csrc/sortkeys.h
    C = int(lib.tw_col_ranks_chunk(big))  # the chunk of large shards: more than one from C + 1 on
    return sorted({2, 3, 1023, 1024, 1025, 2048, 2049, C - 1, C, C + 1, big, big + 1, 2 * big + 5})


def test_col_ranks_sizes(gpu, tw):
    for i, n in enumerate(rank_sizes(tw)):
        for p in (1, 3, 17):
            # every data kind at every (n, p) would be 200 launches: cycle through them instead
            kind = RANK_KINDS[(i + p) % len(RANK_KINDS)]
            S = rank_data(n, p, kind, n + p)
            want = want_ranks(S, [0, n])
            for width in (16, 32):
                got = raw_ranks(tw, S, [0, n], width)
                assert np.array_equal(got, want), (n, p, kind, width)


@pytest.mark.parametrize("kind", RANK_KINDS)
def test_col_ranks_data_kinds(gpu, tw, kind):
    for n, p in ((1025, 3), (4100, 2)):
        S = rank_data(n, p, kind, 5)
        for width in (16, 32):
            assert np.array_equal(raw_ranks(tw, S, [0, n], width), want_ranks(S, [0, n]))


@pytest.mark.parametrize("kind", ["ties", "i64"])
def test_col_ranks_mixed_shards(gpu, tw, kind):
    off = np.array([7, 7 + 1100, 7 + 1101, 7 + 1101 + 4200, 7 + 1101 + 4200 + 3])
    S = rank_data(int(off[-1]) + 5, 3, kind, 9)
    for width in (16, 32):
        assert np.array_equal(raw_ranks(tw, S, off, width), want_ranks(S, off))


# ------------------------------------------------------------------------------ sign_counts
def _sizes(tw):
    T = tile(tw)
    ns = [2, 3, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]
    ps = [1, 2, 15, 16, 17, 33, 64, 65, 130]
    cases = {(n, p) for n in ns for p in (17, 65)} | {(n, p) for p in ps for n in (T + 1, 3 * T + 5)}
    return sorted(cases)


def test_sign_counts_sizes(gpu, tw):
    import tuplewise.kendall as K
    for n, p in _sizes(tw):
        for ties in (False, True):
            S, _, want = case(n, p, ties)
            for width in (0, 16, 32):
                with hooks(tw, width=width):
                    got = K.sign_counts(S)
                check(got, want)
                assert np.array_equal(got.M, got.M.T), (n, p, ties, width)


@pytest.mark.parametrize("p,q", [(3, 17), (17, 3), (64, 2), (65, 16)])
def test_cross_calls(gpu, tw, p, q):
    """Unrelated columns: M is not symmetric, so a row / column swap or a wrong operand map of
    the matrix instruction cannot pass."""
    import tuplewise.kendall as K
    T = tile(tw)
    for n in (17, 2 * T + 1):
        for ties in (False, True):
            S, Y, want = case(n, p, ties, q)
            assert p != q or not np.array_equal(want[0], want[0].T)
            for width in (16, 32):
                with hooks(tw, width=width):
                    check(K.sign_counts(S, Y), want)


def test_cross_call_of_a_copy_is_the_symmetric_call(gpu, tw):
    import tuplewise.kendall as K
    for n, p in ((tile(tw) + 1, 17), (3 * tile(tw) + 5, 130)):
        S, _, want = case(n, p, True)
        for width in (16, 32):
            with hooks(tw, width=width):
                a, b = K.sign_counts(S), K.sign_counts(S, S.copy())
            check(a, want)
            check(b, want)
            assert np.array_equal(b.M, b.M.T)


def test_flush_and_plan_hooks(gpu, tw):
    import tuplewise.kendall as K
    T = tile(tw)
    for p, q in ((65, 0), (17, 0), (17, 33)):
        for n, settings in ((2 * T + 1, ({"flush": 1}, {"flush": 3})),
                            (3 * T + 5, ({"plan": 3}, {"plan": 1}, {"plan": 3, "flush": 3}))):
            S, Y, want = case(n, p, True, q)
            for kw in settings:
                for width in (16, 32):
                    with hooks(tw, width=width, **kw):
                        check(K.sign_counts(S, Y), want)


def test_blocks_of_mixed_sizes(gpu, tw):
    """Four shards of mixed sizes behind a leading gap: the integers of a shard are the same
    alone and beside the others; sentinels behind every output and the work buffer."""
    T = tile(tw)
    sizes = [T + 3, 1, 2 * T + 1, 17]
    lead = 5
    off = lead + np.concatenate([[0], np.cumsum(sizes)])
    for p, q in ((17, 0), (65, 0), (3, 17)):
        S = table(int(off[-1]) + 3, p, 31 + p, ties=True)
        Y = table(int(off[-1]) + 3, q, 32 + q, ties=True) if q else None
        for width in (16, 32):
            M, Ua, Ub = raw_matrix(tw, S, Y, off, width)
            for s, k in enumerate(sizes):
                lo, hi = int(off[s]), int(off[s + 1])
                if k < 2:
                    assert not M[s].any() and not Ua[s].any() and not Ub[s].any()
                    continue
                wm, wa, wb, _ = o_sign_counts(S[lo:hi], None if Y is None else Y[lo:hi])
                assert np.array_equal(M[s], wm) and np.array_equal(Ua[s], wa)
                assert np.array_equal(Ub[s], wb)
                M1, Ua1, Ub1 = raw_matrix(tw, S, Y, [lo, hi], width)
                assert np.array_equal(M1[0], wm) and np.array_equal(Ua1[0], wa)
                assert np.array_equal(Ub1[0], wb)


# ------------------------------------------------------------------------- saturation edges
def _against_onesample(S, width_want, tw):
    import tuplewise.kendall as K
    import tuplewise.onesample as os1
    n, p = S.shape
    assert int(tw._lib.lib().tw_kendall_matrix_width(n)) == width_want
    got = K.sign_counts(S)
    P = n * (n - 1) // 2
    assert got.pairs == P and np.array_equal(got.M, got.M.T)
    for a in range(p):
        for b in range(a + 1, p):
            c, d, tx, ty, _ = os1.kendall_counts(np.ascontiguousarray(S[:, [a, b]]),
                                                 algo="sorted")
            assert int(got.M[a, b]) == c - d
            assert int(got.Us[a]) == P - tx and int(got.Us[b]) == P - ty
    assert np.array_equal(np.diag(got.M), got.Us) and np.array_equal(got.Us, got.Uy)


def test_rank_differences_past_int16(gpu, tw):
    """33 000 distinct values: rank differences pass 32 767, the smallest shape at which the
    packed 16-bit subtract saturates."""
    rng = np.random.RandomState(3)
    a = rng.permutation(33000).astype(np.float64)
    S = np.ascontiguousarray(np.stack([a, 0.3 * a + rng.permutation(33000)], axis=1))
    _against_onesample(S, 16, tw)


def test_the_last_16_bit_size(gpu, tw):
    rng = np.random.RandomState(4)
    a = rng.permutation(65536).astype(np.float64)
    S = np.ascontiguousarray(np.stack([a, rng.permutation(65536).astype(np.float64)], axis=1))
    _against_onesample(S, 16, tw)


def test_the_first_32_bit_size(gpu, tw):
    rng = np.random.RandomState(5)
    S = rng.randint(0, 50000, size=(70001, 3)).astype(np.float64)
    _against_onesample(S, 32, tw)


# ------------------------------------------------------------------------- public functions
def test_tau_matrix_is_the_pair_functions(gpu, tw):
    import tuplewise.kendall as K
    import tuplewise.onesample as os1
    for ties in (False, True):
        S = table(301, 5, 40 + ties, ties)
        if ties:
            S[:, 3] = 2.0
        keep = S.copy()
        tb, ta = K.tau_matrix(S), K.tau_matrix(S, variant="a")
        assert np.array_equal(ta, K.Un(S)) and np.array_equal(S, keep)
        Y = table(301, 3, 50 + ties, ties)
        tc = K.tau_matrix(S, Y)
        for a in range(5):
            for b in range(5):
                pair = np.ascontiguousarray(S[:, [a, b]])
                assert ta[a, b] == os1.Un(pair, "kendall")
                want = os1.kendall_tau_b(pair)
                if np.isnan(want):
                    assert np.isnan(tb[a, b])
                elif a == b:
                    assert tb[a, b] == 1.0
                else:
                    assert tb[a, b] == want
            for b in range(3):
                want = os1.kendall_tau_b(np.ascontiguousarray(np.stack([S[:, a], Y[:, b]], 1)))
                assert (np.isnan(want) and np.isnan(tc[a, b])) or tc[a, b] == want


@pytest.mark.parametrize("N,T", [(3, 1), (8, 1), (64, 1), (8, 3)])
def test_blocks_at_two_columns_are_onesamples(gpu, tw, N, T):
    import tuplewise.kendall as K
    import tuplewise.onesample as os1
    S = table(64 * 9 + 5, 2, 60 + N)
    A, B = S.copy(), S.copy()
    np.random.seed(99 + N)
    got = K.UnN(A, N) if T == 1 else K.UnNT(A, N, T)
    after = np.random.get_state()
    np.random.seed(99 + N)
    want = os1.UnN(B, N, "kendall") if T == 1 else os1.UnNT(B, N, T, "kendall")
    assert got[0, 1] == want and got[1, 0] == want
    assert same_state(after, np.random.get_state()) and np.array_equal(A, B)


def test_blocks_at_five_columns(gpu, tw):
    import tuplewise.kendall as K
    S = table(203, 5, 70, ties=True)
    for N, T in ((4, 1), (9, 2)):
        A, B = S.copy(), S.copy()
        np.random.seed(8)
        got = K.UnN(A, N) if T == 1 else K.UnNT(A, N, T)
        after = np.random.get_state()
        np.random.seed(8)
        want = o_UnN_matrix(B, N) if T == 1 else o_UnNT_matrix(B, N, T)
        assert np.array_equal(got, want) and np.array_equal(A, B)
        assert same_state(after, np.random.get_state())
