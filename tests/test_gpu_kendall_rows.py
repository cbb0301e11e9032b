"""tuplewise.kendall_var on the GPU: tw_kendall_rows against the brute-force oracle of
test_kendall_var_cpu, against tw_kendall_matrix, and (distinct values, two columns) against a
Fenwick-tree count; the public functions against the CPU expressions fed with the device's
integers.  All results are exact integers, or floats formed from them by one division: every
comparison is ==."""
import functools
import statistics

import numpy as np
import pytest

from test_kendall_matrix_cpu import same_state, table
from test_kendall_var_cpu import f_var_a, f_var_b, o_row_moments

pytestmark = pytest.mark.gpu

SENT64 = 0x5A5A5A5A5A5A5A5A
PAD = 64  # sentinel elements behind every buffer

NS = [2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200]
PS = [1, 2, 15, 16, 17, 48, 63, 64, 65, 130]
KINDS = ["f64", "ties", "zeros_inf", "i64", "i64_ties", "i64_ends"]


# ------------------------------------------------------------------------------ inputs
def data(n, p, kind, seed):
    """An (n, p) table of one kind; from 4 columns on, column 1 is constant, column 2 repeats
    column 0 and column 3 reverses its order (-x, or ~x for int64: no overflow at INT64_MIN)."""
    rng = np.random.RandomState(seed)
    if kind == "f64":
        S = rng.normal(size=(n, p))
    elif kind == "ties":
        S = rng.randint(0, 4, size=(n, p)).astype(np.float64)
    elif kind == "zeros_inf":
        S = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -2.5]), size=(n, p))
    elif kind == "i64":
        S = rng.randint(-2 ** 62, 2 ** 62, size=(n, p)).astype(np.int64)
    elif kind == "i64_ties":
        S = rng.randint(0, 4, size=(n, p)).astype(np.int64)
    else:
        assert kind == "i64_ends"
        S = rng.choice(np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1, 1],
                                dtype=np.int64), size=(n, p))
    if p >= 4:
        S[:, 1] = S[0, 1]
        S[:, 2] = S[:, 0]
        S[:, 3] = ~S[:, 0] if S.dtype == np.int64 else -S[:, 0]
    return np.ascontiguousarray(S)


@functools.lru_cache(maxsize=None)
def case(n, p, kind):
    """(S, oracle) computed once and shared; the arrays are never modified."""
    S = data(n, p, kind, 100 * n + p)
    return S, o_row_moments(S, rows=256)


def kind_of(n, p):
    """One data kind per (n, p), cycled so that every n and every p meets every kind: the kind
    reaches tw_col_ranks only (tw_kendall_rows sees ranks), and test_gpu_kendall_matrix crosses
    that entry with every kind; test_row_moments_data_kinds runs every kind at the shapes that
    take each path of the rows kernel."""
    return KINDS[(NS.index(n) + PS.index(p)) % len(KINDS)]


class width:
    """tw_kendall_matrix_set_width for a with-block (the width both modules use)."""

    def __init__(self, tw, w):
        self.L, self.w = tw._lib, w

    def __enter__(self):
        self.L.call("tw_kendall_matrix_set_width", self.w)

    def __exit__(self, *exc):
        self.L.call("tw_kendall_matrix_set_width", 0)


def raw_rows(tw, S, off, w=None):
    """tw_col_ranks and tw_kendall_rows on rows [off[0], off[-1]) of S, with sentinels behind
    the four outputs and the work buffer: (R, Q, F, E), each (shards, p, p) int64 on the host."""
    import torch
    import tuplewise.kendall as K
    L = tw._lib
    lib = L.lib()
    off = np.asarray(off, np.int64)
    n_shards, total = len(off) - 1, int(off[-1] - off[0])
    max_n = int(np.diff(off).max())
    w = w or int(lib.tw_kendall_matrix_width(max_n))
    S = np.ascontiguousarray(S)
    p = S.shape[1]
    sd, od = L.to_device(S.reshape(-1)), L.to_device(off)
    ra = K._ranks_device(sd, od, n_shards, total, max_n, p, K._code(S), w)
    need = int(lib.tw_kendall_rows_work_bytes(n_shards, p))
    assert need >= 8 and need % 8 == 0
    work = torch.full((need // 8 + PAD,), SENT64, dtype=torch.int64, device="cuda")
    used = n_shards * p * p
    out = [torch.full((used + PAD,), SENT64, dtype=torch.int64, device="cuda") for _ in range(4)]
    L.call("tw_kendall_rows", ra, p, od, n_shards, max_n, w, work, *out, L.stream_handle())
    torch.cuda.synchronize()
    assert (work[need // 8:] == SENT64).all()
    for buf in out:
        assert (buf[used:] == SENT64).all()
    return tuple(b[:used].cpu().numpy().reshape(n_shards, p, p) for b in out)


def check(got, want, what):
    for name, g, w in zip("RQFE", got, want):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, name)
    R, Q, _, E = got[:4]
    assert np.array_equal(R, R.T) and np.array_equal(Q, Q.T) and np.array_equal(E, E.T), what


# ------------------------------------------------------------------------------ small shapes
@pytest.mark.parametrize("n", NS)
def test_row_moments_sizes(gpu, tw, n):
    """Every p at this n, both widths forced, float64 and int64 kinds cycled over the shapes;
    R against the matrix kernel at every shape."""
    import tuplewise.kendall as K
    import tuplewise.kendall_var as V
    for p in PS:
        kind = kind_of(n, p)
        S, want = case(n, p, kind)
        keep = S.copy()
        for w in (16, 32):
            with width(tw, w):
                m = V.row_moments(S)
                c = K.sign_counts(S)
            assert type(m.n) is int and m.n == n
            check(m[:4], want, (n, p, kind, w))
            assert np.array_equal(m.R, 2 * c.M) and np.array_equal(np.diag(m.R), 2 * c.Us)
        assert np.array_equal(S, keep)


@pytest.mark.parametrize("kind", KINDS)
def test_row_moments_data_kinds(gpu, tw, kind):
    """Every kind at every path of the kernel: 2 and 4 column blocks, a partly filled second
    group and two full groups with a third; one row, a ragged and a whole last chunk."""
    import tuplewise.kendall_var as V
    for n, p in ((129, 17), (64, 64), (200, 65), (2, 130), (65, 130)):
        S, want = case(n, p, kind)
        for w in (16, 32):
            with width(tw, w):
                check(V.row_moments(S)[:4], want, (n, p, kind, w))


def test_shards_of_mixed_sizes(gpu, tw):
    """Four shards of mixed sizes behind a leading gap: a shard's integers are the same alone
    and beside the others.  The rows before and after the partition hold the largest values of
    the dtype: a partner read from them would change every count."""
    sizes = [2, 65, 64, 131]
    lead, tail = 5, 3
    off = lead + np.concatenate([[0], np.cumsum(sizes)])
    for p, kind in ((17, "ties"), (65, "i64_ties"), (130, "f64")):
        S = data(int(off[-1]) + tail, p, kind, 31 + p)
        big = np.inf if S.dtype == np.float64 else np.iinfo(np.int64).max
        S[:lead] = big
        S[int(off[-1]):] = big
        for w in (16, 32):
            got = raw_rows(tw, S, off, w)
            for s in range(len(sizes)):
                lo, hi = int(off[s]), int(off[s + 1])
                want = o_row_moments(S[lo:hi])
                check([g[s] for g in got], want, (p, w, s))
                alone = raw_rows(tw, S, [lo, hi], w)
                check([g[0] for g in alone], want, (p, w, s, "alone"))


def test_a_shard_of_one_row_gives_zeros(gpu, tw):
    S = data(40, 5, "ties", 3)
    got = raw_rows(tw, S, [0, 20, 21, 40])
    for g in got:
        assert not g[1].any()
    check([g[2] for g in got], o_row_moments(S[21:40]), "after the single row")


# ------------------------------------------------------------------------------ hooks
def _with_hook(hook, v, run):
    old = hook(v)
    try:
        assert old >= 0
        return run()
    finally:
        assert hook(old) == v


def test_plan_and_anchor_hooks(gpu, tw):
    """The plan hook over {1, 2, 7, default} and the anchor hook over its whole range give the
    integers of the defaults, at one, two and three column groups and both widths."""
    import tuplewise.kendall_var as V
    lib = tw._lib.lib()
    assert lib.tw_kendall_rows_set_plan(0) == 0 and lib.tw_kendall_rows_set_anchors(0) == 0
    for n, p in ((200, 64), (129, 17), (333, 130)):
        S = data(n, p, "ties", n + p)
        want = o_row_moments(S, rows=128)
        for w in (16, 32):
            with width(tw, w):
                base = V.row_moments(S)[:4]
                check(base, want, (n, p, w))
                for plan in (1, 2, 7, 0):
                    for k in (0, 1, 2, 4):
                        got = _with_hook(
                            lib.tw_kendall_rows_set_plan, plan,
                            lambda: _with_hook(lib.tw_kendall_rows_set_anchors, k,
                                               lambda: V.row_moments(S)[:4]))
                        check(got, base, (n, p, w, plan, k))
    assert lib.tw_kendall_rows_set_plan(0) == 0 and lib.tw_kendall_rows_set_anchors(0) == 0


# ------------------------------------------------------------------------------ larger shards
def test_mid_size(gpu, tw):
    import tuplewise.kendall_var as V
    S = data(5000, 3, "ties", 77)
    S[:, 2] = np.random.RandomState(1).normal(size=5000)
    check(V.row_moments(S)[:4], o_row_moments(S, rows=250), "n = 5000")


def _below_in_both(a, b):
    """L_i = #{j : a_j < a_i and b_j < b_i} for permutations a, b of 0 .. n - 1 (a Fenwick tree
    over b, the points taken by rising a)."""
    n = len(a)
    tree = [0] * (n + 1)
    L = np.zeros(n, np.int64)
    bl = b.tolist()
    for i in np.argsort(a).tolist():
        k, s = bl[i], 0
        while k > 0:
            s += tree[k]
            k -= k & -k
        L[i] = s
        k = bl[i] + 1
        while k <= n:
            tree[k] += 1
            k += k & -k
    return L


@pytest.mark.parametrize("n,w", [(65536, 16), (70001, 32)])
def test_distinct_values_at_the_width_edge(gpu, tw, n, w):
    """The last 16-bit size and the natural int32 path: with distinct values c_i(0, 1) =
    2 (2 L_i + n - 1 - ra_i - rb_i) - (n - 1) and u_i = n - 1 for every point."""
    import tuplewise.kendall_var as V
    assert int(tw._lib.lib().tw_kendall_matrix_width(n)) == w
    rng = np.random.RandomState(n)
    ra = rng.permutation(n)
    rb = np.where(rng.rand(n) < 0.5, ra, rng.permutation(n))  # correlated, then made distinct
    rb = np.argsort(np.argsort(rb + rng.rand(n)))
    S = np.ascontiguousarray(np.stack([ra, rb], axis=1).astype(np.float64))
    c = 2 * (2 * _below_in_both(ra, rb) + n - 1 - ra - rb) - (n - 1)
    c = [int(v) for v in c]
    sc, sq, u = sum(c), sum(v * v for v in c), n - 1
    m = V.row_moments(S)
    assert m.R.tolist() == [[n * u, sc], [sc, n * u]]
    assert m.Q.tolist() == [[n * u * u, sq], [sq, n * u * u]]
    assert m.F.tolist() == [[n * u * u, u * sc], [u * sc, n * u * u]]
    assert m.E.tolist() == [[n * u * u] * 2] * 2


# ------------------------------------------------------------------------- public functions
def test_public_functions_on_the_device_integers(gpu, tw):
    import tuplewise.kendall as K
    import tuplewise.kendall_var as V
    for kind in ("f64", "ties"):
        S = data(301, 6, kind, 40)
        n, p = S.shape
        keep = S.copy()
        m = V.row_moments(S)
        for variant in ("a", "b"):
            tv = V.tau_var(S, variant)
            assert np.array_equal(tv.tau, K.tau_matrix(S, variant=variant), equal_nan=True)
            for a in range(p):
                for b in range(p):
                    fr = (f_var_a(m.R, m.Q, n, a, b) if variant == "a"
                          else f_var_b(m.R, m.Q, m.F, m.E, n, a, b))
                    if fr is None:
                        assert (a == 1 or b == 1) and np.isnan(tv.var[a, b])
                    else:
                        assert tv.var[a, b] == float(fr), (kind, variant, a, b)
            assert np.array_equal(tv.se, np.sqrt(np.maximum(tv.var, 0.0)), equal_nan=True)
            tau, lo, hi = V.tau_ci(S, variant, 0.9)
            z = statistics.NormalDist().inv_cdf(0.5 + 0.5 * 0.9)
            assert np.array_equal(tau, tv.tau, equal_nan=True)
            assert np.array_equal(lo, np.clip(tv.tau - z * tv.se, -1, 1), equal_nan=True)
            assert np.array_equal(hi, np.clip(tv.tau + z * tv.se, -1, 1), equal_nan=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                assert np.array_equal(V.z_scores(S, variant), tv.tau / tv.se, equal_nan=True)
        tb = V.tau_var(S, "b")
        assert tb.var[0, 2] == 0.0 and tb.var[0, 3] == 0.0 and tb.var[4, 4] == 0.0
        assert np.array_equal(S, keep)


@pytest.mark.parametrize("N", [3, 8])
def test_UnN_var(gpu, tw, N):
    import tuplewise.kendall as K
    import tuplewise.kendall_var as V
    S = table(64 * 5 + 7, 3, 90 + N, ties=True)
    A, B = S.copy(), S.copy()
    np.random.seed(55 + N)
    value, var = V.UnN_var(A, N)
    after = np.random.get_state()
    np.random.seed(55 + N)
    want = K.UnN(B, N)
    assert np.array_equal(value, want) and np.array_equal(A, B)
    assert same_state(after, np.random.get_state())
    k = int(S.shape[0] / N)
    blocks = []
    for b in range(N):
        R, Q, _, _ = o_row_moments(B[b * k:(b + 1) * k])
        blocks.append([[float(f_var_a(R, Q, k, a, c)) for c in range(3)] for a in range(3)])
    assert np.array_equal(var, K._last_axis_mean(np.array(blocks)).reshape(3, 3) / N)
