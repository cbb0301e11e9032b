"""Span items of the digit-table class count (csrc/chainclass.h bits_count_span_digits,
class_span_entries / class_span_item) behind tw_count_pairs_chain_planes: an item
walks M consecutive run-table entries of its bag on one x tile, keeps the low digit tables and
rebuilds G, P, E and the top digit per run of a new class; tw_count_chain_class_span forces M.

Bounds 2^16 - 1 (NB = 16), 2^16 (NB = 18), the bench's 1 000 000 (NB = 20: the digit loop at
k = 8, the masked-plane fallback at k = 6, which keeps one entry per item) and 2^22 (NB = 24:
fallback only).  Spans: forced M in {1, 2, 3, 5, cap, cap + 7} and the automatic rule.  Bags: the
nine of test_gpu_count_digits (every run length, all z equal, digit boundaries, no z, ...), bags
whose z fill exactly 29 and 31 classes of one entry each (M j - 1 and M j + 1 entries for every
M in {2, 3, 5}: the last span short by one, or of one entry), a bag with one class of
3 * chunk + 1 images (consecutive runs of one class, which keep G, P and the top digit) between
two other classes, a bag of one z beside a bag of hundreds of entries; x sizes 31, 2047, 2049,
4101.  Every count equals, exactly, the NumPy integer count, the k = 0 path and M = 1.  The
workspace holds 0xFF before every call; two calls with different M share one in stream order."""
import numpy as np
import pytest

import test_gpu_count_classes as C
import test_gpu_count_digits as D
import test_gpu_count_masked as M

P = C.P
pytestmark = pytest.mark.gpu

# bound -> (NB, class bits to force): 29 .. 31 classes below the bound at the smallest k
CASES = {2 ** 16 - 1: (16, (8, 5)),
         2 ** 16: (18, (8, 7)),
         1_000_000: (20, (8, 6)),
         2 ** 22: (24, (8, 6))}
PLANS = ((2, 8), (0, 600))  # runs of at most 8 images (many entries) and of at most 600
CHUNK = 8                   # the run length of PLANS[0]


@pytest.fixture(autouse=True)
def span_reset():
    """The span control and the other chain hooks, back to automatic whatever the test did."""
    yield
    from tuplewise import _lib as L
    L.lib().tw_count_chain_class_span(0)
    C._reset(L)


def _set_span(L, runs):
    return int(L.lib().tw_count_chain_class_span(runs))


def _cap(a, k, zc):
    """class_capacity of a launch: 2^k + ceil(max_nz / max(zc, 8))."""
    return (1 << k) + -(-a.head[9] // max(zc, 8))


def _bags(rng, bound, nb, ks):
    shift = nb - min(ks)
    narrow = 1 << (nb - 8)  # low bits below this: one class per field at every k <= 8
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    fields = lambda n: np.arange(min(n, bound >> shift), dtype=np.int64) << shift
    one_each = lambda n: fields(n) + rng.randint(0, narrow, len(fields(n)))
    # 3 * chunk + 1 images of field 2 between one image of field 1 and two of field 3
    long_class = np.concatenate([(1 << shift) + rng.randint(0, narrow, 1),
                                 (2 << shift) + rng.randint(0, narrow, 3 * CHUNK + 1),
                                 (3 << shift) + rng.randint(0, narrow, 2)]).astype(np.int64)
    many, c29, c31 = anyx(700), one_each(29), one_each(31)  # (NB = 24: the 16 fields there are)
    return D._bags(rng, bound, nb, ks) + [
        (np.concatenate([anyx(2047 - len(c29)), c29]), rng.permutation(c29)),
        (np.concatenate([anyx(2049 - len(c31)), c31]), rng.permutation(c31)),
        (np.concatenate([anyx(4101 - len(long_class)), long_class]), long_class),
        (anyx(31), np.array([bound // 2], np.int64)),                # one entry ...
        (np.concatenate([anyx(4101 - 700), many]), many),            # ... beside hundreds
        (anyx(2049), np.zeros(0, np.int64)),                         # no z
    ]


@pytest.mark.parametrize("bound", sorted(CASES))
def test_span_count_equals_numpy_k0_and_one_entry_items(gpu, bound):
    import torch
    from tuplewise import _lib as L
    nb, ks = CASES[bound]
    assert float(np.float32(bound)) == bound
    a = C._launch_of(torch, L, bound, _bags(np.random.RandomState(bound % 9941), bound, nb, ks))
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")

    def run():
        work.fill_(0xFF)
        return a.planes(work).cpu().numpy()
    L.call("tw_count_chain_set_swap", 0)
    for R, zc in PLANS:
        L.call("tw_count_chain_set_plan", R, zc)
        L.call("tw_count_chain_set_class_bits", 0)
        base = run()
        assert np.array_equal(base, a.want), (bound, R, zc, "k = 0")
        for k in ks:
            L.call("tw_count_chain_set_class_bits", k)
            cap = _cap(a, k, zc)
            _set_span(L, 1)
            one = run()
            assert np.array_equal(one, a.want), (bound, R, zc, k, "M = 1")
            for m in (2, 3, 5, cap, cap + 7, 0):
                _set_span(L, m)
                assert _set_span(L, -1) == m
                got = run()
                print("bound", bound, "plan", (R, zc), "k", k, "form", D._form(L, nb, k), "M", m,
                      "max |spans - numpy|", np.abs(got - a.want).max())
                assert np.array_equal(got, a.want), (bound, R, zc, k, m)
                assert np.array_equal(got, base) and np.array_equal(got, one), (bound, k, m)


def test_span_count_at_32_bags_under_every_automatic_setting(gpu):
    """32 bags under the automatic plan, swap rule, class bits and span; then forced k = 8 (the
    digit loop) with the automatic span and forced spans."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    rng = np.random.RandomState(13)
    bags = []
    for s in range(16):
        z = M._z(rng, bound, 300 + 29 * s)
        bags.append((M._x(rng, bound, 4101 + 97 * s, z), z))
    a = M._launch(torch, L, bound, bags)
    for m in (0, 1, 4):
        _set_span(L, m)
        M._check(a, torch, L, f"32 bags, M {m}", (0, 0), (-1, 8), swaps=(1,))


def test_span_count_where_the_automatic_rule_takes_long_spans(gpu):
    """128 bags of two x tiles at k = 8: 2^16 one-entry slots, enough for the automatic rule to
    give an item several entries (class_span_auto); equal to M = 1, k = 0 and NumPy."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    rng = np.random.RandomState(14)
    bags = []
    for s in range(64):
        z = M._z(rng, bound, 20 + s)
        bags.append((M._x(rng, bound, 4101 - s, z), z))
    a = M._launch(torch, L, bound, bags)
    for m in (0, 1):
        _set_span(L, m)
        # (swap 0: the x remainder a padded third group, two tiles; 1: the automatic rule)
        M._check(a, torch, L, f"128 bags, M {m}", (0, 0), (8,), swaps=(0, 1))


def test_span_count_twice_on_one_workspace_in_stream_order(gpu):
    """Two launches with different spans (and a fallback launch between them) on one workspace
    without a refill: the grid and the decode follow the launch's own span."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = P._Launch(torch, L, bound, 6), P._Launch(torch, L, bound, 7)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    L.call("tw_count_chain_set_swap", 2)
    L.call("tw_count_chain_set_class_bits", 8)
    _set_span(L, 5)
    oa = a.planes(work)
    _set_span(L, 2)
    ob = b.planes(work)
    L.call("tw_count_chain_set_class_bits", 6)
    oa6 = a.planes(work)
    L.call("tw_count_chain_set_class_bits", 8)
    _set_span(L, 1 << 20)
    ob8 = b.planes(work)
    torch.cuda.synchronize()
    for got, want in ((oa, a.want), (ob, b.want), (oa6, a.want), (ob8, b.want)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_span_control_reports_and_ignores_other_values(gpu):
    from tuplewise import _lib as L
    assert _set_span(L, -1) == 0  # automatic is the default (and what the fixture restores)
    assert _set_span(L, 7) == 0
    assert _set_span(L, -1) == 7
    for bad in (-2, -100, -2 ** 31):
        assert _set_span(L, bad) == 7
        assert _set_span(L, -1) == 7
    assert _set_span(L, 2 ** 31 - 1) == 7  # (clamped to each launch's capacity)
    assert _set_span(L, 0) == 2 ** 31 - 1
    assert _set_span(L, -1) == 0
