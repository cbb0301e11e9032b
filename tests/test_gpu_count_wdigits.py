"""The wide-digit class loop (csrc/chainclass.h bits_count_span_wide) behind
tw_count_pairs_chain_planes: where NB - K = 12 the low field is read as three digits of four
planes — tables of 16 (+ 1) entries in pinned VGPRs, pre-pass 2 writing the images with
class_wide_encode — under tw_count_chain_class_digits 4 (and the automatic rule), and as four
digits of three planes under 3; the K top planes and the top digit's planes are reloaded per
class inside a span.

Bounds and class bits: 2^16 - 1 (NB = 16, k = 4), 2^16 (NB = 18, k = 6) and the bench's
1 000 000 (NB = 20, k = 8).  Settings: hook 4, hook 3 and automatic, under the plans (2, 8),
(3, 600) and automatic, spans forced to 1 and to 8.  Bags: runs of 1, 2, 3, 4, 5, 7, 8 and 9
images in eight consecutive classes (a span crosses class changes and takes the reload path;
every length modulo the batch of four and the trip of eight), all z equal, z whose complemented
digits are all 0 and all 15, z at every 16^j boundary (m 16^j, one less, one more) with x the
same values, x all at the bound, no z; x sizes 31, 2047, 2048, 2049, 4096 and 4101.  Every count
equals, exactly, the NumPy integer count, the k = 0 path and the packed kernel.  The workspace
holds 0xFF before every call; one test runs 4, 3, 4 on one workspace in stream order."""
import numpy as np
import pytest

import test_gpu_count_classes as C
import test_gpu_count_masked as M

P = C.P
pytestmark = pytest.mark.gpu

CASES = {2 ** 16 - 1: (16, 4), 2 ** 16: (18, 6), 1_000_000: (20, 8)}  # bound -> (NB, k)
PLANS = [(2, 8), (3, 600), (0, 0)]
SETTINGS = (4, 3, 0)
SPANS = (1, 8)
RUNS = (1, 2, 3, 4, 5, 7, 8, 9)


def _digits(L, w):
    return int(L.lib().tw_count_chain_class_digits(w))


def _digits_of(L, nb, k):
    return int(L.lib().tw_count_chain_class_digits_of(nb, k))


def _reset(L):
    C._reset(L)
    L.lib().tw_count_chain_class_span(0)
    assert _digits(L, 0) in (0, 3, 4)


def _bags(rng, bound):
    """The bags of one launch (x images, z images), all images in [0, bound]; the class of an
    image under the case's k is its bits from 12 up."""
    low = lambda n: rng.randint(0, 1 << 12, n).astype(np.int64)
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    top = lambda n: np.full(n, bound, np.int64)
    # one class per run length: eight consecutive classes
    runs = np.concatenate([(i << 12) + low(n) for i, n in enumerate(RUNS)])
    assert runs.max() <= bound
    # complemented digits all 15 (low bits 0) and all 0 (low bits ones), in two classes
    flat = np.array([0, (1 << 12) - 1, 1 << 12, (1 << 12) + (1 << 12) - 1,
                     min(bound, 2 ** 16 - 1)] * 3, np.int64)
    edges = np.array(sorted({min(max(m * 16 ** j + d, 0), bound)
                             for j in range(5) for m in range(1, 16) for d in (-1, 0, 1)}),
                     np.int64)
    return [
        (np.concatenate([anyx(2047 - len(runs)), runs]), runs),          # every run length
        (anyx(31), rng.permutation(runs)),
        (anyx(2048), np.full(777, bound // 3, np.int64)),                # all z equal
        (np.concatenate([anyx(2049 - len(flat)), flat]), flat),          # digits all 0 / all 15
        (np.concatenate([anyx(4096 - len(edges)), edges]), edges),       # digit boundaries, x = z
        (top(4101), np.concatenate([edges, runs])),                      # x all at the bound
        (top(2049), np.array([5, 6, 7, bound], np.int64)),
        (np.concatenate([anyx(100), [-1] * 5]), np.zeros(0, np.int64)),  # no z
        (anyx(4101), anyx(130)),
    ]


@pytest.mark.parametrize("bound", sorted(CASES))
def test_wide_count_equals_numpy_k0_and_packed(gpu, bound):
    import torch
    from tuplewise import _lib as L
    nb, k = CASES[bound]
    assert float(np.float32(bound)) == bound and 2 ** (nb - 2) <= bound < 2 ** nb
    assert int(L.lib().tw_count_chain_class_form(nb, k)) == 3
    a = C._launch_of(torch, L, bound, _bags(np.random.RandomState(bound % 9941), bound))
    packed = a.packed().cpu().numpy()
    assert np.array_equal(packed, a.want), bound
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    try:
        L.call("tw_count_chain_set_swap", 2)
        for plan in PLANS:
            L.call("tw_count_chain_set_plan", *plan)
            L.call("tw_count_chain_set_class_bits", 0)
            work.fill_(0xFF)
            base = a.planes(work).cpu().numpy()
            assert np.array_equal(base, a.want), (bound, plan, "k = 0")
            L.call("tw_count_chain_set_class_bits", k)
            for w in SETTINGS:
                _digits(L, w)
                assert _digits_of(L, nb, k) == (w if w else _digits_of(L, nb, k))
                for span in SPANS:
                    L.lib().tw_count_chain_class_span(span)
                    work.fill_(0xFF)
                    got = a.planes(work).cpu().numpy()
                    print("bound", bound, "plan", plan, "digits", w, "span", span,
                          "max |wide - numpy|", np.abs(got - a.want).max())
                    assert np.array_equal(got, a.want), (bound, plan, w, span)
                    assert np.array_equal(got, base) and np.array_equal(got, packed)
    finally:
        _reset(L)


def test_wide_count_at_32_bags_under_the_automatic_plan(gpu):
    """32 bags under the automatic plan, swap rule and span, class bits 8 and automatic: two
    groups and a short last tile, each setting of the hook."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    rng = np.random.RandomState(14)
    bags = []
    for s in range(16):
        z = M._z(rng, bound, 300 + 29 * s)
        bags.append((M._x(rng, bound, 4101 + 97 * s, z), z))
    a = M._launch(torch, L, bound, bags)
    try:
        for w in SETTINGS:
            _digits(L, w)
            M._check(a, torch, L, f"32 bags, digits {w}", (0, 0), (-1, 8), swaps=(1,))
    finally:
        _reset(L)


def test_wide_four_wide_on_one_workspace_in_stream_order(gpu):
    """The wide loop, the four-digit loop and the wide loop again on one workspace without a
    refill in between: every launch re-encodes its z region for the loop it runs."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = P._Launch(torch, L, bound, 6), P._Launch(torch, L, bound, 7)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    try:
        L.call("tw_count_chain_set_swap", 2)
        L.call("tw_count_chain_set_class_bits", 8)
        _digits(L, 4)
        oa = a.planes(work)
        ob = b.planes(work)
        _digits(L, 3)
        oa3 = a.planes(work)
        _digits(L, 4)
        ob4 = b.planes(work)
    finally:
        _reset(L)
    torch.cuda.synchronize()
    for got, want in ((oa, a.want), (ob, b.want), (oa3, a.want), (ob4, b.want)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_digits_hook_and_query(gpu):
    """tw_count_chain_class_digits returns the setting before the call, -1 only reports, other
    values are refused and change nothing; the query answers 4 exactly where NB - K = 12 under
    4, and 3 everywhere under 3."""
    from tuplewise import _lib as L
    before = _digits(L, -1)
    assert before == 0  # (the automatic rule, unless another test left a setting behind)
    try:
        assert _digits(L, 4) == before
        assert _digits(L, -1) == 4
        for nb in (16, 18, 20, 22, 24):
            for k in range(0, 9):
                assert _digits_of(L, nb, k) == (4 if k > 0 and nb - k == 12 else 3), (nb, k)
        for bad in (-2, 1, 2, 5, 12):
            assert _digits(L, bad) == L.TW_ERR_ARG
            assert b"tw_count_chain_class_digits" in L.lib().tw_last_error()
            assert _digits(L, -1) == 4
        assert _digits(L, 3) == 4
        for nb in (16, 18, 20, 22, 24):
            for k in range(0, 9):
                assert _digits_of(L, nb, k) == 3, (nb, k)
        assert _digits(L, 0) == 3
        auto = {(nb, k): _digits_of(L, nb, k) for nb in (16, 18, 20) for k in range(1, 9)}
        assert all(v == 3 for (nb, k), v in auto.items() if nb - k != 12)
        assert len({auto[16, 4], auto[18, 6], auto[20, 8]}) == 1  # one rule for the wide shapes
    finally:
        assert _digits(L, before) in (0, 3, 4)
    assert _digits(L, -1) == before
