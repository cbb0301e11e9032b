"""The LDS-table form of the class count (csrc/chain.hip k_count_chain_classes_lds,
csrc/chainclass.h bits_count_runs_lds) behind tw_count_pairs_chain_planes: where a
launch would run the wide digits (NB - K = 12), one block of 16 waves per (bag, x tile of two
groups) tabulates the carries of the low 8 planes in LDS, its waves draw the bag's runs from an
LDS counter and pre-pass 2 writes the images with class_lds_encode.

Bounds and class bits: 2^16 - 1 (NB = 16, k = 4), 2^16 (NB = 18, k = 6) and the bench's
1 000 000 (NB = 20, k = 8): the three instantiations.  Every case is counted under
tw_count_chain_class_lds 2, 1 and 0 with plans and class bits forced so that small bags take the
form (two groups per tile, never swapped); under 2 tw_count_chain_class_lds_of must answer 1.
Bags: runs of 1, 2, 3, 4, 5, 7, 8, 9, 11, 12 and 13 images in consecutive classes (every length
modulo the batch of four and around the trip of eight with its read-ahead); 5, 16, 17 and 40
runs in a bag (idle waves, one run each, several runs per wave); all z equal under a z chunk of
8 (one class cut into many runs: several waves rebuild the same class); z whose complemented low
12 bits are all 0 and all ones; z at every 16^j boundary with x the same values; x all at the
bound; a class of three z and a class of one under 2048 x at the bound; x sizes 31, 2047, 2048,
2049 (a second group of one image), 4096, 4097 (a second tile of one group) and 4101; a bag with
a single z and a bag with a single x in a ragged 3-shard x 2-step launch, and a 1 x 1 launch.
Every count equals, exactly, NumPy's searchsorted count, the k = 0 path and the packed kernel.
The workspace holds 0xFF and the output 777 before every call; one test runs 2, 1, 2 and the
four-digit loop on one workspace in stream order."""
import numpy as np
import pytest

import test_gpu_count_classes as C
import test_gpu_count_wdigits as W

P = C.P
pytestmark = pytest.mark.gpu

CASES = W.CASES  # bound -> (NB, k)
MODES = (2, 1, 0)
PLANS = [(2, 600), (2, 8)]  # two groups per tile; runs of whole classes / runs of <= 8 images
RUNS = (1, 2, 3, 4, 5, 7, 8, 9, 11, 12, 13)
RUN_COUNTS = (5, 16, 17, 40)


def _lds(L, mode):
    return int(L.lib().tw_count_chain_class_lds(mode))


def _lds_of(L, a, steps=P.T):
    return int(L.lib().tw_count_chain_class_lds_of(a.N, steps, a.head[8], a.head[9], a.bound))


def _reset(L):
    W._reset(L)
    assert _lds(L, 0) in (0, 1, 2)


def _runs_bag(rng, bound, r):
    """z images that make exactly r runs under a z chunk of 8: single runs of 8 images in
    distinct classes and, where r exceeds the classes, one class of 8 j images (j runs)."""
    m = min(r, bound >> 12)
    sizes = [8 * (r - m + 1)] + [8] * (m - 1)
    z = np.concatenate([(i << 12) + rng.randint(0, 1 << 12, n) for i, n in enumerate(sizes)])
    assert z.max() <= bound and sum(-(-n // 8) for n in sizes) == r
    return rng.permutation(z.astype(np.int64))


def _bags(rng, bound):
    low = lambda n: rng.randint(0, 1 << 12, n).astype(np.int64)
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    top = lambda n: np.full(n, bound, np.int64)
    runs = np.concatenate([(i << 12) + low(n) for i, n in enumerate(RUNS)])  # a class per length
    assert runs.max() <= bound
    # complemented low 12 bits all ones (low bits 0) and all 0 (low bits ones), in two classes
    flat = np.array([0, (1 << 12) - 1, 1 << 12, (1 << 12) + (1 << 12) - 1,
                     min(bound, 2 ** 16 - 1)] * 3, np.int64)
    edges = np.array(sorted({min(max(m * 16 ** j + d, 0), bound)
                             for j in range(5) for m in range(1, 16) for d in (-1, 0, 1)}),
                     np.int64)
    sizes = iter((2048, 2049, 4096, 4097))
    return [
        (np.concatenate([anyx(2047 - len(runs)), runs]), runs),          # every run length
        (anyx(31), rng.permutation(runs)),
        *[(anyx(next(sizes)), _runs_bag(rng, bound, r)) for r in RUN_COUNTS],
        (anyx(4101), np.full(777, bound // 3, np.int64)),                # all z equal
        (np.concatenate([anyx(2049 - len(flat)), flat]), flat),          # low bits all 0 / all 1
        (np.concatenate([anyx(4096 - len(edges)), edges]), edges),       # digit boundaries, x = z
        (top(4101), np.concatenate([edges, runs])),                      # x all at the bound
        (top(2048), np.array([5, 6, 7, bound], np.int64)),               # three z + one z
    ]


def _count_all_modes(torch, L, a, k, tag, steps=P.T):
    """a's launch under every plan and mode == NumPy == k = 0 == packed (rows below steps)."""
    want = a.want[:steps]
    head = a.head[:7] + (steps,) + a.head[8:]

    def planes(work):
        o = a.out()
        L.call("tw_count_pairs_chain_planes", *head, a.bound, o, L.stream_handle(), work,
               a.work_bytes)
        o = o.cpu().numpy()
        assert (o[steps:] == 777).all()  # (rows past the launch's steps are not touched)
        return o[:steps]

    packed = a.packed().cpu().numpy()[:steps]
    assert np.array_equal(packed, want), tag
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    L.call("tw_count_chain_set_swap", 0)
    for plan in PLANS:
        L.call("tw_count_chain_set_plan", *plan)
        L.call("tw_count_chain_set_class_bits", 0)
        work.fill_(0xFF)
        base = planes(work)
        assert np.array_equal(base, want), (tag, plan, "k = 0")
        L.call("tw_count_chain_set_class_bits", k)
        for mode in MODES:
            _lds(L, mode)
            if mode == 2:
                assert _lds_of(L, a, steps) == 1, (tag, plan)  # no silent fall-back
            if mode == 1:
                assert _lds_of(L, a, steps) == 0, (tag, plan)
            work.fill_(0xFF)
            got = planes(work)
            print(tag, "plan", plan, "lds", mode, "runs the form", _lds_of(L, a, steps),
                  "max |lds - numpy|", np.abs(got - want).max())
            assert np.array_equal(got, want), (tag, plan, mode)
            assert np.array_equal(got, base) and np.array_equal(got, packed)


@pytest.mark.parametrize("bound", sorted(CASES))
def test_lds_count_equals_numpy_k0_and_packed(gpu, bound):
    import torch
    from tuplewise import _lib as L
    nb, k = CASES[bound]
    assert float(np.float32(bound)) == bound and 2 ** (nb - 2) <= bound < 2 ** nb
    assert int(L.lib().tw_count_chain_class_digits_of(nb, k)) == 4
    a = C._launch_of(torch, L, bound, _bags(np.random.RandomState(bound % 9949), bound))
    try:
        _count_all_modes(torch, L, a, k, f"bound {bound}")
    finally:
        _reset(L)


@pytest.mark.parametrize("bound", sorted(CASES))
def test_lds_count_single_images_ragged_and_one_bag(gpu, bound):
    """A bag with a single z and a bag with a single x in a ragged 3-shard x 2-step launch, and a
    1 x 1 launch (one shard, one step) of a bag of two tiles."""
    import torch
    from tuplewise import _lib as L
    nb, k = CASES[bound]
    rng = np.random.RandomState(bound % 9931)
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    ragged = C._launch_of(torch, L, bound, [(anyx(4101), np.array([bound // 2], np.int64)),
                                            (np.array([bound // 2 + 1], np.int64), anyx(130)),
                                            (anyx(2049), anyx(65))])
    one = C._launch_of(torch, L, bound, [(anyx(4097), anyx(257))])
    try:
        _count_all_modes(torch, L, ragged, k, f"ragged, bound {bound}")
        _count_all_modes(torch, L, one, k, f"1 x 1, bound {bound}", steps=1)
    finally:
        _reset(L)


def test_lds_wide_lds_four_on_one_workspace_in_stream_order(gpu):
    """The table form, the wide loop, the table form again and the four-digit loop on one
    workspace without a refill in between: every launch re-encodes its z region."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = P._Launch(torch, L, bound, 6), P._Launch(torch, L, bound, 7)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    try:
        L.call("tw_count_chain_set_plan", 2, 600)
        L.call("tw_count_chain_set_swap", 0)
        L.call("tw_count_chain_set_class_bits", 8)
        _lds(L, 2)
        assert _lds_of(L, a) == 1 and _lds_of(L, b) == 1
        oa = a.planes(work)
        _lds(L, 1)
        ob = b.planes(work)
        _lds(L, 2)
        oa2 = a.planes(work)
        W._digits(L, 3)
        assert _lds_of(L, b) == 0  # (forced four digits keep meaning the four-digit loop)
        ob3 = b.planes(work)
    finally:
        _reset(L)
    torch.cuda.synchronize()
    for got, want in ((oa, a.want), (ob, b.want), (oa2, a.want), (ob3, b.want)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_lds_hook_and_query(gpu):
    """tw_count_chain_class_lds returns the setting before the call, -1 only reports, other
    values are refused and change nothing; the query answers 1 only where the wide loop would
    run with two groups per tile and no swapped items, and never under 1; the span hook keeps
    its return values."""
    from tuplewise import _lib as L
    before = _lds(L, -1)
    assert before == 0  # (the automatic rule, unless another test left a setting behind)
    of = lambda nx=4101, nz=700, bound=1_000_000: int(
        L.lib().tw_count_chain_class_lds_of(3, 2, nx, nz, bound))
    try:
        assert _lds(L, 2) == before and _lds(L, -1) == 2
        for bad in (-2, 3, 4, 100):
            assert _lds(L, bad) == L.TW_ERR_ARG
            assert b"tw_count_chain_class_lds" in L.lib().tw_last_error()
            assert _lds(L, -1) == 2
        L.call("tw_count_chain_set_plan", 2, 600)
        L.call("tw_count_chain_set_swap", 0)
        L.call("tw_count_chain_set_class_bits", 8)
        assert of() == 1
        assert int(L.lib().tw_count_chain_class_span(3)) == 0
        assert int(L.lib().tw_count_chain_class_span(-1)) == 3 and of() == 1
        assert int(L.lib().tw_count_chain_class_span(0)) == 3
        assert of(bound=2 ** 22) == 0            # NB = 24: no 12-plane low field at k = 8
        L.call("tw_count_chain_set_class_bits", 6)
        assert of() == 0 and of(bound=2 ** 16) == 1
        L.call("tw_count_chain_set_class_bits", 0)
        assert of() == 0                          # no classes
        L.call("tw_count_chain_set_class_bits", 8)
        L.call("tw_count_chain_set_swap", 2)
        assert of() == 0                          # swapped items planned
        L.call("tw_count_chain_set_swap", 0)
        W._digits(L, 3)
        assert of() == 0                          # four digits forced
        W._digits(L, 0)
        assert _lds(L, 1) == 2 and of() == 0
        assert _lds(L, 0) == 1
        assert of(0, 5) == 0 and of(5, 0) == 0
    finally:
        _reset(L)
    assert _lds(L, -1) == before
