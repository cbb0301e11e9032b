"""The digit-table class loop (csrc/chainclass.h bits_count_class_digits) behind
tw_count_pairs_chain_planes: the run's images reach the loop digit-ready (pre-pass 2 writes them
so), the per-z chain is one VGPR-indexed instruction per digit, whole batches of four images and
the images left over take different statements, and (NB, K) pairs whose low field does not fit
the tables fall back to the masked-plane loop on the same workspace.

Bounds 2^16 - 1 (NB = 16: the digit loop at k = 4 .. 8) and 2^16 (NB = 18: k = 6 .. 8), the
bench's 1 000 000 (NB = 20: the digit loop at k = 8, the fallback at k = 6) and 2^22 (NB = 24:
fallback only).  Bags: runs of 1, 2, 3, 4, 5, 7, 8 and 9 images in one bag (every length modulo
the batch of four and the trip of eight), all z equal, z whose digits are all 0 and all 7, z at
every digit boundary (multiples of 8^j, one less, one more) with x the same values, x all at the
bound, no z; x sizes 31, 2047, 2048, 2049, 4096, 4101 (one or two groups per item, the last tile
short).  Every count equals, exactly, the NumPy integer count, the k = 0 path and the packed
kernel.  The workspace holds 0xFF before every call; two calls share one in stream order."""
import numpy as np
import pytest

import test_gpu_count_classes as C
import test_gpu_count_masked as M

P = C.P
pytestmark = pytest.mark.gpu

# bound -> (NB, class bits to force, the class bits at which the digit loop runs)
CASES = {2 ** 16 - 1: (16, (4, 5, 6, 7, 8), (4, 5, 6, 7, 8)),
         2 ** 16: (18, (6, 7, 8), (6, 7, 8)),
         1_000_000: (20, (8, 6), (8,)),
         2 ** 22: (24, (8, 6), ())}
PLANS = P.PLANS  # (2, 8), (3, 600), (4, 600), automatic: tiles of two and of three groups
RUNS = (1, 2, 3, 4, 5, 7, 8, 9)


def _form(L, nb, k):
    return int(L.lib().tw_count_chain_class_form(nb, k))


def test_the_default_build_runs_the_digit_loop_where_the_tables_fit(gpu):
    from tuplewise import _lib as L
    assert _form(L, 20, 8) == 3
    for nb in (16, 18, 20, 22, 24):
        for k in range(1, 9):
            assert _form(L, nb, k) == (3 if 4 <= nb - k <= 12 else 2), (nb, k)
    for bound, (nb, ks, digit_ks) in CASES.items():
        assert 2 ** (nb - 2) <= bound < 2 ** nb
        assert tuple(k for k in ks if _form(L, nb, k) == 3) == digit_ks


def _bags(rng, bound, nb, ks):
    """The bags of one launch (x images, z images), all images in [0, bound]."""
    shift = nb - min(ks)  # fields apart by this much are different classes at every forced k
    low = lambda n: rng.randint(0, 1 << shift, n).astype(np.int64)
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    top = lambda n: np.full(n, bound, np.int64)
    # one class per run length: fields 0 .. 7 (the highest image stays below the bound)
    runs = np.concatenate([(i << shift) + low(n) for i, n in enumerate(RUNS)])
    assert runs.max() <= bound
    # complemented digits all 7 (low bits 0) and all 0 (low bits ones), in two classes
    flat = np.array([0, (1 << 12) - 1, 1 << shift, (1 << shift) + (1 << 12) - 1,
                     min(bound, 2 ** 16 - 1)] * 3, np.int64)
    edges = np.array(sorted({min(max(m * 8 ** j + d, 0), bound)
                             for j in range(6) for m in range(1, 8) for d in (-1, 0, 1)}),
                     np.int64)
    return [
        (np.concatenate([anyx(2047 - len(runs)), runs]), runs),          # every run length
        (anyx(31), rng.permutation(runs)),
        (anyx(2048), np.full(777, bound // 3, np.int64)),                # all z equal
        (np.concatenate([anyx(2049 - len(flat)), flat]), flat),          # digits all 0 / all 7
        (np.concatenate([anyx(4096 - len(edges)), edges]), edges),       # digit boundaries, x = z
        (top(4101), np.concatenate([edges, runs])),                      # x all at the bound
        (top(2049), np.array([5, 6, 7, bound], np.int64)),
        (np.concatenate([anyx(100), [-1] * 5]), np.zeros(0, np.int64)),  # no z
        (anyx(4101), anyx(130)),
    ]


@pytest.mark.parametrize("bound", sorted(CASES))
def test_digit_count_equals_numpy_k0_and_packed(gpu, bound):
    import torch
    from tuplewise import _lib as L
    nb, ks, _ = CASES[bound]
    assert float(np.float32(bound)) == bound
    a = C._launch_of(torch, L, bound, _bags(np.random.RandomState(bound % 9949), bound, nb, ks))
    packed = a.packed().cpu().numpy()
    assert np.array_equal(packed, a.want), bound
    try:
        for plan in PLANS:
            # (M._check: 0xFF before every call; each k == NumPy == k = 0 under both swap modes)
            M._check(a, torch, L, f"bound {bound}", plan, ks + (-1,))
    finally:
        C._reset(L)


def test_digit_count_under_the_automatic_rule_at_32_bags(gpu):
    """32 bags under the automatic plan, swap rule and class bits (k = 1 at these sizes would be
    the fallback; forced k = 8 is the bench's digit loop): two groups and a short last tile."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    rng = np.random.RandomState(12)
    bags = []
    for s in range(16):
        z = M._z(rng, bound, 300 + 29 * s)
        bags.append((M._x(rng, bound, 4101 + 97 * s, z), z))
    a = M._launch(torch, L, bound, bags)
    try:
        M._check(a, torch, L, "32 bags", (0, 0), (-1, 8), swaps=(1,))
    finally:
        C._reset(L)


def test_digit_count_twice_on_one_workspace_in_stream_order(gpu):
    """The digit loop, the fallback and the digit loop again on one workspace without a refill
    in between: pre-pass 2 writes the images digit-ready or plain as the launch's form asks."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = P._Launch(torch, L, bound, 4), P._Launch(torch, L, bound, 5)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    try:
        L.call("tw_count_chain_set_swap", 2)
        L.call("tw_count_chain_set_class_bits", 8)
        oa = a.planes(work)
        ob = b.planes(work)
        L.call("tw_count_chain_set_class_bits", 6)
        oa6 = a.planes(work)
        L.call("tw_count_chain_set_class_bits", 8)
        ob8 = b.planes(work)
    finally:
        C._reset(L)
    torch.cuda.synchronize()
    for got, want in ((oa, a.want), (ob, b.want), (oa6, a.want), (ob8, b.want)):
        assert np.array_equal(got.cpu().numpy(), want)
