"""The class-run form of the plane-reading chain count (k_chain_zclasses +
k_count_chain_classes, csrc/chainclass.h) behind tw_count_pairs_chain_planes /
tw_chain_unpack_count_planes: the ragged bags of tests/test_gpu_count_planes.py (extreme images,
"never" and NaN x, heavy ties) and added z cases — all z equal, z at the class boundaries, an
odd class beside a class of one image with every x at the bound (the smallest input at which an
evaluated padded scalar slot would show), x all equal to the bound — at bounds 2^k - 1 and 2^k
around the plane counts and the bench's 1 000 000, under forced class bits {1, 2, 6, 8} and the
automatic rule and the forced plans of the planes test.  Every count equals, exactly, the NumPy
integer count, the k = 0 path (k_count_chain_planes) and the packed kernel.  The workspace holds
0xFF before every call."""
import numpy as np
import pytest

import test_gpu_count_planes as P

pytestmark = pytest.mark.gpu

T = P.T
BOUNDS = sorted({2 ** k - d for k in (16, 18, 20, 22) for d in (1, 0)} | {1_000_000})
CLASS_BITS = [1, 2, 6, 8, -1]


def _reset(L):
    L.call("tw_count_chain_set_plan", 0, 0)
    L.call("tw_count_chain_set_swap", 1)
    L.call("tw_count_chain_set_class_bits", -1)


def _launch_of(torch, L, bound, bags):
    """A P._Launch on given bags: bags[s] = (x images, -1 for "never"; z images), the same in
    both steps but for the order of the images."""
    a = object.__new__(P._Launch)
    a.torch, a.L, a.bound, a.N = torch, L, bound, len(bags)
    xs, zs = [len(b[0]) for b in bags], [len(b[1]) for b in bags]
    x_off = np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)
    z_off = np.concatenate([[0], np.cumsum(zs)]).astype(np.int64)
    xb, zb = np.zeros((T, x_off[-1]), np.float32), np.zeros((T, z_off[-1]), np.float32)
    a.want = np.zeros((T, a.N), np.int64)
    for c in range(T):
        for s, (x, z) in enumerate(bags):
            x, z = np.asarray(x, np.int64), np.asarray(z, np.int64)
            if c:
                x, z = x[::-1], z[::-1]
            xb[c, x_off[s]:x_off[s + 1]] = np.where(x < 0, np.float32(P.NEVER), x)
            zb[c, z_off[s]:z_off[s + 1]] = -z.astype(np.float32)
            a.want[c, s] = int(np.searchsorted(np.sort(z), x, side="left").sum())
    a.xd, a.zd = torch.from_numpy(xb).cuda(), torch.from_numpy(zb).cuda()
    a.xd_never = a.xd
    a.xo, a.zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    a.head = (a.xd, a.xo, xb.shape[1], a.zd, a.zo, zb.shape[1], a.N, T, max(xs), max(zs), 0)
    a.work_bytes = int(L.lib().tw_chain_planes_work_bytes(a.N, T, max(xs), max(zs), 0, bound))
    return a


def _check(a, torch, L, tag, plans=P.PLANS, swaps=(2,)):
    """a's counts under every class-bits setting and plan == NumPy == k = 0 == packed."""
    work = torch.empty(max(a.work_bytes, 256), dtype=torch.uint8, device="cuda")
    assert a.work_bytes > 0
    packed = a.packed().cpu().numpy()
    assert np.array_equal(packed, a.want), tag
    try:
        for R, zc in plans:
            L.call("tw_count_chain_set_plan", R, zc)
            for swap in swaps:
                L.call("tw_count_chain_set_swap", swap)
                L.call("tw_count_chain_set_class_bits", 0)
                work.fill_(0xFF)
                base = a.planes(work).cpu().numpy()
                assert np.array_equal(base, a.want), (tag, R, zc, swap, "k = 0")
                for k in CLASS_BITS:
                    L.call("tw_count_chain_set_class_bits", k)
                    work.fill_(0xFF)
                    got = a.planes(work).cpu().numpy()
                    print(tag, "plan", (R, zc), "swap", swap, "k", k, "max |classes - numpy|",
                          np.abs(got - a.want).max())
                    assert np.array_equal(got, a.want), (tag, R, zc, swap, k)
                    assert np.array_equal(got, base) and np.array_equal(got, packed)
    finally:
        _reset(L)


@pytest.mark.parametrize("bound", BOUNDS)
def test_classes_count_equals_numpy_k0_and_packed(gpu, bound):
    import torch
    from tuplewise import _lib as L
    assert float(np.float32(bound)) == bound
    a = P._Launch(torch, L, bound, bound % 9973)
    _check(a, torch, L, f"bound {bound}", swaps=(2, 0, 1) if bound == 1_000_000 else (2,))


@pytest.mark.parametrize("bound", [2 ** 16 - 1, 1_000_000, 2 ** 22])
def test_classes_added_z_cases(gpu, bound):
    """All z equal; z at the class boundaries of every forced k (multiples of 2^(NB - k), one
    less, one more); an odd class beside a class of one image under x all at the bound; x all
    at the bound against random z.  x sizes around a plane group, z sizes odd and even."""
    import torch
    from tuplewise import _lib as L
    rng = np.random.RandomState(bound % 977)
    nb = next(b for b in (16, 18, 20, 22, 24) if bound < 2 ** b)
    edges = np.array(sorted({min(max(c * 2 ** (nb - k) + d, 0), bound)
                             for k in (1, 2, 6, 8) for c in range(2 ** k + 1)
                             for d in (-1, 0, 1)}), np.int64)
    anyx = lambda n: rng.randint(0, bound + 1, n).astype(np.int64)
    top = lambda n: np.full(n, bound, np.int64)
    bags = [
        (anyx(2049), np.full(777, bound // 3, np.int64)),             # all z equal (odd count)
        (anyx(4101), np.full(2048, 0, np.int64)),                     # ... to 0
        (np.concatenate([anyx(1500), edges]), edges),                 # class boundaries, x = z
        (top(2048), np.array([5, 6, 7, bound], np.int64)),            # odd class + class of one
        (top(2049), np.array([bound - 1], np.int64)),                 # one z
        (top(31), np.concatenate([anyx(64), [bound // 2] * 3])),      # x all at the bound
        (top(4101), anyx(1289)),
        (np.concatenate([anyx(100), [-1] * 5]), np.zeros(0, np.int64)),  # no z
    ]
    _check(_launch_of(torch, L, bound, bags), torch, L, f"added z cases, bound {bound}")


def test_classes_two_calls_share_a_workspace_in_stream_order(gpu):
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = P._Launch(torch, L, bound, 1), P._Launch(torch, L, bound, 2)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    try:
        L.call("tw_count_chain_set_swap", 2)
        L.call("tw_count_chain_set_class_bits", 6)
        oa = a.planes(work)
        ob = b.planes(work)
        L.call("tw_count_chain_set_class_bits", 2)
        oa2 = a.planes(work)
    finally:
        _reset(L)
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), a.want)
    assert np.array_equal(ob.cpu().numpy(), b.want)
    assert np.array_equal(oa2.cpu().numpy(), a.want)


def test_classes_undersized_workspace_is_refused_before_any_launch(gpu):
    import torch
    from tuplewise import _lib as L
    a = P._Launch(torch, L, 1_000_000, 3)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    o = a.out()
    args = [L.ptr(v) if isinstance(v, torch.Tensor) else v for v in a.head]
    try:
        for k in (6, 8, -1, 0):  # the size asked for does not depend on the class bits
            L.call("tw_count_chain_set_class_bits", k)
            assert int(L.lib().tw_chain_planes_work_bytes(
                a.N, T, max(P.X_SIZES), max(P.Z_SIZES), 0, a.bound)) == a.work_bytes
            rc = L.lib().tw_count_pairs_chain_planes(*args, a.bound, L.ptr(o), L.stream_handle(),
                                                     L.ptr(work), a.work_bytes - 1)
            assert rc == L.TW_ERR_ARG
            assert b"work_bytes" in L.lib().tw_last_error()
    finally:
        _reset(L)
    torch.cuda.synchronize()
    assert int((o != 777).sum().item()) == 0  # not even zeroed
    assert int((work != 0xFF).sum().item()) == 0


def test_class_bits_setter_refuses_other_values(gpu):
    from tuplewise import _lib as L
    try:
        for k in (-2, 9, 100):
            assert L.lib().tw_count_chain_set_class_bits(k) == L.TW_ERR_ARG
        for k in (-1, 0, 1, 8):
            assert L.lib().tw_count_chain_set_class_bits(k) == 0
    finally:
        _reset(L)


@pytest.mark.parametrize("k", [6, 8])
def test_unpack_count_planes_with_classes(gpu, k):
    """tw_chain_unpack_count_planes goes through the same launcher: one world-1 receive buffer
    (the planes test's layout), counts under forced class bits == k = 0 == NumPy."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import prop_swor_layout
    rng = np.random.RandomState(7)
    n, m, N, bound = 9000, 5000, 2, 1_000_000
    x_off, z_off, _ = prop_swor_layout(n, m, N)
    kx, kz = int(n / N), int((n + m) / N) - int(n / N)
    cap = n + m
    recv = np.zeros((T, cap + 1), np.uint64)
    want = np.zeros((T, N), np.int64)
    for c in range(T):
        x, xf, z = P._images(rng, bound, n, m)
        img = np.concatenate([xf, -z.astype(np.float32)]).view(np.uint32).astype(np.uint64)
        order = rng.permutation(n + m).astype(np.uint64)
        recv[c, 0] = n + m
        recv[c, 1:] = img[order] | (order << np.uint64(32))
        for s in range(N):
            zs = np.sort(z[z_off[s]:z_off[s + 1]])
            want[c, s] = int(np.searchsorted(zs, x[x_off[s]:x_off[s + 1]], side="left").sum())
    rd = torch.from_numpy(recv.view(np.int64).reshape(-1)).cuda()
    xo, zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    max_nx, max_nz = int(np.diff(x_off).max()), int(np.diff(z_off).max())
    wb = int(L.lib().tw_chain_planes_work_bytes(N, T, max_nx, max_nz, 0, bound))
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    cur = torch.empty(T * 2 * (N + 1), dtype=torch.int32, device="cuda")

    def run(bits):
        L.call("tw_count_chain_set_class_bits", bits)
        work.fill_(0xFF)
        xbag = torch.empty((T, n), dtype=torch.float32, device="cuda")
        zbag = torch.empty((T, m), dtype=torch.float32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.full((T, N), 777, dtype=torch.int64, device="cuda")
        L.call("tw_chain_unpack_count_planes", rd, 1, T, cap, 0, n, m, kx, kz, N, xbag, zbag, cur,
               flag, xo, zo, max_nx, max_nz, bound, out, L.stream_handle(), work, wb)
        assert int(flag.item()) == 0
        return out.cpu().numpy()
    try:
        L.call("tw_count_chain_set_plan", 4, 600)
        L.call("tw_count_chain_set_swap", 2)
        base, got = run(0), run(k)
    finally:
        _reset(L)
    assert np.array_equal(base, want)
    assert np.array_equal(got, want)


def test_unn_many_with_classes_equals_k0(gpu):
    """ShardedSample.UnN_many on the chain path (strict, carried images over two calls):
    estimates and final arrays under forced class bits and the automatic rule are bit-identical
    to k = 0."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import ShardedSample
    gen = torch.Generator(device="cuda").manual_seed(9)
    n = 300_000
    X = (torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) + 0.3).round(
        decimals=3)
    Z = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen).round(decimals=3)
    calls = [range(3, 7), range(10, 14)]

    def run(bits):
        L.call("tw_count_chain_set_class_bits", bits)
        S = ShardedSample(X.clone(), Z.clone(), 16, tie_mode="strict", algo="pairs")
        assert S._chain_ok()
        out = []
        for i, ks in enumerate(calls):
            assert (S._carried(False) is not None) == (i > 0)
            out.append(([float(v) for v in S.UnN_many(ks)], S.X.cpu().numpy(),
                        S.Z.cpu().numpy()))
        return out
    try:
        want = run(0)
        for bits in (6, -1):
            got = run(bits)
            for (gv, gx, gz), (wv, wx, wz) in zip(got, want):
                assert gv == wv, bits
                assert np.array_equal(gx, wx) and np.array_equal(gz, wz), bits
    finally:
        _reset(L)
