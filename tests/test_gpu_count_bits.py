"""The bit-sliced chain count as HipOps issues it under bounded_images:
tw_count_pairs_chain_planes / tw_chain_unpack_count_planes, that is the pre-pass k_chain_planes
and k_count_chain_planes (launches this small run without class bits under the automatic rule),
or the packed k_count_chain where the automatic plan keeps a launch on it.  On bags built
directly (ragged x and z tails, empty bags, sub-wave tiles, z bags shorter and longer than a
chunk, heavy ties, the extreme images 0 and bound, "never" x images) its counts equal the packed
kernel's (tw_count_pairs_chain) and a NumPy integer count, exactly, at every plane-count
boundary and under every forced plan (R in {2, 4} plane groups, z chunks of 8 and 600)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 3
X_SIZES = [0, 1, 63, 2049, 4100, 8193]
Z_SIZES = [5, 0, 1, 7, 1025, 2051]
NEVER = -float(2 ** 25)
# 2^k - 1 and 2^k around each instantiated plane count (16, 18, 20, 22, 24), and the bench's
BOUNDS = sorted({2 ** k - d for k in (16, 18, 20, 22, 24) for d in (1, 0)} | {1_000_000})
PLANS = [(2, 8), (2, 600), (4, 8), (4, 600)]


def _images(rng, bound, nx, nz):
    """x images and z images (not yet negated) of one bag: integers in [0, bound] drawn half
    from a small common pool (ties), with exact 0, exact bound and "never" x images."""
    pool = np.unique(np.concatenate([rng.randint(0, bound + 1, 6), [0, bound, bound // 2]]))
    def draw(k):
        v = rng.randint(0, bound + 1, k).astype(np.int64)
        tie = rng.rand(k) < 0.5
        v[tie] = pool[rng.randint(0, len(pool), int(tie.sum()))]
        return v
    x, z = draw(nx), draw(nz)
    xf = x.astype(np.float32)
    if nx > 4:
        x[:2], xf[:2] = [0, bound], [0.0, float(bound)]
        xf[2::37] = NEVER
        x[2::37] = -1  # greater than no z
    if nz > 2:
        z[0], z[1] = bound, 0
    return x, xf, z


def _reference(rng, bound):
    """The bags [T][sum sizes] as the kernels read them, and the NumPy counts [T][shards]."""
    x_off = np.concatenate([[0], np.cumsum(X_SIZES)]).astype(np.int64)
    z_off = np.concatenate([[0], np.cumsum(Z_SIZES)]).astype(np.int64)
    xb = np.zeros((T, x_off[-1]), np.float32)
    zb = np.zeros((T, z_off[-1]), np.float32)
    want = np.zeros((T, len(X_SIZES)), np.int64)
    for c in range(T):
        for s, (nx, nz) in enumerate(zip(X_SIZES, Z_SIZES)):
            x, xf, z = _images(rng, bound, nx, nz)
            xb[c, x_off[s]:x_off[s + 1]] = xf
            zb[c, z_off[s]:z_off[s + 1]] = -z.astype(np.float32)
            want[c, s] = int(np.searchsorted(np.sort(z), x, side="left").sum())  # #{z < x}
    return x_off, z_off, xb, zb, want


@pytest.mark.parametrize("bound", BOUNDS)
def test_bound_count_equals_packed_and_numpy(gpu, bound):
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    assert float(np.float32(bound)) == bound  # the images are exact in f32
    x_off, z_off, xb, zb, want = _reference(np.random.RandomState(bound % 9973), bound)
    ops = HipOps()
    N = len(X_SIZES)
    xd, zd = torch.from_numpy(xb).cuda(), torch.from_numpy(zb).cuda()
    xo, zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    args = (xd, xo, zd, zo, N, T, xb.shape[1], zb.shape[1], max(X_SIZES), max(Z_SIZES), False)

    def run(with_bound):
        out = torch.full((T, N), 777, dtype=torch.int64, device="cuda")
        if with_bound:
            with ops.bounded_images(bound):
                ops.count_chain(*args, out)
        else:
            ops.count_chain(*args, out)
        return out.cpu().numpy()
    packed = run(False)
    print("bound", bound, "packed == numpy:", np.array_equal(packed, want))
    assert np.array_equal(packed, want)
    try:
        for R, zc in PLANS:
            L.call("tw_count_chain_set_plan", R, zc)
            got = run(True)
            print("bound", bound, "R", R, "z chunk", zc, "max |diff|", np.abs(got - want).max())
            assert np.array_equal(got, want), (R, zc)
    finally:
        L.call("tw_count_chain_set_plan", 0, 0)
    assert np.array_equal(run(True), want)  # the automatic plan (either kernel)


@pytest.mark.parametrize("plan", [(0, 0), (2, 8), (4, 600)])
def test_unpack_count_bound_equals_unpack_count(gpu, plan):
    """One world-1 receive buffer (tw_chain_emit's exchange layout: per step a count slot, then
    {image | local position << 32} records): HipOps.chain_unpack_count under bounded_images
    (tw_chain_unpack_count_planes) == tw_chain_unpack_count == NumPy on the prop-SWOR shard
    regions."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps, prop_swor_layout
    rng = np.random.RandomState(5)
    n, m, N, bound = 9000, 5000, 2, 1_000_000
    x_off, z_off, _ = prop_swor_layout(n, m, N)
    kx, kz = int(n / N), int((n + m) / N) - int(n / N)
    cap = n + m
    recv = np.zeros((T, cap + 1), np.uint64)
    want = np.zeros((T, N), np.int64)
    for c in range(T):
        x, xf, z = _images(rng, bound, n, m)
        img = np.concatenate([xf, -z.astype(np.float32)]).view(np.uint32).astype(np.uint64)
        order = rng.permutation(n + m).astype(np.uint64)  # records arrive in any order
        recv[c, 0] = n + m
        recv[c, 1:] = img[order] | (order << np.uint64(32))
        for s in range(N):
            zs = np.sort(z[z_off[s]:z_off[s + 1]])
            want[c, s] = int(np.searchsorted(zs, x[x_off[s]:x_off[s + 1]], side="left").sum())
    ops = HipOps()
    rd = torch.from_numpy(recv.view(np.int64).reshape(-1)).cuda()
    xo, zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    max_nx, max_nz = int(np.diff(x_off).max()), int(np.diff(z_off).max())

    def run(with_bound):
        xbag = torch.empty((T, n), dtype=torch.float32, device="cuda")
        zbag = torch.empty((T, m), dtype=torch.float32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.full((T, N), 777, dtype=torch.int64, device="cuda")
        a = (rd, 1, T, cap, False, n, m, xbag, zbag, flag, kx, kz, N, xo, zo, max_nx, max_nz, out)
        if with_bound:
            with ops.bounded_images(bound):
                ops.chain_unpack_count(*a)
        else:
            ops.chain_unpack_count(*a)
        assert int(flag.item()) == 0
        return out.cpu().numpy()
    assert np.array_equal(run(False), want)
    try:
        L.call("tw_count_chain_set_plan", *plan)
        got = run(True)
    finally:
        L.call("tw_count_chain_set_plan", 0, 0)
    assert np.array_equal(got, want)
