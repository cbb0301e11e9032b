"""The chain count on bit planes built once per bag (k_chain_planes + k_count_chain_planes,
DESIGN §4.1f) behind tw_count_pairs_chain_planes / tw_chain_unpack_count_planes: ragged bags in
one launch (empty, sub-wave, one image short of a plane group, exactly one, one more, several
groups with a remainder, the bench's 15625; z bags shorter and longer than a group and a chunk)
with heavy ties, the extreme images 0 and bound, "never" x images — counts equal, exactly, a
NumPy integer count and the packed kernel (tw_count_pairs_chain), at every plane-count boundary
and under the forced plans (2, 8), (3, 600), (4, 600) and the automatic one.  The workspace holds 0xFF before
every call: a plane word read without having been written would count every pair."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T = 2
X_SIZES = [0, 1, 31, 2047, 2048, 2049, 4101, 15625]
Z_SIZES = [1, 63, 64, 65, 2047, 2049, 15625, 0]
NEVER = -float(2 ** 25)
# 2^k - 1 and 2^k around each instantiated plane count (16, 18, 20, 22, 24), and the bench's
BOUNDS = sorted({2 ** k - d for k in (16, 18, 20, 22, 24) for d in (1, 0)} | {1_000_000})
PLANS = [(2, 8), (3, 600), (4, 600), (0, 0)]


def _images(rng, bound, nx, nz):
    """x images and z images (not yet negated) of one bag: integers in [0, bound] drawn half
    from a small common pool (ties), with exact 0, exact bound, "never" and NaN x images."""
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
        xf[3::41] = np.nan
        x[2::37] = -1  # greater than no z
        x[3::41] = -1
    if nz > 2:
        z[0], z[1] = bound, 0
    return x, xf, z


def _bags(seed, bound):
    """The bags [T][sum sizes] as the kernels read them, and the NumPy counts [T][shards]."""
    rng = np.random.RandomState(seed)
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


class _Launch:
    """One set of bags on the device and the two entry points on them."""

    def __init__(self, torch, L, bound, seed):
        self.torch, self.L, self.bound = torch, L, bound
        x_off, z_off, xb, zb, self.want = _bags(seed, bound)
        self.N = len(X_SIZES)
        self.xd, self.zd = torch.from_numpy(xb).cuda(), torch.from_numpy(zb).cuda()
        self.xo, self.zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
        self.head = (self.xd, self.xo, xb.shape[1], self.zd, self.zo, zb.shape[1], self.N, T,
                     max(X_SIZES), max(Z_SIZES), 0)
        # (the packed kernel's contract writes a NaN x as the "never" image; the bit-sliced
        # conversions take either)
        self.xd_never = torch.from_numpy(np.where(np.isnan(xb), np.float32(NEVER), xb)).cuda()
        self.work_bytes = int(L.lib().tw_chain_planes_work_bytes(
            self.N, T, max(X_SIZES), max(Z_SIZES), 0, bound))

    def out(self):
        return self.torch.full((T, self.N), 777, dtype=self.torch.int64, device="cuda")

    def packed(self):
        o = self.out()
        self.L.call("tw_count_pairs_chain", self.xd_never, *self.head[1:], o,
                    self.L.stream_handle())
        return o

    def planes(self, work, work_bytes=None):
        o = self.out()
        self.L.call("tw_count_pairs_chain_planes", *self.head, self.bound, o,
                    self.L.stream_handle(), work,
                    self.work_bytes if work_bytes is None else work_bytes)
        return o


@pytest.mark.parametrize("bound", BOUNDS)
def test_planes_count_equals_numpy_and_packed(gpu, bound):
    import torch
    from tuplewise import _lib as L
    assert float(np.float32(bound)) == bound  # the images are exact in f32
    a = _Launch(torch, L, bound, bound % 9973)
    sliced = bound < 2 ** 24  # (2^24 itself needs a 25th plane: the packed kernel, no workspace)
    assert (a.work_bytes > 0) == sliced
    work = torch.empty(max(a.work_bytes, 256), dtype=torch.uint8, device="cuda")
    packed = a.packed().cpu().numpy()
    print("bound", bound, "packed == numpy:", np.array_equal(packed, a.want))
    assert np.array_equal(packed, a.want)
    try:
        for R, zc in PLANS:
            L.call("tw_count_chain_set_plan", R, zc)
            # the x remainders swapped wherever the per-bag rule allows (2), never (0), and as
            # the automatic plan decides for a launch this small (1)
            for swap in (2, 0, 1):
                L.call("tw_count_chain_set_swap", swap)
                work.fill_(0xFF)
                got = a.planes(work).cpu().numpy()
                print("bound", bound, "plan", (R, zc), "swap", swap, "max |planes - numpy|",
                      np.abs(got - a.want).max())
                assert np.array_equal(got, a.want), (R, zc, swap)
                assert (int((work != 0xFF).sum().item()) > 0) == sliced, "the pre-pass's planes"
    finally:
        L.call("tw_count_chain_set_plan", 0, 0)
        L.call("tw_count_chain_set_swap", 1)


def test_two_calls_share_a_workspace_in_stream_order(gpu):
    """Two launches back to back on one stream, different bags, one workspace: the second
    pre-pass overwrites the first's planes only after the first count has read them."""
    import torch
    from tuplewise import _lib as L
    bound = 1_000_000
    a, b = _Launch(torch, L, bound, 1), _Launch(torch, L, bound, 2)
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    try:
        L.call("tw_count_chain_set_swap", 2)  # (x and z planes both in use)
        oa = a.planes(work)
        ob = b.planes(work)
        oa2 = a.planes(work)
    finally:
        L.call("tw_count_chain_set_swap", 1)
    torch.cuda.synchronize()
    assert np.array_equal(oa.cpu().numpy(), a.want)
    assert np.array_equal(ob.cpu().numpy(), b.want)
    assert np.array_equal(oa2.cpu().numpy(), a.want)


def test_undersized_workspace_is_refused_before_any_launch(gpu):
    import torch
    from tuplewise import _lib as L
    a = _Launch(torch, L, 1_000_000, 3)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    o = a.out()
    rc = L.lib().tw_count_pairs_chain_planes(
        *[L.ptr(v) if isinstance(v, torch.Tensor) else v for v in a.head], a.bound, L.ptr(o),
        L.stream_handle(), L.ptr(work), a.work_bytes - 1)
    assert rc == L.TW_ERR_ARG
    assert b"work_bytes" in L.lib().tw_last_error()
    rc = L.lib().tw_count_pairs_chain_planes(
        *[L.ptr(v) if isinstance(v, torch.Tensor) else v for v in a.head], a.bound, L.ptr(o),
        L.stream_handle(), None, a.work_bytes)
    assert rc == L.TW_ERR_ARG
    torch.cuda.synchronize()
    assert int((o != 777).sum().item()) == 0  # not even zeroed
    assert int((work != 0xFF).sum().item()) == 0
    with pytest.raises(ValueError, match="work_bytes"):
        a.planes(work, 0)


@pytest.mark.parametrize("plan", PLANS)
def test_unpack_count_planes_equals_unpack_count(gpu, plan):
    """One world-1 receive buffer (tw_chain_emit's exchange layout: per step a count slot, then
    {image | local position << 32} records): tw_chain_unpack_count_planes ==
    tw_chain_unpack_count == NumPy on the prop-SWOR shard regions (shards of 4500 x and 2500 z: two full groups and a swapped remainder)."""
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
    wb = int(L.lib().tw_chain_planes_work_bytes(N, T, max_nx, max_nz, 0, bound))
    assert wb > 0
    work = torch.empty(wb, dtype=torch.uint8, device="cuda")
    cur = torch.empty(T * 2 * (N + 1), dtype=torch.int32, device="cuda")

    def run(entry, *tail):
        xbag = torch.empty((T, n), dtype=torch.float32, device="cuda")
        zbag = torch.empty((T, m), dtype=torch.float32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.full((T, N), 777, dtype=torch.int64, device="cuda")
        st = L.stream_handle()
        L.call(entry, rd, 1, T, cap, 0, n, m, kx, kz, N, xbag, zbag, cur, flag, xo, zo, max_nx,
               max_nz, *[out if v is Ellipsis else st if v is None else v for v in tail])
        assert int(flag.item()) == 0
        return out.cpu().numpy()
    assert np.array_equal(run("tw_chain_unpack_count", ..., None), want)
    try:
        L.call("tw_count_chain_set_plan", *plan)
        L.call("tw_count_chain_set_swap", 2)
        work.fill_(0xFF)
        got = run("tw_chain_unpack_count_planes", bound, ..., None, work, wb)
        if plan != (0, 0):  # (the automatic plan keeps bags this small on the packed kernel)
            assert int((work != 0xFF).sum().item()) > 0, "the pre-pass wrote no planes"
        work.fill_(0xFF)
        xbag = torch.empty((T, n), dtype=torch.float32, device="cuda")
        zbag = torch.empty((T, m), dtype=torch.float32, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        out = torch.full((T, N), 777, dtype=torch.int64, device="cuda")
        with ops.bounded_images(bound):  # HipOps routes a bounded strict count to the planes
            ops.chain_unpack_count(rd, 1, T, cap, False, n, m, xbag, zbag, flag, kx, kz, N, xo,
                                   zo, max_nx, max_nz, out)
        routed = out.cpu().numpy()
    finally:
        L.call("tw_count_chain_set_plan", 0, 0)
        L.call("tw_count_chain_set_swap", 1)
    print("plan", plan, "max |planes - numpy|", np.abs(got - want).max())
    assert np.array_equal(got, want)
    assert np.array_equal(routed, want)
    with pytest.raises(ValueError, match="work_bytes"):
        run("tw_chain_unpack_count_planes", bound, ..., None, work, wb - 1)
