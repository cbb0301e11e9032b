"""The fused pre-pass of the class-run chain count (csrc/chain.hip k_chain_prepass, DESIGN
§4.1l) behind tw_count_pairs_chain_planes: one launch builds the planes, sorts every bag's z
images into class runs — in registers, one pass over global memory, for bags of up to 16384
images; the two-pass streaming loop for larger ones — and zeroes the counts.

Every case is counted under tw_count_chain_prepass 1 (the separate launches) and 2 (fused) and
both must equal, exactly, NumPy's integer count per bag,
np.searchsorted(np.sort(z), x, "left").sum().  tw_count_chain_prepass_of must report the form
the case is meant to run, so a silent fallback cannot pass.  Planes are forced with
tw_count_chain_set_plan(2, 0) and class bits with tw_count_chain_set_class_bits(k), so small bags
take the class form; every hook is restored in a finally.  The workspace holds 0xFF and the
output 777 before every call.

Bags: 3 shards x 2 steps with ragged offsets, one shard with a single z and one with a single x,
and beside it 1 shard x 1 step.  z images per bag: 1; 255, 256, 257 (the block's threads); 4096,
4097 (16 and 64 images per thread); 16383, 16384 (the register-resident capacity); 16385 (form
3).  x images per bag: 1, 2047, 2048, 2049, 4097.  Bounds 2^16 - 1, 2^20 - 1, 2^24 - 1 (NB = 16,
20, 24), class bits 1, 4, 8 and automatic: NB - K = 12 runs the wide digits, (16, 8) the
four-digit loop, the others the masked planes.  Distributions: uniform; all z equal; z only in
class 0 and class 2^k - 1; z and x at 0 and at the bound; x drawn from the z images."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BOUNDS = [2 ** 16 - 1, 2 ** 20 - 1, 2 ** 24 - 1]
CLASS_BITS = [1, 4, 8, -1]
THREADS, CAP_SMALL, CAP = 256, 4096, 16384
# (x sizes, z sizes) per shard; shard 1 has a single z, shard 2 a single x
LAYOUTS3 = [
    ((2047, 2049, 1), (255, 1, 257)),
    ((2048, 4097, 1), (256, 1, 4097)),
    ((1, 2049, 1), (4096, 1, 16383)),
    ((2047, 1, 1), (16384, 1, 1)),
    ((4097, 2048, 1), (16385, 1, 16384)),
]
LAYOUTS1 = [((2049,), (257,)), ((1,), (16384,)), ((2047,), (16385,)), ((4097,), (1,))]
DISTS = ["uniform", "equal", "ends", "extremes", "x_from_z"]


def _nb(bound):
    return next(b for b in (16, 18, 20, 22, 24) if bound < 2 ** b)


def _draw(rng, dist, bound, k, nx, nz):
    """x and z images (integers in [0, bound]) of one bag."""
    nb = _nb(bound)
    kk = k if k > 0 else 2
    low = 2 ** (nb - kk)
    if dist == "uniform":
        z = rng.randint(0, bound + 1, nz)
    elif dist == "equal":
        z = np.full(nz, bound // 3)
    elif dist == "ends":  # complemented class 2^k - 1: z < 2^(NB - k); class 0: the top images
        z = np.where(rng.rand(nz) < 0.5, rng.randint(0, low, nz),
                     2 ** nb - low + rng.randint(0, low, nz))
    elif dist == "extremes":
        z = np.where(rng.rand(nz) < 0.5, 0, bound)
    else:
        z = rng.randint(0, bound + 1, nz)
    if dist == "extremes":
        x = np.where(rng.rand(nx) < 0.5, 0, bound)
    elif dist == "x_from_z":
        x = z[rng.randint(0, nz, nx)]
    else:
        x = rng.randint(0, bound + 1, nx)
    x, z = x.astype(np.int64), z.astype(np.int64)
    assert 0 <= z.min() and z.max() <= bound and 0 <= x.min() and x.max() <= bound
    return x, z


class _Bags:
    """The bags [steps][shards] of one launch on the device, and NumPy's counts."""

    def __init__(self, torch, L, rng, bound, k, xs, zs, steps, dist):
        self.torch, self.L, self.bound = torch, L, bound
        self.N, self.T = len(xs), steps
        x_off = np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)
        z_off = np.concatenate([[0], np.cumsum(zs)]).astype(np.int64)
        xb = np.zeros((steps, x_off[-1]), np.float32)
        zb = np.zeros((steps, z_off[-1]), np.float32)
        self.want = np.zeros((steps, self.N), np.int64)
        for c in range(steps):
            for s in range(self.N):
                x, z = _draw(rng, dist, bound, k, xs[s], zs[s])
                xb[c, x_off[s]:x_off[s + 1]] = x
                zb[c, z_off[s]:z_off[s + 1]] = -z.astype(np.float32)
                self.want[c, s] = int(np.searchsorted(np.sort(z), x, "left").sum())
        self.xd, self.zd = torch.from_numpy(xb).cuda(), torch.from_numpy(zb).cuda()
        self.xo, self.zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
        self.shape = (self.N, steps, max(xs), max(zs))
        self.head = (self.xd, self.xo, xb.shape[1], self.zd, self.zo, zb.shape[1], *self.shape, 0)
        self.work_bytes = int(L.lib().tw_chain_planes_work_bytes(*self.shape, 0, bound))

    def form(self):
        return int(self.L.lib().tw_count_chain_prepass_of(*self.shape, self.bound))

    def count(self, work):
        o = self.torch.full((self.T, self.N), 777, dtype=self.torch.int64, device="cuda")
        self.L.call("tw_count_pairs_chain_planes", *self.head, self.bound, o,
                    self.L.stream_handle(), work, self.work_bytes)
        return o


def _mode(L, m):
    return int(L.lib().tw_count_chain_prepass(m))


def _reset(L):
    L.call("tw_count_chain_set_plan", 0, 0)
    L.call("tw_count_chain_set_swap", 1)
    L.call("tw_count_chain_set_class_bits", -1)
    assert _mode(L, 0) in (0, 1, 2)


def _expected_form(mode, k, n_bags, max_nz):
    """prepass_of under forced planes: class bits k (automatic: none below 32 bags)."""
    if mode == 1 or k == 0 or (k < 0 and n_bags < 32):
        return 1
    return 2 if max_nz <= CAP else 3


@pytest.mark.parametrize("k", CLASS_BITS)
@pytest.mark.parametrize("bound", BOUNDS)
def test_prepass_counts_equal_numpy_under_both_forms(gpu, bound, k):
    import torch
    from tuplewise import _lib as L
    assert float(np.float32(bound)) == bound
    rng = np.random.RandomState(bound % 9949 + 8 * (k + 1))
    forms = set()
    try:
        L.call("tw_count_chain_set_plan", 2, 0)
        L.call("tw_count_chain_set_class_bits", k)
        for steps, layouts in ((2, LAYOUTS3), (1, LAYOUTS1)):
            for i, (xs, zs) in enumerate(layouts):
                for dist in DISTS if i % 2 == 0 or steps == 1 else DISTS[:1] + DISTS[2:3]:
                    a = _Bags(torch, L, rng, bound, k, xs, zs, steps, dist)
                    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
                    for mode in (1, 2):
                        _mode(L, mode)
                        want_form = _expected_form(mode, k, len(xs) * steps, max(zs))
                        assert a.form() == want_form, (xs, zs, dist, mode)
                        forms.add(want_form)
                        work.fill_(0xFF)
                        got = a.count(work).cpu().numpy()
                        print("bound", bound, "k", k, "x", xs, "z", zs, dist, "mode", mode,
                              "form", want_form, "max |count - numpy|",
                              np.abs(got - a.want).max())
                        assert np.array_equal(got, a.want), (xs, zs, dist, mode)
    finally:
        _reset(L)
    assert forms == ({1, 2, 3} if k > 0 else {1})


def test_prepass_automatic_class_bits_at_32_bags(gpu):
    """32 bags, where the automatic rule gives class bits: automatic and forced-fused settings
    run the fused launch, mode 1 the separate ones; same counts."""
    import torch
    from tuplewise import _lib as L
    bound = 2 ** 20 - 1
    rng = np.random.RandomState(32)
    xs = tuple(2049 + 61 * s if s % 3 else 1 + s for s in range(16))
    zs = tuple(300 + 25 * s if s % 5 else 1 for s in range(16))
    a = _Bags(torch, L, rng, bound, 2, xs, zs, 2, "uniform")
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    try:
        L.call("tw_count_chain_set_plan", 2, 0)
        for mode, form in ((0, 2), (1, 1), (2, 2)):
            _mode(L, mode)
            assert a.form() == form
            work.fill_(0xFF)
            assert np.array_equal(a.count(work).cpu().numpy(), a.want), mode
    finally:
        _reset(L)


def test_prepass_forms_alternate_on_one_workspace(gpu):
    """Modes 1, 2, 1, 2 and then 2 again on one workspace without a refill, in stream order:
    every launch rewrites its regions before its count."""
    import torch
    from tuplewise import _lib as L
    bound = 2 ** 20 - 1
    rng = np.random.RandomState(5)
    a = _Bags(torch, L, rng, bound, 8, (2049, 4097, 1), (4097, 1, 16384), 2, "uniform")
    b = _Bags(torch, L, rng, bound, 8, (2049, 4097, 1), (4097, 1, 16384), 2, "ends")
    assert not np.array_equal(a.want, b.want)
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    work.fill_(0xFF)
    outs = []
    try:
        L.call("tw_count_chain_set_plan", 2, 0)
        L.call("tw_count_chain_set_class_bits", 8)
        for mode, bags in ((1, a), (2, a), (1, a), (2, a), (2, b), (2, b), (1, b)):
            _mode(L, mode)
            assert bags.form() == (1 if mode == 1 else 2)
            outs.append((bags, bags.count(work)))
    finally:
        _reset(L)
    torch.cuda.synchronize()
    for bags, o in outs:
        assert np.array_equal(o.cpu().numpy(), bags.want)


def test_prepass_hook_and_query(gpu):
    """tw_count_chain_prepass returns the setting before the call, -1 only reports, any other
    value is refused and changes nothing; the query follows the setting."""
    from tuplewise import _lib as L
    before = _mode(L, -1)
    assert before == 0  # (automatic, unless another test left a setting behind)
    try:
        assert _mode(L, 2) == before
        assert _mode(L, -1) == 2
        for bad in (-2, 3, 4, 100):
            assert _mode(L, bad) == L.TW_ERR_ARG
            assert b"tw_count_chain_prepass" in L.lib().tw_last_error()
            assert _mode(L, -1) == 2
        assert _mode(L, 1) == 2
        assert _mode(L, -1) == 1
        q = lambda *a: int(L.lib().tw_count_chain_prepass_of(*a))
        # the bench's launch: 64 shards x 20 steps of 15625 images, automatic plan
        assert q(64, 20, 15625, 15625, 1_000_000) == 1
        assert _mode(L, 0) == 1
        assert q(64, 20, 15625, 15625, 1_000_000) == 2
        assert q(64, 20, 15625, 16385, 1_000_000) == 3
        assert q(1, 1, 100_000, 100_000, 1_000_000) == 1  # fewer than 32 bags: no class bits
        assert q(64, 20, 15625, 15625, 2 ** 24) == 0  # no bound below 2^24: packed
        assert q(0, 20, 15625, 15625, 1_000_000) == 0
    finally:
        assert _mode(L, before) in (0, 1, 2)
    assert _mode(L, -1) == before
