"""The masked-plane class loop with the run read by scalar loads (csrc/chainclass.h
bits_count_class) behind tw_count_pairs_chain_planes: the class-constant term
len * popc(G) needs the run's exact length, whole batches of a scalar load and the images left
over take different paths, run starts are arbitrary word offsets, and a batch may read past its
run's end — into the next run, the next bag or, from the last run of the last bag, the entry
counts — without ever comparing what it read there.

x tiles of 1 .. 4 plane groups with ragged tails, under forced class bits {1, 4, 8} and a
forced z chunk of 8 (many short runs, unaligned starts); z bags of 1 .. 130 images; runs of
b - 1, b, b + 1 images for every scalar batch width b in {2, 4, 8, 16}; one bound per plane
count NB in {16, 18, 20, 22, 24}; ties x == z, NaN x, the "never" image, z image 0 and all x at the
bound; 3 shards x 2 steps per launch, the last run of the last bag included; and one launch of
32 small bags under the automatic rule.  Every count equals, exactly, a NumPy broadcast compare
and the k = 0 path (tw_count_chain_set_class_bits(0): k_count_chain_planes).  The workspace
holds 0xFF before every call: a word past a run's end that reached the compare, or a plane word
read without having been written, would count."""
import numpy as np
import pytest

import test_gpu_count_planes as P

pytestmark = pytest.mark.gpu

T = P.T
NEVER, NAN = -1, -2  # x images that are greater than no z
BATCHES = (2, 4, 8, 16)  # the scalar load widths the class loop can be built for (shipped: 4)


@pytest.fixture
def hooks(gpu):
    """The tuning hooks, put back to automatic whatever the test did."""
    from tuplewise import _lib as L
    yield L
    L.call("tw_count_chain_set_plan", 0, 0)
    L.call("tw_count_chain_set_swap", 1)
    L.call("tw_count_chain_set_class_bits", -1)


def _launch(torch, L, bound, bags):
    """A P._Launch on given bags: bags[s] = (x images, NEVER / NAN among them; z images); step 1
    holds every bag's images in reverse order.  want: the NumPy broadcast compare."""
    a = object.__new__(P._Launch)
    a.torch, a.L, a.bound, a.N = torch, L, bound, len(bags)
    xs, zs = [len(b[0]) for b in bags], [len(b[1]) for b in bags]
    x_off = np.concatenate([[0], np.cumsum(xs)]).astype(np.int64)
    z_off = np.concatenate([[0], np.cumsum(zs)]).astype(np.int64)
    xb, zb = np.zeros((T, x_off[-1]), np.float32), np.zeros((T, z_off[-1]), np.float32)
    a.want = np.zeros((T, a.N), np.int64)
    for s, (x, z) in enumerate(bags):
        x, z = np.asarray(x, np.int64), np.asarray(z, np.int64)
        assert x.max(initial=0) <= bound and z.max(initial=0) <= bound and z.min(initial=0) >= 0
        xf = np.where(x == NEVER, np.float32(P.NEVER), x).astype(np.float32)
        xf[x == NAN] = np.nan
        count = int((x[:, None] > z[None, :]).sum())  # (NEVER and NAN are negative: no z)
        for c in range(T):
            xb[c, x_off[s]:x_off[s + 1]] = xf[::-1] if c else xf
            zb[c, z_off[s]:z_off[s + 1]] = -(z[::-1] if c else z).astype(np.float32)
            a.want[c, s] = count
    a.xd, a.zd = torch.from_numpy(xb).cuda(), torch.from_numpy(zb).cuda()
    a.xo, a.zo = torch.from_numpy(x_off).cuda(), torch.from_numpy(z_off).cuda()
    a.head = (a.xd, a.xo, xb.shape[1], a.zd, a.zo, zb.shape[1], a.N, T, max(xs), max(zs), 0)
    a.work_bytes = int(L.lib().tw_chain_planes_work_bytes(a.N, T, max(xs), max(zs), 0, bound))
    assert a.work_bytes > 0
    return a


def _check(a, torch, L, tag, plan, ks, swaps=(0, 2)):
    """a's counts under the plan, each swap mode and each class-bits setting == NumPy == k = 0."""
    work = torch.empty(a.work_bytes, dtype=torch.uint8, device="cuda")
    L.call("tw_count_chain_set_plan", *plan)
    for swap in swaps:
        L.call("tw_count_chain_set_swap", swap)
        L.call("tw_count_chain_set_class_bits", 0)
        work.fill_(0xFF)
        base = a.planes(work).cpu().numpy()
        assert np.array_equal(base, a.want), (tag, swap, "k = 0")
        for k in ks:
            L.call("tw_count_chain_set_class_bits", k)
            work.fill_(0xFF)
            got = a.planes(work).cpu().numpy()
            print(tag, "plan", plan, "swap", swap, "k", k, "max |masked - numpy|",
                  np.abs(got - a.want).max())
            assert np.array_equal(got, a.want), (tag, swap, k)
            assert np.array_equal(got, base), (tag, swap, k)


def _x(rng, bound, n, z):
    """n x images: random, ties with the bag's z, 0, the bound, "never" and NaN."""
    x = rng.randint(0, bound + 1, n).astype(np.int64)
    if len(z):
        tie = rng.rand(n) < 0.3
        x[tie] = z[rng.randint(0, len(z), int(tie.sum()))]
    if n > 4:
        x[0], x[1] = 0, bound
        x[2::37] = NEVER
        x[3::41] = NAN
    return x


def _z(rng, bound, n):
    """n z images: random, a few equal ones, image 0 and the bound."""
    z = rng.randint(0, bound + 1, n).astype(np.int64)
    if n > 2:
        z[0], z[1] = 0, bound
    if n > 8:
        z[5:8] = z[4]
    return z


NZ = (1, 7, 9, 63, 65, 130)


@pytest.mark.parametrize("k", [1, 4, 8])
@pytest.mark.parametrize("nx", [1, 2047, 2048, 2049, 4097, 6145, 8193])
def test_masked_count_over_x_tiles_and_short_runs(hooks, nx, k):
    """Every x tile shape (1 .. 4 groups, ragged tails) against z bags of 1 .. 130 images cut
    into runs of at most 8: 3 shards x 2 steps per launch, ragged sizes."""
    import torch
    L = hooks
    bound = 1_000_000
    rng = np.random.RandomState(1000 * k + nx)
    for nzs in (NZ[0::2], NZ[1::2]):  # (1, 9, 65) and (7, 63, 130): the longest bag last
        bags = []
        for s, nz in enumerate(nzs):
            z = _z(rng, bound, nz)
            bags.append((_x(rng, bound, nx if s != 1 else max(1, nx - 1000), z), z))
        _check(_launch(torch, L, bound, bags), torch, L, f"nx {nx} nz {nzs}", (0, 8), (k,))


@pytest.mark.parametrize("k", [1, 8])
def test_masked_count_runs_around_every_batch_width(hooks, k):
    """Runs of exactly b - 1, b and b + 1 images for each scalar batch width b: every z of a
    bag in one class (equal top 8 bits) under a z chunk that does not cut it, so the bag is one
    run; the last bag's single run is the last of the region, and x all at the bound in one
    shard makes G full, where a wrong length in the constant term shows."""
    import torch
    L = hooks
    bound = 1_000_000
    rng = np.random.RandomState(77 + k)
    lens = sorted({b + d for b in BATCHES for d in (-1, 0, 1)})
    for i in range(0, len(lens), 3):
        bags = []
        for s, n in enumerate(lens[i:i + 3]):
            field = int(rng.randint(0, 200)) << 12  # NB = 20: the top 8 bits, below the bound's
            z = field + rng.randint(0, 1 << 12, n).astype(np.int64)
            x = _x(rng, bound, 2049 + 64 * s, z) if s != 1 else np.full(2049, bound, np.int64)
            bags.append((x, z))
        _check(_launch(torch, L, bound, bags), torch, L, f"run lengths {lens[i:i + 3]}",
               (4, 600), (k,))


@pytest.mark.parametrize("bound", [2 ** 16 - 1, 2 ** 18 - 1, 1_000_000, 2 ** 22 - 1, 2 ** 24 - 1])
def test_masked_count_at_every_plane_count(hooks, bound):
    """One bound per instantiated NB, k in {4, 8}: z image 0 against padded x slots (E set, the
    planes 0), all x at the bound, ties, NaN and "never" x."""
    import torch
    L = hooks
    assert float(np.float32(bound)) == bound
    rng = np.random.RandomState(bound % 9973)
    z0 = _z(rng, bound, 65)
    z1 = np.concatenate([np.zeros(5, np.int64), _z(rng, bound, 25)])  # z image 0, repeated
    z2 = _z(rng, bound, 130)
    bags = [(_x(rng, bound, 4097, z0), z0),
            (np.full(2049, bound, np.int64), z1),  # all x at the bound
            (np.concatenate([z2, _x(rng, bound, 2047 - 130, z2)]), z2)]  # every z met by an x
    _check(_launch(torch, L, bound, bags), torch, L, f"bound {bound}", (0, 8), (4, 8))


def test_masked_count_under_the_automatic_rule(hooks):
    """32 small bags (16 shards x 2 steps) under the automatic plan, swap rule and class bits:
    the shipped default path (k > 0 from 32 bags of >= 96 z images up)."""
    import torch
    L = hooks
    bound = 1_000_000
    rng = np.random.RandomState(5)
    bags = []
    for s in range(16):
        z = _z(rng, bound, 200 + 13 * s)
        bags.append((_x(rng, bound, 2100 + 97 * s, z), z))
    a = _launch(torch, L, bound, bags)
    _check(a, torch, L, "automatic", (0, 0), (-1,), swaps=(1,))
