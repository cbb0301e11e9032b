"""Every tuning hook's launch plans at small shapes, exact counts.

The C ABI's process-global tuning hooks (tw_*_set_* in include/tuplewise.h) promise that results
do not depend on them.  The automatic plans choose by size, so a small test runs the small-size
variant and the variant the workload runs is reached by a full-size test at one shape.  Here
every hook forces the large-shape code at shapes that take microseconds: each family below
loops over its plan table inside the test body (inputs uploaded once), and every plan's output
is compared, exactly, with a NumPy result that comes from no kernel of this project (a
broadcast compare, np.sort + np.searchsorted, oracle.permute_scatter, the oracle's permutation
chain) and with the default plan's output (explicitly where outputs are kept; where every plan,
the default included, is compared with one reference array, the equality follows).  No
tolerance anywhere: integer counts and bit patterns.

HOOKS is the inventory tests/test_plan_hooks_cpu.py checks the header against; the reference
functions and the input builders of this module are checked there too, without a GPU.
"""
import itertools

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
M64 = 2 ** 64 - 1


def _product(*axes):
    return [tuple(p) for p in itertools.product(*axes)]


Z_CHUNKS = (0, 5, 8, 15, 16, 17, 24, 31, 32, 33, 520)
# hook -> its default (the initial value in the source file) and the values swept below
HOOKS = {
    "tw_count_set_plan": dict(default=(0, 0), values=_product((1, 2, 4, 8), Z_CHUNKS)),
    "tw_count_set_scalar_mix": dict(default=(1,), values=[(0,), (1,)]),
    "tw_count_step_set_plan": dict(default=(0, 0, 1),
                                   values=_product((0, 8, 24, 64), (0, 8, 16, 40), (0, 1))),
    "tw_count_rank_set_plan": dict(default=(0, 0), values=_product((8, 16), (0, 8, 264, 1024))),
    "tw_count_rank_set_next": dict(default=(0,), values=[(0,), (1,)]),
    "tw_rank_set_plan": dict(default=(1024, 8), values=_product((512, 1024, 2048), (4, 8, 16))),
    "tw_rank_set_small": dict(default=(256, 2048, 4),
                              values=_product((256, 512, 1024, 2048), (512, 1024, 2048),
                                              (4, 8, 16))),
    "tw_count_sorted_set_chunk": dict(default=(4096,),
                                      values=[(c,) for c in (1024, 2048, 4096, 8192, 16384)]),
    "tw_count_sorted_set_bucket": dict(default=(1,), values=[(0,), (1,), (2,)]),
    "tw_count_idx_set_variant": dict(default=(0,), values=[(v,) for v in range(6)]),
    "tw_count_idx_set_parts": dict(default=(0,), values=[(p,) for p in range(4)]),
    "tw_count_img_set_plan": dict(default=(0, 9), values=_product((0, 3), (1, 2, 4, 9, 10, 12))),
    "tw_count_rng_set_codes": dict(default=(3,), values=[(c,) for c in range(4)]),
    "tw_chain_set_emit": dict(default=(0, 0),
                              values=[(2, 1), (2, 8), (4, 1), (4, 4), (8, 1), (8, 2)]),
    "tw_exchange_set_grid": dict(default=(0,), values=[(g,) for g in (0, 1, 3, 8, 1000)]),
}
# table values the ABI answers with TW_ERR_ARG: asserted as refused wherever they are set, never
# dropped from the table (none today)
REFUSED = set()


def reset_hooks(L):
    for name, h in HOOKS.items():
        L.call(name, *h["default"])


def set_hook(L, name, args):
    """Set one hook; a refusal (TW_ERR_ARG -> ValueError) must be one the table expects.
    Returns whether the value is in force."""
    try:
        L.call(name, *args)
    except ValueError:
        assert (name, tuple(args)) in REFUSED, (name, args)
        return False
    assert (name, tuple(args)) not in REFUSED, (name, args)
    return True


@pytest.fixture(autouse=True)
def _hooks_back_to_default():
    """Hooks are process-global and have no getters: every test of this module leaves every
    hook at its default, whatever happened in it."""
    yield
    from tuplewise import _lib as L
    reset_hooks(L)


# ------------------------------------------------------------------ NumPy references
def pair_weights(x, z, pred):
    """The (nx, nz) matrix of counted units of one shard, from the broadcast compare: 1{x > z}
    ("gt"; "subgt" on doubles is the same predicate), 2 1{x > z} + 1{x == z} ("half"),
    1{(x - z) mod 2^64 as int64 > 0} ("subgt" on int64)."""
    a, b = np.asarray(x).reshape(-1, 1), np.asarray(z).reshape(1, -1)
    if pred == "half":
        return 2 * (a > b).astype(np.int64) + (a == b)
    if pred == "subgt" and a.dtype == np.int64:
        with np.errstate(over="ignore"):
            return ((a - b) > 0).astype(np.int64)  # int64 array subtraction wraps
    assert pred in ("gt", "subgt")
    return (a > b).astype(np.int64)


def ref_count(x, z, pred):
    if pred == "gt" or (pred == "subgt" and np.asarray(x).dtype != np.int64):
        return O.un_count(x, z)
    return int(pair_weights(x, z, pred).sum())


def ref_sorted_count(x, z, half):
    """#{x > z} (half: + #{x >= z}) by np.sort + np.searchsorted; NaN compares false."""
    x, z = np.asarray(x).reshape(-1), np.asarray(z).reshape(-1)
    if x.dtype.kind == "f":
        x, z = x[~np.isnan(x)], z[~np.isnan(z)]
    zs = np.sort(z)
    c = int(np.searchsorted(zs, x, side="left").sum())
    return c + int(np.searchsorted(zs, x, side="right").sum()) if half else c


def ref_images(v, z_all, side="left"):
    """g(v) = #{z in z_all : z < v} (side="right": h(v) = #{z <= v}) by np.searchsorted on the
    sorted non-NaN z; a NaN v lies above every value (tw_rank_images' order; a NaN x is replaced
    by the "never" image by ref_records)."""
    v, z = np.asarray(v).reshape(-1), np.asarray(z_all).reshape(-1)
    if z.dtype.kind == "f":
        z = z[~np.isnan(z)]
    g = np.searchsorted(np.sort(z), v, side=side).astype(np.int64)
    if v.dtype.kind == "f":
        g[np.isnan(v)] = z.size
    return g


def _f32_words(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)


def ref_records(X, Z, Z_all, flags):
    """tw_rank_images_query's outputs as the header states them: x image g (a NaN x: -2^25), z
    image -g; flags bit 0: the X high word is h as f32 bits instead of the index; bit 1: compact
    (x: f32, or int64 {g, h} pairs with bit 0; z: f32)."""
    X, Z = np.asarray(X).reshape(-1), np.asarray(Z).reshape(-1)
    gx = ref_images(X, Z_all).astype(np.float32)
    hx = ref_images(X, Z_all, "right").astype(np.float32)
    if X.dtype.kind == "f":
        gx[np.isnan(X)] = hx[np.isnan(X)] = np.float32(-2.0 ** 25)
    gz = -ref_images(Z, Z_all).astype(np.float32)
    if flags & 2:
        xr = (_f32_words(gx) | (_f32_words(hx) << np.uint64(32))).view(np.int64) if flags & 1 \
            else gx
        return xr, gz
    hi_x = _f32_words(hx) if flags & 1 else np.arange(X.size, dtype=np.uint64)
    xr = _f32_words(gx) | (hi_x << np.uint64(32))
    zr = _f32_words(gz) | (np.arange(Z.size, dtype=np.uint64) << np.uint64(32))
    return xr.view(np.int64), zr.view(np.int64)


def bag_regions(n, k, n_shards):
    """Region of every position of one side of a rank's prop-SWOR layout: shard b holds
    [min(b k, n), min((b + 1) k, n)), region n_shards the tail that belongs to no shard."""
    p = np.arange(n, dtype=np.int64)
    return np.minimum(p // k, n_shards) if k > 0 else np.full(n, n_shards, dtype=np.int64)


def bag_canon(bags, region):
    """The (steps, n) bags as sorted arrays: each row's words sorted inside every region (signed
    integer order of the bit patterns), so two emissions agree iff every (step, shard) bag
    holds the same multiset."""
    bags = np.asarray(bags)
    out = np.empty_like(bags)
    for c in range(bags.shape[0]):
        out[c] = bags[c][np.lexsort((bags[c], region))]
    return out


def _bag_canon_dev(bags, region_dev):
    """bag_canon on the device (the sweep compares hundreds of bags)."""
    import torch
    if bags.shape[1] == 0:
        return bags
    v, idx = torch.sort(bags, dim=1)
    _, idx2 = torch.sort(region_dev[idx], dim=1, stable=True)
    return torch.gather(v, 1, idx2)


# ------------------------------------------------------------------ inputs of the counts
# ~ten ragged shards in one launch: an empty x side, an empty z side, nx at and around one wave
# (63, 64, 65) and one R = 8 tile (511, 513); max_nx = 1100 gives R = 8 three tiles of 512, the
# last ragged; max_nz = 530
SHARD_NX = (0, 1, 63, 64, 65, 511, 513, 1100, 700, 257)
SHARD_NZ = (3, 0, 9, 530, 17, 33, 64, 529, 520, 100)
X_TILES = tuple(sorted({64 * R for R in (1, 2, 4, 8, 16)}))  # count R 1..8, rank-step R 8 / 16
Z_STEPS = tuple(sorted({c for c in Z_CHUNKS if c} | {8, 264, 1024}))  # + the rank step's chunks
SPECIALS = (np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324)
# positions next to no tile or chunk boundary and not last: the special values go there, so
# the boundary elements keep ordinary values that take part in counted pairs
X_SPECIAL_AT = (1, 2, 3, 4, 5, 6, 7)
Z_SPECIAL_AT = (1, 2, 3, 6, 11, 12, 13)
COUNT_KINDS = {("f64", "gt"): "f64", ("f64", "half"): "f64", ("f64", "subgt"): "f64",
               ("i64", "gt"): "i64", ("i64", "half"): "i64", ("i64", "subgt"): "i64wrap"}


def boundary_positions(n, steps):
    """The last position and the positions on each side of every multiple of every step."""
    s = {n - 1} if n else set()
    for st in steps:
        for k in range(st, n, st):
            s.update((k - 1, k))
    return sorted(s)


def participation(x, z, pred):
    """Which x and which z of a shard take part in at least one counted pair."""
    w = pair_weights(x, z, pred)
    return w.any(axis=1), w.any(axis=0)


def count_inputs(kind):
    """The shards' scores.  f64: ties by rounding, NaN, +-0, +-inf, +-5e-324 in valid lanes of x
    and z (under scalar-unit counting the padded lanes hold NaN too); i64: ties; i64wrap: values
    whose difference wraps.  Boundary elements (boundary_positions) that would take part in no
    counted pair get a value that does, so a dropped tail or a chunk off by one changes a
    count; tests/test_plan_hooks_cpu.py asserts the property from the references alone."""
    rng = np.random.RandomState(77)
    preds = {"f64": ("gt",), "i64": ("gt",), "i64wrap": ("subgt",)}[kind]
    xs, zs = [], []
    for nx, nz in zip(SHARD_NX, SHARD_NZ):
        if kind == "f64":
            x, z = rng.normal(size=nx).round(1), rng.normal(size=nz).round(1)
            if nx > 16:
                x[list(X_SPECIAL_AT)] = SPECIALS
                if nx > 1092:
                    x[1090] = np.nan  # a NaN in a valid lane of the last, ragged tile
            if nz > 16:
                z[list(Z_SPECIAL_AT)] = SPECIALS
        elif kind == "i64":
            x = rng.randint(-20, 20, nx).astype(np.int64)
            z = rng.randint(-20, 20, nz).astype(np.int64)
        else:
            x = (rng.randint(-2 ** 62, 2 ** 62, nx) * 2).astype(np.int64)
            z = (rng.randint(-2 ** 62, 2 ** 62, nz) * 2).astype(np.int64)
        bx, bz = boundary_positions(nx, X_TILES), boundary_positions(nz, Z_STEPS)
        for _ in range(8):
            if not (nx and nz):
                break
            changed = False
            for pred in preds:
                px, pz = participation(x, z, pred)
                for i in bx:
                    if not px[i]:  # above some z
                        x[i] = 9.5 if kind == "f64" else 25 if kind == "i64" else z[0] + 1
                        changed = True
                for j in bz:
                    if not pz[j]:  # below some x
                        z[j] = -9.5 if kind == "f64" else -25 if kind == "i64" else x[0] - 1
                        changed = True
            if not changed:
                break
        xs.append(x)
        zs.append(z)
    return xs, zs


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)


def _concat(parts, dtype):
    return np.concatenate([np.asarray(p, dtype=dtype) for p in parts]) if parts else \
        np.zeros(0, dtype=dtype)


class _Shards:
    """The count inputs on the device, uploaded once per test."""

    def __init__(self, L, xs, zs):
        dt = np.int64 if xs[0].dtype == np.int64 else np.float64
        self.code = L.TW_I64 if dt == np.int64 else L.TW_F64
        self.xs, self.zs = xs, zs
        self.X, self.Z = _concat(xs, dt), _concat(zs, dt)
        self.x, self.z = L.to_device(self.X), L.to_device(self.Z)
        self.xo, self.zo = L.to_device(_offsets(xs)), L.to_device(_offsets(zs))
        self.n = len(xs)
        self.max_nx, self.max_nz = max(map(len, xs)), max(map(len, zs))


def _pred_code(L, pred):
    return {"gt": L.TW_PRED_GT, "half": L.TW_PRED_HALF, "subgt": L.TW_PRED_SUBGT}[pred]


def _bits(t):
    """A device tensor as int64 bit patterns (NaN-safe equality)."""
    import torch
    return t.view(torch.int64) if t.dtype == torch.float64 else t


def _failed(labels, oks):
    """The labels of the plans whose device-side verdict is false (one D2H for all)."""
    import torch
    if not oks:
        return []
    bad = (~torch.stack(oks)).cpu().numpy()
    return [lab for lab, b in zip(labels, bad) if b]


# ------------------------------------------------------------------ A. complete count
@pytest.mark.parametrize("dtype,pred", sorted(COUNT_KINDS))
def test_complete_count_every_plan(gpu, dtype, pred):
    """tw_count_pairs under every (R, z_chunk) of tw_count_set_plan, with scalar-unit counting
    on and off: k_count_complete<T, R, NS, PRED> for R in {1, 2, 4, 8}, NS > 0 and NS = 0, and
    each regime of count_item's z loop (chunks of 5 and 8: the scalar tail and one group of 8;
    15: 8 + tail; 16, 17: the prefetch pipeline with and without a tail; 24, 31: pipeline + a
    group of 8 (+ tail); 32, 33: two pipeline rounds; 520: one chunk and a ragged second)
    against the broadcast compare, per shard.  The scalar-mix hook is ignored for int64: the
    same equality is asserted there."""
    import torch
    from tuplewise import _lib as L
    xs, zs = count_inputs(COUNT_KINDS[dtype, pred])
    want = np.array([ref_count(x, z, pred) for x, z in zip(xs, zs)], dtype=np.uint64)
    assert (want > 0).sum() == 8  # every shard with both sides non-empty counts something
    sh = _Shards(L, xs, zs)
    code = _pred_code(L, pred)
    plans = [(mix[0], R, zc) for mix in HOOKS["tw_count_set_scalar_mix"]["values"]
             for R, zc in HOOKS["tw_count_set_plan"]["values"]]
    outs = torch.full((1 + len(plans), sh.n), -1, dtype=torch.int64, device="cuda")

    def run(row):
        L.call("tw_count_pairs", sh.x, sh.xo, sh.z, sh.zo, sh.n, sh.max_nx, sh.max_nz, sh.code,
               code, outs[row], L.stream_handle())

    run(0)  # the default plan
    for row, (mix, R, zc) in enumerate(plans, 1):
        assert set_hook(L, "tw_count_set_scalar_mix", (mix,))
        assert set_hook(L, "tw_count_set_plan", (R, zc))
        run(row)
    got = outs.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[0], want), ("default", got[0], want)
    for plan, g in zip(plans, got[1:]):
        assert np.array_equal(g, want), (plan, g, want)
        assert np.array_equal(g, got[0]), plan


# ------------------------------------------------------------------ B. fused steps
# count plans under the step sweep.  With the shards above (10 shards, max 1100 x 530):
#   (8, 0): 3 tiles x 1 chunk -> 8 count blocks: FEWER COUNT BLOCKS THAN SPARE BLOCKS for
#           blocks = 24 and 64 (and 8 against 8 for blocks = 0 / 8);
#   (1, 0): 18 tiles -> 45 count blocks.  blocks = 24, every = 16, tail = 0 is the SPREAD
#           placement: groups at blocks 0-7, 16-23 and 32-39 of a 69-block grid, count blocks
#           8-15 and 24-31 between them and 40-68 after them (group 0 always leads the grid, so
#           no count block comes before it); blocks = 64, every = 40 needs (8 - 1) * 40 + 8 = 288
#           blocks and the grid has 109: the FALLBACK TO THE LEADING BLOCKS (likewise every =
#           16 with 64 spare blocks: 120 > 109);
#   (1, 33): 17 chunks -> 765 count blocks: every = 40 with 64 spare blocks fits (288 <= 829)
#           and spreads 8 groups; every = 0 chooses its own spacing (three groups 248 apart for
#           blocks = 24).
# The "nothing to count" launches (n_shards == 0, max_nx == 0) run under every step plan too.
STEP_COUNT_PLANS = ((1, 0), (8, 0), (1, 33))


@pytest.mark.parametrize("dtype,pred", [("f64", "gt"), ("f64", "half"), ("i64", "subgt")])
def test_count_step_every_plan(gpu, dtype, pred):
    """tw_count_pairs_step under every (blocks, every, tail) of tw_count_step_set_plan crossed
    with the count plans above: counts == the broadcast compare, x_next / z_next ==
    oracle.permute_scatter, out_next zeroed — spare blocks last, leading and spread, with fewer
    count blocks than spare blocks, with the forced spacing falling back to the leading blocks,
    and in the launches that have nothing to count."""
    import torch
    from tuplewise import _lib as L
    xs, zs = count_inputs(COUNT_KINDS[dtype, pred])
    want = np.array([ref_count(x, z, pred) for x, z in zip(xs, zs)], dtype=np.uint64)
    sh = _Shards(L, xs, zs)
    code = _pred_code(L, pred)
    kx, kz = 11, 12
    want_dev = L.to_device(want.view(np.int64))
    xn_want = _bits(L.to_device(O.permute_scatter(sh.X, kx)))
    zn_want = _bits(L.to_device(O.permute_scatter(sh.Z, kz)))
    n_x, n_z = int(sh.X.size), int(sh.Z.size)

    def step(n_shards, max_nx, max_nz):
        """One call on fresh buffers; the device-side verdicts (counts, next arrays, zeroing)."""
        out = torch.zeros(sh.n, dtype=torch.int64, device="cuda")
        out_next = torch.full((5,), 77, dtype=torch.int64, device="cuda")
        xn, zn = torch.full_like(sh.x, 3), torch.full_like(sh.z, 3)
        L.call("tw_count_pairs_step", sh.x, sh.xo, sh.z, sh.zo, n_shards, max_nx, max_nz,
               sh.code, code, out, n_x, xn, kx, n_z, zn, kz, out_next, 5, L.stream_handle())
        nxt = (_bits(xn) == xn_want).all() & (_bits(zn) == zn_want).all() & \
            (out_next == 0).all()
        return out, nxt

    labels, oks, outs = [], [], []
    base, ok = step(sh.n, sh.max_nx, sh.max_nz)  # every hook at its default
    labels.append("default")
    oks.append(ok & (base == want_dev).all())
    for cp in STEP_COUNT_PLANS:
        assert set_hook(L, "tw_count_set_plan", cp)
        for sp in HOOKS["tw_count_step_set_plan"]["values"]:
            assert set_hook(L, "tw_count_step_set_plan", sp)
            out, ok = step(sh.n, sh.max_nx, sh.max_nz)
            labels.append(("count", cp, sp))
            oks.append(ok & (out == want_dev).all() & (out == base).all())
            if cp == STEP_COUNT_PLANS[0]:  # nothing to count, with a next step
                # (only the next step's outputs are checked: there is no count to check)
                for name, args in (("no shards", (0, 0, 0)), ("max_nx == 0", (sh.n, 0, 0))):
                    labels.append((name, sp))
                    oks.append(step(*args)[1])
    assert _failed(labels, oks) == []


def _edge_sample(rng, n, kind):
    """tests/test_gpu_rankimage.py's value generator."""
    from test_gpu_rankimage import _edge_sample as gen
    return gen(rng, n, kind)


@pytest.mark.parametrize("kind", ["f64", "i64"])
def test_count_rank_step_every_plan(gpu, kind):
    """tw_count_pairs_rank_step with its spare blocks last and first (tw_count_rank_set_next)
    under R = 8 / 16 and z chunks 0 / 8 / 264 / 1024 of tw_count_rank_set_plan, on the shards of
    the complete count (count_inputs: its boundary elements cover the rank step's 512- and
    1024-value tiles and its chunks too): counts == the broadcast compare on the scores, both
    record arrays' next repartition == oracle.permute_scatter of the records, out_next zeroed;
    and the launches with nothing to count under both placements."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    xs, zs = count_inputs(kind)
    sh = _Shards(L, xs, zs)
    want = np.array([O.un_count(a, b) for a, b in zip(xs, zs)], dtype=np.uint64)
    assert (want > 0).sum() == 8
    want_dev = L.to_device(want.view(np.int64))
    ops = HipOps()
    xr, zr = ops.rank_images(sh.x, sh.z, sh.code)
    wx, wz = ref_records(sh.X, sh.Z, sh.Z, 0)
    assert np.array_equal(xr.cpu().numpy(), wx) and np.array_equal(zr.cpu().numpy(), wz)
    kx, kz = 11, 12
    xn_want = L.to_device(O.permute_scatter(wx, kx))
    zn_want = L.to_device(O.permute_scatter(wz, kz))

    def step(n_shards, max_nx, max_nz):
        out = torch.zeros(sh.n, dtype=torch.int64, device="cuda")
        out_next = torch.full((5,), 77, dtype=torch.int64, device="cuda")
        xn, zn = torch.full_like(xr, 3), torch.full_like(zr, 3)
        ops.count_rank_step(xr, sh.xo, zr, sh.zo, n_shards, max_nx, max_nz, out, xn, kx, zn,
                            kz, out_next)
        return out, (xn == xn_want).all() & (zn == zn_want).all() & (out_next == 0).all()

    labels, oks = [], []
    base, ok = step(sh.n, sh.max_nx, sh.max_nz)
    labels.append("default")
    oks.append(ok & (base == want_dev).all())
    for front in HOOKS["tw_count_rank_set_next"]["values"]:
        assert set_hook(L, "tw_count_rank_set_next", front)
        for plan in HOOKS["tw_count_rank_set_plan"]["values"]:
            assert set_hook(L, "tw_count_rank_set_plan", plan)
            out, ok = step(sh.n, sh.max_nx, sh.max_nz)
            labels.append((front, plan))
            oks.append(ok & (out == want_dev).all() & (out == base).all())
        for name, args in (("no shards", (0, 0, 0)), ("max_nx == 0", (sh.n, 0, 0))):
            labels.append((name, front))  # (nothing counted: the next step's outputs only)
            oks.append(step(*args)[1])
    assert _failed(labels, oks) == []


# ------------------------------------------------------------------ C. ranking
def _rank_all_layouts(L, ops, Xd, Zd, code, want_dev):
    """tw_rank_images and the half bit 0 / bit 1 record layouts of tw_rank_images_query, each
    with the workspace size queried again (HipOps asks tw_rank_images_work_bytes per call, as the
    header requires after a set): one device-side verdict."""
    import torch
    n, m = int(Xd.numel()), int(Zd.numel())
    assert L.lib().tw_rank_images_work_bytes(n, m) >= 0
    got = [ops.rank_images(Xd, Zd, code),
           ops.rank_images_query(Zd, Xd, Zd, code, half=True),
           ops.rank_images_query(Zd, Xd, Zd, code, compact=True),
           ops.rank_images_query(Zd, Xd, Zd, code, half=True, compact=True)]
    ok = None
    for (gx, gz), (wx, wz) in zip(got, want_dev):
        for g, w in ((gx, wx), (gz, wz)):
            assert g.dtype == w.dtype and g.shape == w.shape
            if g.is_floating_point():  # compact f32 images: compare the bit patterns
                g, w = g.view(torch.int32), w.view(torch.int32)
            e = (g == w).all()
            ok = e if ok is None else ok & e
    return ok


def _rank_case(L, rng, n_x, n_z, kind):
    X, Z = _edge_sample(rng, n_x, kind), _edge_sample(rng, n_z, kind)
    code = L.TW_I64 if kind == "i64" else L.TW_F64
    want = [ref_records(X, Z, Z, f) for f in (0, 1, 2, 3)]
    want_dev = [(L.to_device(a), L.to_device(b)) for a, b in want]
    return L.to_device(X), L.to_device(Z), code, want_dev


@pytest.mark.parametrize("kind", ["edge", "i64"])
@pytest.mark.parametrize("n_z", [1, 2, 255, 4097, 40_000])
def test_rank_images_every_small_plan(gpu, n_z, kind):
    """tw_rank_images / tw_rank_images_query under every (sample, z per interval, z per thread)
    of tw_rank_set_small (n_z <= 2^18): the records equal g(v) = #{z < v} (and h, and the
    compact layouts) from np.searchsorted, bit for bit."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    Xd, Zd, code, want_dev = _rank_case(L, np.random.RandomState(n_z), 3001, n_z, kind)
    labels, oks = ["default"], [_rank_all_layouts(L, ops, Xd, Zd, code, want_dev)]
    for plan in HOOKS["tw_rank_set_small"]["values"]:
        assert set_hook(L, "tw_rank_set_small", plan)
        labels.append(plan)
        oks.append(_rank_all_layouts(L, ops, Xd, Zd, code, want_dev))
    assert _failed(labels, oks) == []


@pytest.mark.parametrize("kind", ["edge", "i64"])
def test_rank_images_every_large_plan(gpu, kind):
    """The same under every (sample, z per thread) of tw_rank_set_plan, one element past the
    small-Z gate: n_z = 2^18 + 1."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    Xd, Zd, code, want_dev = _rank_case(L, np.random.RandomState(18), 3001, 2 ** 18 + 1, kind)
    labels, oks = ["default"], [_rank_all_layouts(L, ops, Xd, Zd, code, want_dev)]
    for plan in HOOKS["tw_rank_set_plan"]["values"]:
        assert set_hook(L, "tw_rank_set_plan", plan)
        labels.append(plan)
        oks.append(_rank_all_layouts(L, ops, Xd, Zd, code, want_dev))
    assert _failed(labels, oks) == []


# ------------------------------------------------------------------ D. sorted count
SORTED_NZ = (1, 1023, 1024, 1025, 4096, 4097, 16384, 16385, 20000)
SORTED_NX = (700, 1, 257, 1000, 513, 64, 2000, 300, 1500)


def sorted_inputs(dtype):
    rng = np.random.RandomState(41)
    if dtype == "i64":
        return ([rng.randint(-50, 50, n).astype(np.int64) for n in SORTED_NX],
                [rng.randint(-50, 50, n).astype(np.int64) for n in SORTED_NZ])
    xs = [rng.normal(0, 3, n).round(1) for n in SORTED_NX]
    zs = [rng.normal(0, 3, n).round(1) for n in SORTED_NZ]
    for a in xs + zs:
        if a.size > 16:
            a[1:8] = SPECIALS
    return xs, zs


@pytest.mark.parametrize("dtype", ["f64", "i64"])
def test_sorted_count_every_chunk_and_bucket(gpu, dtype):
    """tw_count_pairs_sorted under every chunk cap (1024 .. 16384) and bucket mode (0, 1, 2), GT
    and HALF, on shards whose nz sit at and around every cap: the seven shards of nz <= 16384
    alone (the bucket path where the mode allows it) and all nine (max_nz = 20000: sorted chunks
    and binary searches, one to twenty chunks per shard).  The workspace is sized again after
    every set.  Reference: np.searchsorted counts."""
    import torch
    from tuplewise import _lib as L
    xs, zs = sorted_inputs(dtype)
    groups = [_Shards(L, xs[:7], zs[:7]), _Shards(L, xs, zs)]
    labels, oks = [], []
    for pred in ("gt", "half"):
        want = np.array([ref_sorted_count(x, z, pred == "half") for x, z in zip(xs, zs)],
                        dtype=np.uint64)
        brute = np.array([ref_count(x, z, pred) for x, z in zip(xs[:4], zs[:4])], dtype=np.uint64)
        assert np.array_equal(want[:4], brute)
        want_dev = L.to_device(want.view(np.int64))
        plans = [None] + _product(HOOKS["tw_count_sorted_set_chunk"]["values"],
                                  HOOKS["tw_count_sorted_set_bucket"]["values"])
        for plan in plans:
            if plan is not None:
                assert set_hook(L, "tw_count_sorted_set_chunk", plan[0])
                assert set_hook(L, "tw_count_sorted_set_bucket", plan[1])
            for sh in groups:
                wb = int(L.lib().tw_count_pairs_sorted_work_bytes(sh.n, sh.max_nz))
                if plan is not None:  # chunks of at most the cap, padded to whole chunks
                    cap = plan[0][0]
                    C = min(cap, max(1024, 1 << (sh.max_nz - 1).bit_length()))
                    assert wb == sh.n * -(-sh.max_nz // C) * C * 8, (plan, wb)
                work = torch.empty(max(wb, 8), dtype=torch.uint8, device="cuda")
                out = torch.full((sh.n,), -1, dtype=torch.int64, device="cuda")
                L.call("tw_count_pairs_sorted", sh.x, sh.xo, sh.z, sh.zo, sh.n, sh.max_nx,
                       sh.max_nz, sh.code, _pred_code(L, pred), work, out, L.stream_handle())
                labels.append((pred, plan, sh.n))
                oks.append((out == want_dev[:sh.n]).all())
        reset_hooks(L)
    assert _failed(labels, oks) == []


def _chain(a, keys):
    """The oracle's permutation chain: the arrays after each repartition."""
    out = []
    for k in keys:
        a = O.permute_scatter(a, int(k))
        out.append(a)
    return out


@pytest.mark.parametrize("dtype", ["f64", "i64"])
def test_sorted_steps_every_chunk(gpu, dtype):
    """One tw_count_pairs_sorted_steps call (T = 3) per chunk cap and bucket mode: every step's
    counts == the np.searchsorted counts on the oracle's permutation chain, the final arrays ==
    the chain's.  The _steps form counts by value buckets only (launch_bucket_count), so the
    chunk cap does not reach it: those calls pin that it stays without effect.  The hook that
    does reach it is tw_count_sorted_set_bucket: 1 and 2 choose the bucket map, and under 0 the
    form does not apply (its work size is 0, as the header says)."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps, prop_swor_layout
    rng = np.random.RandomState(43)
    n, m, N, keys = 5000, 4099, 7, [5, 6, 7]
    X, Z = (rng.randint(-50, 50, n), rng.randint(-50, 50, m)) if dtype == "i64" else \
        (rng.normal(size=n).round(1), rng.normal(size=m).round(1))
    if dtype == "f64":
        X[1:8], Z[1:8] = SPECIALS, SPECIALS
    code = L.TW_I64 if dtype == "i64" else L.TW_F64
    x_off, z_off, _ = prop_swor_layout(n, m, N)
    kx, kz = int(n / N), int((n + m) / N) - int(n / N)
    Xc = _chain(X, [(2 * k) & M64 for k in keys])
    Zc = _chain(Z, [(2 * k + 1) & M64 for k in keys])
    ops = HipOps()
    Xd, Zd, xo, zo = L.to_device(X), L.to_device(Z), L.to_device(x_off), L.to_device(z_off)
    for pred in ("gt", "half"):
        want = np.array([[ref_sorted_count(Xc[t][x_off[s]:x_off[s + 1]],
                                           Zc[t][z_off[s]:z_off[s + 1]], pred == "half")
                          for s in range(N)] for t in range(len(keys))], dtype=np.uint64)
        plans = [None] + _product(HOOKS["tw_count_sorted_set_chunk"]["values"],
                                  HOOKS["tw_count_sorted_set_bucket"]["values"])
        for plan in plans:
            if plan is not None:
                assert set_hook(L, "tw_count_sorted_set_chunk", plan[0])
                assert set_hook(L, "tw_count_sorted_set_bucket", plan[1])
            got = ops.count_sorted_steps(Xd, Zd, xo, zo, N, kx, kz, kx, kz, code,
                                         _pred_code(L, pred), keys)
            if plan is not None and plan[1] == (0,):  # always sort + search: not this form
                assert got is None, (pred, plan)
                continue
            assert got is not None
            out, Xo, Zo = got
            assert np.array_equal(out.cpu().numpy().view(np.uint64), want), (pred, plan)
            assert np.array_equal(Xo.cpu().numpy(), Xc[-1], equal_nan=dtype == "f64")
            assert np.array_equal(Zo.cpu().numpy(), Zc[-1], equal_nan=dtype == "f64")
        reset_hooks(L)


# ------------------------------------------------------------------ E. ranked indexed count
# pairs per shard: none, one, fewer than a 16-B vector of int32 pairs, one 4096-pair tile (1024
# threads x one vector) minus / exactly / plus one, and three of the largest batches (4 vectors
# per thread: 16384 pairs) plus 3
IDX_PAIRS = (0, 1, 7, 4095, 4096, 4097, 3 * 16384 + 3)
IDX_NX = (300, 1, 17, 1000, 513, 64, 700)
IDX_NZ = (200, 5, 9, 999, 64, 700, 513)


def idx_inputs(dtype):
    rng = np.random.RandomState(51)
    if dtype == "i64":
        xs = [rng.randint(-9, 9, n).astype(np.int64) for n in IDX_NX]
        zs = [rng.randint(-9, 9, n).astype(np.int64) for n in IDX_NZ]
    else:
        vals = np.array(SPECIALS + (1.0, 1.0, -1.0, 0.5, 2.5))
        xs = [rng.choice(vals, n) for n in IDX_NX]
        zs = [rng.choice(vals, n) for n in IDX_NZ]
    xo, zo = _offsets(xs), _offsets(zs)
    ix = [xo[s] + rng.randint(0, IDX_NX[s], B) for s, B in enumerate(IDX_PAIRS)]
    iz = [zo[s] + rng.randint(0, IDX_NZ[s], B) for s, B in enumerate(IDX_PAIRS)]
    # a few indices outside their shard's span (allowed: they compare the scores)
    ix[-1][::97] = rng.randint(0, xo[-1], ix[-1][::97].size)
    iz[-1][::89] = rng.randint(0, zo[-1], iz[-1][::89].size)
    return xs, zs, np.concatenate(ix), np.concatenate(iz), _offsets(ix)


def ref_idx_count(X, Z, ix, iz, po, half):
    """A NumPy gather and compare of every shard's pairs."""
    a, b = X[ix], Z[iz]
    w = (a > b).astype(np.int64) + ((a >= b) if half else 0)
    return np.array([w[po[s]:po[s + 1]].sum() for s in range(len(po) - 1)], dtype=np.uint64)


def idx_plans():
    """(codes, variant, idx parts, img parts, img u): the load schedules and blocks per shard of
    the rank-code kernel under the three code builders (sort + search, equal-depth and
    value-range buckets), and the image kernel's vectors per batch (plain and nontemporal) and
    blocks per shard under the default float32 images."""
    plans = [(c[0], v[0], p[0], 0, 9) for c in HOOKS["tw_count_rng_set_codes"]["values"][:3]
             for v in HOOKS["tw_count_idx_set_variant"]["values"]
             for p in HOOKS["tw_count_idx_set_parts"]["values"]]
    plans += [(3, 0, 0, parts, u) for parts, u in HOOKS["tw_count_img_set_plan"]["values"]]
    return plans


@pytest.mark.parametrize("dtype", ["f64", "i64"])
def test_idx_ranked_every_plan(gpu, dtype):
    """tw_count_pairs_idx32_ws under every plan of idx_plans(), GT and HALF, the index tensors
    16-B aligned and sliced one element in (the VEC = false branch of launch_idx_ranked and of
    the image kernel's launcher): counts == a NumPy gather and compare."""
    import torch
    from tuplewise import _engine as E, _lib as L
    xs, zs, ix, iz, po = idx_inputs(dtype)
    sh = _Shards(L, xs, zs)
    pod = L.to_device(po)
    aligned = (L.to_device(ix, np.int32), L.to_device(iz, np.int32))
    pad_x = L.to_device(np.concatenate([[0], ix]), np.int32)
    pad_z = L.to_device(np.concatenate([[0], iz]), np.int32)
    sliced = (pad_x[1:], pad_z[1:])
    assert aligned[0].data_ptr() % 16 == 0 and sliced[0].data_ptr() % 16 == 4
    labels, oks = [], []
    for pred in ("gt", "half"):
        want = ref_idx_count(sh.X, sh.Z, ix, iz, po, pred == "half")
        want_dev = L.to_device(want.view(np.int64))
        # the rank-code kernel applies at these shapes (else the call runs the plain kernel and
        # the variant / parts sweep under codes 0..2 would be hollow)
        assert L.lib().tw_count_pairs_rng_work_bytes(sh.n, sh.max_nx, sh.max_nz, sh.code,
                                                     _pred_code(L, pred)) > 0
        for plan in [None] + idx_plans():
            if plan is not None:
                codes, variant, parts, img_parts, u = plan
                assert set_hook(L, "tw_count_rng_set_codes", (codes,))
                assert set_hook(L, "tw_count_idx_set_variant", (variant,))
                assert set_hook(L, "tw_count_idx_set_parts", (parts,))
                assert set_hook(L, "tw_count_img_set_plan", (img_parts, u))
            for name, (ixd, izd) in (("aligned", aligned), ("sliced", sliced)):
                got = E.count_indexed_ranked_dev(sh.x, sh.xo, sh.z, sh.zo, sh.max_nx, sh.max_nz,
                                                 sh.code, ixd, izd, po, _pred_code(L, pred),
                                                 pair_off_dev=pod)
                labels.append((pred, plan, name))
                oks.append((got == want_dev).all())
        reset_hooks(L)
    assert _failed(labels, oks) == []


# ------------------------------------------------------------------ F. chain emission
# (n_x, n_z, n_shards) per rank: sizes of 1 and 256 * 8 -1 / +0 / +1 (one EPR = 8 tile), a
# ragged pair, and for one process the two bucket layouts that change the kernel: 701 buckets
# (> 512: the unstaged k_chain_emit<EPR, 1, false>) and 101 buckets (8 steps per round x 101 >
# 512: tw_chain_emit halves the steps per round)
CHAIN_SHAPES = [(1, 1, 1), (2047, 2049, 3), (2048, 2048, 4), (2049, 2047, 1), (1, 2048, 2),
                (2049, 1, 2), (5000, 4099, 7)]
CHAIN_SHAPES_ONE = CHAIN_SHAPES + [(5000, 4099, 700), (2048, 2049, 100)]
CHAIN_STEPS = (1, 5, 32)


def _chain_case(G, n_loc, m_loc, N, half):
    """Scores, the oracle's image chain and the reference counts of G ranks x N shards for 32
    steps (shorter emissions use a prefix: the keys are the same)."""
    rng = np.random.RandomState(n_loc + 3 * m_loc + N + G)
    X, Z = rng.normal(0.3, 1, G * n_loc).round(2), rng.normal(0, 1, G * m_loc).round(2)
    keys = list(range(21, 21 + max(CHAIN_STEPS)))
    kxs, kzs = [(2 * k) & M64 for k in keys], [(2 * k + 1) & M64 for k in keys]
    wx, wz = ref_records(X, Z, Z, 3 if half else 2)  # the bag words: images without indices
    wx = wx.view(np.int64 if half else np.int32)
    wz = wz.view(np.int32)
    bags_x, bags_z = np.stack(_chain(wx, kxs)), np.stack(_chain(wz, kzs))
    xs, zs = _chain(X, kxs), _chain(Z, kzs)
    from tuplewise.device import prop_swor_layout
    x_off, z_off, _ = prop_swor_layout(n_loc, m_loc, N)
    counts = np.array([[ref_sorted_count(xs[c][g * n_loc + x_off[s]:g * n_loc + x_off[s + 1]],
                                         zs[c][g * m_loc + z_off[s]:g * m_loc + z_off[s + 1]],
                                         half)
                        for g in range(G) for s in range(N)] for c in range(len(keys))],
                      dtype=np.uint64)
    return X, Z, kxs, kzs, bags_x, bags_z, counts, x_off, z_off


def _positions(base, n, n_total, keys):
    p = np.arange(base, base + n)
    for k in keys:
        p = O.feistel_perm(p, n_total, int(k))
    return p.astype(np.uint32)


def _emit_plans():
    return [None] + HOOKS["tw_chain_set_emit"]["values"]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n,m,N", CHAIN_SHAPES_ONE)
def test_chain_emit_every_plan_one_process(gpu, n, m, N, half):
    """tw_chain_emit into the bags (d_send == NULL) under every (elements per thread, steps per
    round) of tw_chain_set_emit, for 1, 5 and 32 steps: the position arrays equal the oracle's
    Feistel positions, every (step, shard) bag as a sorted array equals the default plan's and
    the oracle chain's, and tw_count_pairs_chain's counts equal the np.searchsorted counts."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    X, Z, kxs, kzs, bags_x, bags_z, counts, x_off, z_off = _chain_case(1, n, m, N, half)
    ops = HipOps()
    Xd, Zd = L.to_device(X), L.to_device(Z)
    xr, zr = ops.rank_images_query(Zd, Xd, Zd, L.TW_F64, half)
    kx, kz = int(n / N), int((n + m) / N) - int(n / N)
    rx, rz = bag_regions(n, kx, N), bag_regions(m, kz, N)
    rxd, rzd = L.to_device(rx), L.to_device(rz)
    xo, zo = L.to_device(x_off), L.to_device(z_off)
    xdt = torch.int64 if half else torch.float32
    labels, oks = [], []
    for T in CHAIN_STEPS:
        want_x = L.to_device(bag_canon(bags_x[:T], rx))
        want_z = L.to_device(bag_canon(bags_z[:T], rz))
        want_c = L.to_device(counts[:T].view(np.int64))
        want_px = L.to_device(_positions(0, n, n, kxs[:T]).view(np.int32))
        want_pz = L.to_device(_positions(0, m, m, kzs[:T]).view(np.int32))
        base = None
        for plan in _emit_plans():
            if plan is not None:
                assert set_hook(L, "tw_chain_set_emit", plan)
            x_bag = torch.full((T, n), -7, dtype=xdt, device="cuda")
            z_bag = torch.full((T, m), -7, dtype=torch.float32, device="cuda")
            xpos = torch.full((n,), -1, dtype=torch.int32, device="cuda")
            zpos = torch.full((m,), -1, dtype=torch.int32, device="cuda")
            cur = torch.empty(T * 2 * (N + 1), dtype=torch.int32, device="cuda")
            ops.chain_emit(xr, zr, half, xpos, zpos, True, 0, 1, kxs[:T], kzs[:T], kx, kz, N,
                           x_bag=x_bag, z_bag=z_bag, cursors=cur)
            out = torch.full((T, N), 7, dtype=torch.int64, device="cuda")
            ops.count_chain(x_bag, xo, z_bag, zo, N, T, n, m, kx, kz, half, out)
            cx = _bag_canon_dev(x_bag if half else x_bag.view(torch.int32), rxd)
            cz = _bag_canon_dev(z_bag.view(torch.int32), rzd)
            ok = (cx == want_x).all() & (cz == want_z).all() & (out == want_c).all() & \
                (xpos == want_px).all() & (zpos == want_pz).all()
            if base is None:
                base = (cx, cz, out)
                # the device's sorted-array form is the NumPy one
                assert np.array_equal(cx.cpu().numpy(), bag_canon(
                    (x_bag if half else x_bag.view(torch.int32)).cpu().numpy(), rx))
            else:
                ok = ok & (cx == base[0]).all() & (cz == base[1]).all() & (out == base[2]).all()
            labels.append((T, plan))
            oks.append(ok)
        reset_hooks(L)
    assert _failed(labels, oks) == []


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("n_loc,m_loc,N", CHAIN_SHAPES)
def test_chain_emit_every_plan_three_ranks(gpu, n_loc, m_loc, N, half):
    """The same with three ranks simulated in one process as in
    test_chain_exchange_simulated_ranks: every rank emits into send buckets (world = 3), the
    all-to-all is done by hand, tw_chain_unpack fills the bags, tw_count_pairs_chain counts
    them.  Per plan: positions == the oracle's, the overflow flag clear, every bag as a sorted
    array == the default plan's == the oracle chain's, counts == np.searchsorted's; and with a
    capacity of one record the flag is raised under every plan."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    G = 3
    X, Z, kxs, kzs, bags_x, bags_z, counts, x_off, z_off = _chain_case(G, n_loc, m_loc, N, half)
    ops = HipOps()
    Zall, Xall = L.to_device(Z), L.to_device(X)
    recs = []
    for r in range(G):
        xq, zq = Xall[r * n_loc:(r + 1) * n_loc], Zall[r * m_loc:(r + 1) * m_loc]
        recs.append(ops.rank_images_query(Zall, xq, zq, L.TW_F64, half))
    kx, kz = int(n_loc / N), int((n_loc + m_loc) / N) - int(n_loc / N)
    rx, rz = bag_regions(n_loc, kx, N), bag_regions(m_loc, kz, N)
    rxd, rzd = L.to_device(rx), L.to_device(rz)
    xo, zo = L.to_device(x_off), L.to_device(z_off)
    tot = n_loc + m_loc
    cap = tot // G + tot // (8 * G) + 1024
    W = 2 if half else 1
    xdt = torch.int64 if half else torch.float32
    labels, oks = [], []
    for T in CHAIN_STEPS:
        want = []
        for r in range(G):
            a, b = slice(r * n_loc, (r + 1) * n_loc), slice(r * m_loc, (r + 1) * m_loc)
            want.append((L.to_device(bag_canon(bags_x[:T, a], rx)),
                         L.to_device(bag_canon(bags_z[:T, b], rz)),
                         L.to_device(counts[:T, r * N:(r + 1) * N].view(np.int64)),
                         L.to_device(_positions(r * n_loc, n_loc, G * n_loc,
                                                kxs[:T]).view(np.int32)),
                         L.to_device(_positions(r * m_loc, m_loc, G * m_loc,
                                                kzs[:T]).view(np.int32))))
        base = None
        for plan in _emit_plans():
            if plan is not None:
                assert set_hook(L, "tw_chain_set_emit", plan)
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            sends, ok = [], None
            for r in range(G):
                xpos = torch.full((n_loc,), -1, dtype=torch.int32, device="cuda")
                zpos = torch.full((m_loc,), -1, dtype=torch.int32, device="cuda")
                send = torch.empty(G * T * (cap + 1) * W, dtype=torch.int64, device="cuda")
                ops.chain_emit(recs[r][0], recs[r][1], half, xpos, zpos, True, r, G, kxs[:T],
                               kzs[:T], kx, kz, N, send=send, cap=cap, flag=flag)
                e = (xpos == want[r][3]).all() & (zpos == want[r][4]).all()
                ok = e if ok is None else ok & e
                sends.append(send.view(G, -1))
            got = []
            for r in range(G):
                recv = torch.cat([sends[g][r] for g in range(G)])
                x_bag = torch.full((T, n_loc), -7, dtype=xdt, device="cuda")
                z_bag = torch.full((T, m_loc), -7, dtype=torch.float32, device="cuda")
                ops.chain_unpack(recv, G, T, cap, half, n_loc, m_loc, x_bag, z_bag, flag, kx, kz,
                                 N)
                out = torch.full((T, N), 7, dtype=torch.int64, device="cuda")
                ops.count_chain(x_bag, xo, z_bag, zo, N, T, n_loc, m_loc, kx, kz, half, out)
                cx = _bag_canon_dev(x_bag if half else x_bag.view(torch.int32), rxd)
                cz = _bag_canon_dev(z_bag.view(torch.int32), rzd)
                ok = ok & (cx == want[r][0]).all() & (cz == want[r][1]).all() & \
                    (out == want[r][2]).all()
                got.append((cx, cz, out))
            ok = ok & (flag == 0).all()
            if base is None:
                base = got
            else:
                for (a, b, c), (a0, b0, c0) in zip(got, base):
                    ok = ok & (a == a0).all() & (b == b0).all() & (c == c0).all()
            if tot >= 16:  # a capacity of one record: some bucket overflows, the flag says so
                over = torch.zeros(1, dtype=torch.int32, device="cuda")
                xpos = torch.empty(n_loc, dtype=torch.int32, device="cuda")
                zpos = torch.empty(m_loc, dtype=torch.int32, device="cuda")
                send = torch.empty(G * T * 2 * W, dtype=torch.int64, device="cuda")
                ops.chain_emit(recs[0][0], recs[0][1], half, xpos, zpos, True, 0, G, kxs[:T],
                               kzs[:T], kx, kz, N, send=send, cap=1, flag=over)
                ok = ok & (over == 1).all()
            labels.append((T, plan))
            oks.append(ok)
        reset_hooks(L)
    assert _failed(labels, oks) == []


# ------------------------------------------------------------------ G. exchange kernels
@pytest.mark.parametrize("G,n_loc,m_loc", [(3, 20_011, 7_003), (2, 1, 1)])
def test_exchange_kernels_every_grid(gpu, G, n_loc, m_loc):
    """The bodies of test_exchange_kernels_simulated_ranks, test_fused_exchange_kernels_
    simulated_ranks and test_fixed_exchange_kernels_simulated_ranks (tests/test_gpu_parity.py)
    under every grid cap of tw_exchange_set_grid: with 1 block every grid-stride loop does all
    the work, with 1000 the cap never binds."""
    import test_gpu_parity as P
    from tuplewise import _lib as L
    for grid in HOOKS["tw_exchange_set_grid"]["values"]:
        assert set_hook(L, "tw_exchange_set_grid", grid)
        P.exchange_kernels_body(G, n_loc)
        P.fused_exchange_kernels_body(G, n_loc, m_loc)
        P.fixed_exchange_kernels_body(G, n_loc, m_loc)
