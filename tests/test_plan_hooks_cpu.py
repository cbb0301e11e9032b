"""The launch-plan sweep's bookkeeping, without a GPU (tests/test_gpu_plan_sweep.py):

  * inventory: every `int tw_*set_*(` of include/tuplewise.h is swept there or exempt here with
    a reason, so a hook added later without a sweep fails;
  * the setters take every table value and refuse values outside their documented sets;
  * the sweep's NumPy references against triple-loop brute force at sizes of a few dozen,
    special values included;
  * the sweep's count inputs: every boundary element takes part in a counted pair.
"""
import pathlib
import re

import numpy as np
import pytest

import test_gpu_plan_sweep as S
from oracle import oracle as O

ROOT = pathlib.Path(__file__).resolve().parents[1]

# hooks the sweep leaves out: deadlines, or hooks with a sweep of their own (the test file that
# holds it; checked below to name the hook)
EXEMPT = {
    "tw_comm_set_timeout": "a deadline, not a launch plan",
    "tw_comm_set_prior_timeout": "a deadline, not a launch plan",
    "tw_count_chain_set_plan": "tests/test_gpu_count_bits.py",
    "tw_count_chain_set_swap": "tests/test_gpu_count_planes.py",
    "tw_count_chain_set_class_bits": "tests/test_gpu_count_classes.py",
    "tw_pair_moments_set_algo": "tests/test_gpu_moments.py",
    "tw_hinge_set_variant": "tests/test_gpu_parity.py",
    "tw_gemv_set_variant": "tests/test_gpu_parity.py",
    "tw_pair_grad_complete_set_search": "tests/test_gpu_parity.py",
    "tw_shuffle_swaps_set_rounds": "tests/test_gpu_devshuffle.py",
    "tw_shuffle_swaps_set_tail": "tests/test_gpu_devshuffle.py",
    "tw_count_rng_img_set_unroll": "tests/test_gpu_parity.py",
}


def header_hooks():
    text = (ROOT / "include" / "tuplewise.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^\s*int\s+(tw_\w*set_\w+)\s*\(", text, re.M)))


def test_every_hook_is_swept_or_exempt():
    names = header_hooks()
    assert len(names) >= 27
    for n in names:
        assert (n in S.HOOKS) != (n in EXEMPT), f"{n}: add it to the sweep's HOOKS table"
    assert set(S.HOOKS) <= set(names) and set(EXEMPT) <= set(names)
    for n, why in EXEMPT.items():
        if why.startswith("tests/"):  # swept elsewhere: that file sets the hook
            assert f'"{n}"' in (ROOT / why).read_text(), (n, why)
    for n, h in S.HOOKS.items():
        assert h["values"] and all(len(v) == len(h["default"]) for v in h["values"]), n


def test_setters_take_the_table_and_refuse_the_rest(tw):
    L = tw._lib
    try:
        for n, h in S.HOOKS.items():
            for v in h["values"]:
                S.set_hook(L, n, v)
            L.call(n, *h["default"])
        for n, bad in [("tw_count_set_plan", (3, 0)), ("tw_count_set_plan", (1, -1)),
                       ("tw_count_set_scalar_mix", (2,)), ("tw_count_step_set_plan", (8, 12, 1)),
                       ("tw_count_step_set_plan", (8, 8, 2)), ("tw_count_rank_set_plan", (4, 0)),
                       ("tw_count_rank_set_next", (2,)), ("tw_rank_set_plan", (256, 8)),
                       ("tw_rank_set_small", (128, 2048, 4)), ("tw_rank_set_small", (256, 4096, 4)),
                       ("tw_count_sorted_set_chunk", (3000,)), ("tw_count_sorted_set_chunk", (512,)),
                       ("tw_count_sorted_set_bucket", (3,)), ("tw_count_idx_set_variant", (6,)),
                       ("tw_count_idx_set_parts", (-1,)), ("tw_count_img_set_plan", (0, 3)),
                       ("tw_count_rng_set_codes", (4,)), ("tw_chain_set_emit", (4, 2)),
                       ("tw_chain_set_emit", (3, 1)), ("tw_exchange_set_grid", (-1,))]:
            with pytest.raises(ValueError):
                L.call(n, *bad)
    finally:
        S.reset_hooks(L)


# ------------------------------------------------------------------ reference self-checks
VALS_F = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 1.0, 1.0, -1.5, 2.5])
VALS_I = np.array([2 ** 63 - 1, -(2 ** 63), 2 ** 62, -(2 ** 62), 0, 1, -1, 7, 7], dtype=np.int64)


def _samples():
    rng = np.random.RandomState(3)
    return [(rng.choice(VALS_F, 37), rng.choice(VALS_F, 29)),
            (rng.choice(VALS_I, 31), rng.choice(VALS_I, 41)),
            (rng.choice(VALS_F, 5), np.zeros(0)), (np.zeros(0, np.int64), rng.choice(VALS_I, 3))]


def _wrap(d):
    return (d + 2 ** 63) % 2 ** 64 - 2 ** 63


def test_count_references_against_brute_force():
    for x, z in _samples():
        gt = half = sub = 0
        for a in x.tolist():
            for b in z.tolist():
                gt += a > b
                half += 2 * (a > b) + (a == b)
                sub += (_wrap(a - b) > 0) if x.dtype == np.int64 else (a > b)
        assert S.ref_count(x, z, "gt") == gt
        assert S.ref_count(x, z, "half") == half
        assert S.ref_count(x, z, "subgt") == sub
        assert S.ref_sorted_count(x, z, False) == gt
        assert S.ref_sorted_count(x, z, True) == half
        px, pz = S.participation(x, z, "half")
        assert px.tolist() == [any(a >= b for b in z.tolist()) for a in x.tolist()]
        assert pz.tolist() == [any(a >= b for a in x.tolist()) for b in z.tolist()]
    x, z = _samples()[1]
    assert S.ref_count(x, z, "subgt") != S.ref_count(x, z, "gt")  # the sample does wrap


def test_idx_reference_against_brute_force():
    rng = np.random.RandomState(4)
    x, z = rng.choice(VALS_F, 23), rng.choice(VALS_F, 19)
    ix, iz = rng.randint(0, 23, 50), rng.randint(0, 19, 50)
    po = np.array([0, 0, 13, 50])
    xl, zl = x.tolist(), z.tolist()
    for half in (False, True):
        want = [sum(int(xl[i] > zl[j]) + int(half and xl[i] >= zl[j]) for i, j in
                    zip(ix[a:b].tolist(), iz[a:b].tolist())) for a, b in zip(po[:-1], po[1:])]
        assert S.ref_idx_count(x, z, ix, iz, po, half).tolist() == want


def test_image_reference_against_brute_force():
    for x, z in _samples()[:2]:
        zl = [b for b in z.tolist() if b == b]  # NaN z are below nothing
        for side, op in (("left", lambda b, a: b < a), ("right", lambda b, a: b <= a)):
            want = [len(zl) if a != a else sum(op(b, a) for b in zl) for a in x.tolist()]
            assert S.ref_images(x, z, side).tolist() == want
        # the record layouts, against the oracle's restatement of tw_rank_images(_query)
        for flags in (0, 1):
            wx, wz = O.rank_records(x, z, half=bool(flags))
            gx, gz = S.ref_records(x, z, z, flags)
            assert np.array_equal(gx, wx) and np.array_equal(gz, wz)
        cx, cz = S.ref_records(x, z, z, 2)
        px, _ = S.ref_records(x, z, z, 3)
        low = np.uint64(0xFFFFFFFF)
        assert np.array_equal(cx.view(np.uint32), (wx.view(np.uint64) & low).astype(np.uint32))
        assert np.array_equal(cz.view(np.uint32), (wz.view(np.uint64) & low).astype(np.uint32))
        assert np.array_equal(px, wx)  # half records are the {g, h} pairs
        if x.dtype.kind == "f":
            assert (cx[np.isnan(x)] == np.float32(-2.0 ** 25)).all()


def test_bag_comparison_against_brute_force():
    rng = np.random.RandomState(5)
    n, k, N, T = 47, 9, 4, 3  # four shards of 9 and a tail of 11
    region = S.bag_regions(n, k, N)
    assert region.tolist() == [min(p // k, N) for p in range(n)]
    assert S.bag_regions(5, 0, 2).tolist() == [2] * 5
    bags = rng.randint(-5, 5, (T, n)).astype(np.int32)
    canon = S.bag_canon(bags, region)
    for c in range(T):
        for b in range(N + 1):
            sel = [p for p in range(n) if region[p] == b]
            assert canon[c, sel].tolist() == sorted(bags[c, sel].tolist())
    shuffled = bags.copy()
    for c in range(T):
        for b in range(N + 1):
            sel = np.flatnonzero(region == b)
            shuffled[c, sel] = bags[c, rng.permutation(sel)]
    assert np.array_equal(S.bag_canon(shuffled, region), canon)
    moved = bags.copy()
    moved[1, [0, n - 1]] = [bags[1, 0] + 100, bags[1, n - 1]]  # one bag's multiset changes
    assert not np.array_equal(S.bag_canon(moved, region), canon)
    swapped = bags.copy()
    swapped[2, 0], swapped[2, n - 1] = 50, -50
    crossed = swapped.copy()
    crossed[2, 0], crossed[2, n - 1] = -50, 50  # the same row multiset, other bags
    assert not np.array_equal(S.bag_canon(swapped, region), S.bag_canon(crossed, region))


# ------------------------------------------------------------------ the count inputs
def test_boundary_positions():
    assert S.boundary_positions(0, (8,)) == []
    assert S.boundary_positions(8, (8,)) == [7]
    assert S.boundary_positions(9, (8,)) == [7, 8]
    assert S.boundary_positions(20, (5, 8)) == [4, 5, 7, 8, 9, 10, 14, 15, 16, 19]


@pytest.mark.parametrize("dtype,pred", sorted(S.COUNT_KINDS))
def test_count_inputs_boundary_elements_take_part(dtype, pred):
    """count_inputs() feeds the complete count, the fused step and (kinds f64 and i64, strict
    predicate) the rank step of the sweep.  For every swept (R, z_chunk) — tw_count_set_plan's
    and tw_count_rank_set_plan's — the last x and z of every shard, the z on each side of every
    chunk boundary and the x on each side of every 64 R tile boundary take part in at least one
    counted pair (from the reference alone): a dropped tail or a chunk off by one would change
    a count."""
    xs, zs = S.count_inputs(S.COUNT_KINDS[dtype, pred])
    assert tuple(map(len, xs)) == S.SHARD_NX and tuple(map(len, zs)) == S.SHARD_NZ
    assert 0 in S.SHARD_NX and 0 in S.SHARD_NZ and {1, 63, 64, 65, 511, 513} <= set(S.SHARD_NX)
    plans = [(64 * R, zc) for R, zc in S.HOOKS["tw_count_set_plan"]["values"]]
    plans += [(64 * R, zc) for R, zc in S.HOOKS["tw_count_rank_set_plan"]["values"]]
    checked = 0
    for x, z in zip(xs, zs):
        if not (x.size and z.size):
            continue
        px, pz = S.participation(x, z, pred)
        for tile, zc in plans:
            bx = S.boundary_positions(x.size, (tile,))
            bz = S.boundary_positions(z.size, (zc,) if zc else ())
            assert px[bx].all() and pz[bz].all(), (x.size, z.size, tile, zc)
            assert set(bx) <= set(S.boundary_positions(x.size, S.X_TILES))
            assert set(bz) <= set(S.boundary_positions(z.size, S.Z_STEPS))
            checked += len(bx) + len(bz)
    assert checked > 1000
    if dtype == "f64":  # the special values sit in valid lanes of x and of z
        big_x, big_z = xs[7], zs[7]
        for v in S.SPECIALS:
            same = (lambda a: np.isnan(a)) if v != v else \
                (lambda a: (a == v) & (np.signbit(a) == np.signbit(v)))
            assert same(big_x).any() and same(big_z).any()
        assert np.isnan(big_x[1090])  # in the last, ragged tile of every R
    if S.COUNT_KINDS[dtype, pred] == "i64wrap":
        x, z = xs[7], zs[7]
        assert S.ref_count(x, z, "subgt") != S.ref_count(x, z, "gt")
