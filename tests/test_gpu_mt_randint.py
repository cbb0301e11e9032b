"""NumPy-order randint streams drawn on the device (csrc/mtdraw.hip, numpy_rng.randint_device;
DESIGN §4.4c).  Every case makes the same calls with np.random.randint from the same state and
asserts: the int32 values and offsets are NumPy's, np.random.get_state() is equal afterwards
(key, pos and the gauss fields), and DEVICE_DRAWS_STATS shows the device path ran.  Small
stream_blocks / round_words put sub-stream, key-block and round boundaries inside small inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SB = 2  # key blocks per sub-stream in the tests: 1248 words


def _set_start(seed, pos):
    """A state at the given pos: 624 = a fresh seed; else a regenerated key moved to pos."""
    np.random.seed(seed)
    if pos != 624:
        np.random.randint(0, 2 ** 32, 1, dtype=np.uint32)
        st = np.random.get_state()
        np.random.set_state((st[0], st[1], pos, st[3], st[4]))


def _check(calls, add=None, seed=1, pos=624, state=None, **kw):
    from tuplewise import numpy_rng as R
    kw.setdefault("stream_blocks", SB)
    if state is None:
        _set_start(seed, pos)
    else:
        np.random.set_state(state)
    st0 = np.random.get_state()
    adds = [0] * len(calls) if add is None else add
    want = [np.random.randint(lo, hi, n) + a for (lo, hi, n), a in zip(calls, adds)]
    st_want = np.random.get_state()
    np.random.set_state(st0)
    before = dict(R.DEVICE_DRAWS_STATS)
    got = R.randint_device(calls, add, **kw)
    assert got is not None, "the device path refused a supported batch"
    out, offs = got
    st_got = np.random.get_state()
    draws = any(n > 0 and hi - lo > 1 for lo, hi, n in calls)
    assert R.DEVICE_DRAWS_STATS["calls"] == before["calls"] + len(calls)
    assert (R.DEVICE_DRAWS_STATS["rounds"] > before["rounds"]) == draws
    assert str(out.dtype) == "torch.int32" and out.is_cuda
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum([c[2] for c in calls])]))
    flat = np.concatenate(want) if want else np.zeros(0, np.int64)
    assert np.array_equal(out.cpu().numpy().astype(np.int64), flat)
    assert st_got[0] == st_want[0] and st_got[2] == st_want[2], (st_got[2], st_want[2])
    assert np.array_equal(st_got[1], st_want[1])
    assert st_got[3] == st_want[3] and st_got[4] == st_want[4]
    return R.DEVICE_DRAWS_STATS["rounds"] - before["rounds"]


@pytest.mark.parametrize("n", [1, 7, 600])
def test_tiny_single_call(gpu, n):
    _check([(0, 15625, n)], seed=3)


def test_boundary_spans(gpu):
    """5e4 draws over ~40 sub-streams; call boundaries inside a group and a key block."""
    _check([(0, 15625, 20_011), (0, 15625, 13), (0, 15625, 29_976)], seed=4)


@pytest.mark.parametrize("pos", [0, 1, 623, 624])
def test_starting_pos(gpu, pos):
    _check([(0, 15625, 3000), (0, 15625, 1000)], seed=5, pos=pos)


def test_starting_pos_zero_of_a_seeded_key(gpu):
    """pos 0 on a key that was never regenerated: NumPy tempers key[0] as it stands."""
    st = np.random.RandomState(6).get_state()
    _check([(0, 65536, 2000)], state=(st[0], st[1], 0, st[3], st[4]))


@pytest.mark.parametrize("bound", [2, 4096, 16385, 15625, 2 ** 31 - 1])
def test_bounds(gpu, bound):
    _check([(0, bound, 5000)], seed=bound % 1000)


def test_full_width_range(gpu):
    _check([(-2 ** 31, 2 ** 31 - 1, 4000)], seed=8)


def test_constant_and_empty_calls(gpu):
    _check([(0, 15625, 2000), (7, 8, 300), (0, 15625, 0), (0, 15625, 1500)], seed=9)
    _check([(5, 6, 10)], seed=9)  # no draw at all: the state is untouched
    _check([], seed=9)


def test_alternating_bounds(gpu):
    calls = [(0, 1000 if c % 2 == 0 else 70000, 3000) for c in range(16)]
    _check(calls, seed=10)


def test_four_configurations_and_refusal_of_five(gpu):
    from tuplewise import numpy_rng as R
    bounds = [1000, 70000, 15625, 3]
    _check([(0, bounds[c % 4], 1500 + c) for c in range(12)], seed=11)
    np.random.seed(11)
    st = np.random.get_state()
    assert R.randint_device([(0, b, 100) for b in bounds + [300_000]], stream_blocks=SB) is None
    assert np.array_equal(np.random.get_state()[1], st[1]) and np.random.get_state()[2] == st[2]


def test_low_and_add(gpu):
    _check([(-50, 1200, 2500), (10, 15635, 2500), (-2 ** 31, -2 ** 31 + 9, 100)],
           add=[1_000_000, -10, 0], seed=12)
    _check([(0, 100, 500)], add=[2 ** 31 - 100], seed=12)


def test_one_call_over_three_rounds(gpu):
    rounds = _check([(0, 16385, 3500)], seed=13, round_words=2 * 624 * SB)
    assert rounds >= 3


def test_round_ending_on_a_calls_last_word(gpu):
    """Every word accepted: from a fresh seed the first round's buffer (2 sub-streams) serves
    words 624 .. 2495, exactly the first call; the second call starts the next round."""
    rounds = _check([(0, 65536, 2 * 624 * SB - 624), (0, 65536, 500)], seed=14,
                    round_words=2 * 624 * SB)
    assert rounds == 2


def _counts_ending(seed, bound, want):
    """The first cnt >= 1500 after which want(blocks regenerated, pos) holds for
    np.random.randint(0, bound, cnt) from seed(seed)."""
    rs = np.random.RandomState(seed)
    rs.randint(0, bound, 1499)
    for cnt in range(1500, 12000):
        rs.randint(0, bound, 1)
        p = rs.get_state()[2]
        if want(_block_of(rs, seed), p):
            return cnt
    raise AssertionError("no such count")


def _block_of(rs, seed):
    """Index (in key blocks after the seeded key) of the block NumPy's key holds."""
    ref = np.random.RandomState(seed)
    key = rs.get_state()[1]
    for b in range(1, 40):
        ref.randint(0, 2 ** 32, 624, dtype=np.uint32)
        if np.array_equal(ref.get_state()[1], key):
            return b
    raise AssertionError("key block not found")


@pytest.mark.parametrize("which", ["pos624", "pos624_first_block_of_substream",
                                   "mid_first_block_of_substream"])
def test_final_state_at_block_and_substream_boundaries(gpu, which):
    """pos == 624 after the last draw (no regeneration yet), and consumed words that end inside
    the first key block of a sub-stream (block index even at SB = 2): no regeneration follows the
    sub-stream's starting state, so its word 0 must be the true sequence word."""
    want = {"pos624": lambda b, p: p == 624 and b % SB == 1,
            "pos624_first_block_of_substream": lambda b, p: p == 624 and b % SB == 0,
            "mid_first_block_of_substream": lambda b, p: 100 < p < 500 and b % SB == 0}[which]
    cnt = _counts_ending(21, 15625, want)
    _check([(0, 15625, cnt)], seed=21)


@pytest.mark.parametrize("S", [1, 2, 3, 64])
def test_state_tables_against_host_jumps(gpu, S):
    """Row 0 is the key; row k is the window one word before sub-stream k: words 1..623 and one
    recurrence step make the key block mt_jumped gives for the same offset."""
    from tuplewise import numpy_rng as R
    key = np.random.RandomState(31).get_state()[1]
    tab = R.mt_states(key, S, SB).cpu().numpy().view(np.uint32)
    assert tab.shape == (S, 624) and np.array_equal(tab[0], key)
    Lw = 624 * SB
    for k in range(1, S):
        blk, pos = R.mt_jumped(key, 624, k * Lw - 624 + 1)  # NumPy's key block x[kL ..], pos 1
        assert pos == 1
        u = tab[k]
        assert np.array_equal(u[1:], blk[:623]), k
        y = (u[0] & np.uint32(0x80000000)) | (u[1] & np.uint32(0x7fffffff))
        last = u[397] ^ (y >> np.uint32(1)) ^ (np.uint32(0x9908b0df) if y & 1 else np.uint32(0))
        assert last == blk[623], k


def test_default_stream_length(gpu):
    _check([(0, 15625, 200_000), (0, 15625, 100_000)], seed=41, stream_blocks=None)


# ------------------------------------------------------------------------------ the drop-in
def _dropin(fn, X0, Z0, on, seed=77):
    from tuplewise import _blocks as Bk
    from tuplewise import numpy_rng as R
    X, Z = X0.copy(), Z0.copy()
    np.random.seed(seed)
    old, before = (Bk.DEVICE_DRAWS, Bk.DEVICE_DRAWS_MIN), R.DEVICE_DRAWS_STATS["rounds"]
    Bk.DEVICE_DRAWS, Bk.DEVICE_DRAWS_MIN = on, 1 << 20  # (these calls draw 2.4e6 a repetition)
    try:
        v = fn(X, Z)
    finally:
        Bk.DEVICE_DRAWS, Bk.DEVICE_DRAWS_MIN = old
    return v, X, Z, np.random.get_state(), R.DEVICE_DRAWS_STATS["rounds"] - before


@pytest.fixture(scope="module")
def samples():
    rng = np.random.RandomState(123)
    return rng.normal(0.4, 1, 70_000), rng.normal(0, 1, 90_001)


@pytest.mark.parametrize("kernel", ["AUC", "gini"])
@pytest.mark.parametrize("m", [70_000, 90_001])
@pytest.mark.parametrize("est", ["UnNB", "UnNBT"])
def test_dropin_device_draws_equal_host_draws_and_oracle(gpu, samples, est, m, kernel):
    import tuplewise.compute_stats as cs
    from oracle import oracle as O
    X0, Z0 = samples[0], samples[1][:m]
    if est == "UnNB":
        fn = lambda X, Z: cs.UnNB(X, Z, 4, 300_000, "prop-SWOR", kernel=kernel)
        ref = lambda X, Z: O.cs_UnNB(X, Z, 4, 300_000, "prop-SWOR", kernel=kernel)
    else:
        fn = lambda X, Z: cs.UnNBT(X, Z, 4, 300_000, 2, "prop-SWOR", kernel=kernel)
        ref = lambda X, Z: O.cs_UnNBT(X, Z, 4, 300_000, 2, "prop-SWOR", kernel=kernel)
    v_on, X_on, Z_on, st_on, r_on = _dropin(fn, X0, Z0, True)
    v_off, X_off, Z_off, st_off, r_off = _dropin(fn, X0, Z0, False)
    assert r_on >= 1 and r_off == 0
    assert v_on == v_off
    assert np.array_equal(X_on, X_off) and np.array_equal(Z_on, Z_off)
    assert st_on[2] == st_off[2] and np.array_equal(st_on[1], st_off[1])
    assert st_on[3:] == st_off[3:]
    Xo, Zo = X0.copy(), Z0.copy()
    np.random.seed(77)
    want = ref(Xo, Zo)
    assert v_on == want if kernel == "AUC" else np.isclose(v_on, want, rtol=1e-12, atol=0)
    assert np.array_equal(X_on, Xo) and np.array_equal(Z_on, Zo)
    assert np.array_equal(np.random.get_state()[1], st_on[1])


def test_large_golden_unnbt_runs_on_the_device_draws(gpu):
    """The reference's own cs.UnNBT run at 1e6 per class (tests/golden/golden_large.json) with
    the default settings: the device draws serve it (2 repetitions of 128 calls), and value, RNG
    probe and the shuffled arrays are the reference's."""
    import hashlib
    import json
    import pathlib
    import sys
    import tuplewise.compute_stats as cs
    from tuplewise import numpy_rng as R
    here = pathlib.Path(__file__).resolve().parent / "golden"
    sys.path.insert(0, str(here))
    from shapes import large_inputs
    spec = next(c for c in json.loads((here / "golden_large.json").read_text())["cases"]
                if c["call"] == "cs.UnNBT")
    X, Z = large_inputs(spec)
    before = dict(R.DEVICE_DRAWS_STATS)
    np.random.seed(spec["rng_seed"])
    got = cs.UnNBT(X, Z, spec["N"], spec["B"], spec["T"], spec["sampling"], kernel="AUC")
    assert R.DEVICE_DRAWS_STATS["rounds"] >= before["rounds"] + spec["T"]
    assert R.DEVICE_DRAWS_STATS["calls"] == before["calls"] + 2 * spec["N"] * spec["T"]
    assert int(np.random.randint(0, 2 ** 31 - 1)) == spec["probe"]
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    assert sha(X) == spec["sha_X_after"] and sha(Z) == spec["sha_Z_after"]
    assert float(got).hex() == spec["value_hex"]


def test_dropin_swor_keeps_the_host_path(gpu, samples):
    import tuplewise.compute_stats as cs
    X0, Z0 = samples[0], samples[1][:70_000]
    fn = lambda X, Z: cs.UnNB(X, Z, 4, 300_000, "SWOR", kernel="AUC")
    v_on, X_on, Z_on, st_on, r_on = _dropin(fn, X0, Z0, True)
    v_off, X_off, Z_off, st_off, r_off = _dropin(fn, X0, Z0, False)
    assert r_on == 0 and r_off == 0 and v_on == v_off
    assert np.array_equal(X_on, X_off) and np.array_equal(st_on[1], st_off[1])


def test_host_path_incomplete_draw(gpu):
    """Incomplete.draw on the host path: the values and state of two np.random.randint calls,
    and np.random.randint itself under a global generator that is not the legacy MT19937."""
    from tuplewise import _blocks as Bk
    spec = Bk.Incomplete(5000, "AUC")
    np.random.seed(51)
    ix, iz = spec.draw(15625, 15000)
    st = np.random.get_state()
    np.random.seed(51)
    wx, wz = np.random.randint(0, 15625, 5000), np.random.randint(0, 15000, 5000)
    assert ix.dtype == wx.dtype and np.array_equal(ix, wx) and np.array_equal(iz, wz)
    assert st[2] == np.random.get_state()[2] and np.array_equal(st[1], np.random.get_state()[1])
    old = np.random.get_bit_generator()
    np.random.set_bit_generator(np.random.PCG64(5))
    try:
        ix, iz = spec.draw(100, 90)
    finally:
        np.random.set_bit_generator(old)
    chk = np.random.RandomState(np.random.PCG64(5))
    assert np.array_equal(ix, chk.randint(0, 100, 5000))
    assert np.array_equal(iz, chk.randint(0, 90, 5000))
