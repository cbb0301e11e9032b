"""MT19937 jump-ahead on the host (csrc/mtjump.cpp, numpy_rng.mt_jump_poly / mt_jumped; DESIGN
§4.4c): the minimal polynomial, the power polynomials' additivity, and the jumped state against
NumPy itself — key and pos of get_state() after drawing J words.  No GPU needed."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"

JUMPS = [1, 623, 624, 625, 65520, 2 * 65520 + 17, 10 ** 6]


def _degree(p):
    bits = np.unpackbits(p.view(np.uint8), bitorder="little")
    return int(np.nonzero(bits)[0][-1])


def test_minpoly_degree_and_reproducible(tw):
    from tuplewise import numpy_rng as R
    phi = R.mt_minpoly()
    assert phi.shape == (312,) and phi.dtype == np.uint64
    assert _degree(phi) == 19937 and int(phi[0]) & 1
    assert np.array_equal(phi, R.mt_minpoly())
    assert _degree(R.mt_jump_poly(5)) == 5 and _degree(R.mt_jump_poly(0)) == 0
    assert _degree(R.mt_jump_poly(19937)) < 19937
    assert R.mt_jump_poly(10 ** 6) is R.mt_jump_poly(10 ** 6)  # cached


def _start_states():
    """(label, state tuple): a fresh seed (pos 624: key[0] is not a sequence word) and
    regenerated keys at pos 0, 1 and 623."""
    out = []
    rs = np.random.RandomState(20240)
    out.append(("fresh", rs.get_state()))
    for pos in (0, 1, 623):
        rs = np.random.RandomState(100 + pos)
        rs.randint(0, 2 ** 32, 1, dtype=np.uint32)  # regenerates: key[0] is a true word
        st = rs.get_state()
        out.append((f"pos{pos}", (st[0], st[1], pos, st[3], st[4])))
    return out


@pytest.mark.parametrize("J", JUMPS + [624 * 3, 624 * 1603])
@pytest.mark.parametrize("label,state", _start_states(), ids=lambda v: v if isinstance(v, str) else "")
def test_host_jump_against_numpy(tw, label, state, J):
    """J = 624 q from a fresh seed is the word-0 case: no regeneration follows the jump, so
    key[0] must come out as the true sequence word."""
    from tuplewise import numpy_rng as R
    rs = np.random.RandomState(0)
    rs.set_state(state)
    rs.randint(0, 2 ** 32, J, dtype=np.uint32)
    want = rs.get_state()
    key0 = state[1].copy()
    key, pos = R.mt_jumped(state[1], state[2], J)
    assert pos == want[2]
    assert np.array_equal(key, want[1])
    assert np.array_equal(state[1], key0)  # the argument is not advanced


def test_jump_refuses_bad_arguments(tw):
    from tuplewise import numpy_rng as R
    key = np.random.RandomState(1).get_state()[1]
    with pytest.raises(ValueError):
        R.mt_jumped(key, 625, 1)
    with pytest.raises(ValueError):
        R.mt_jumped(key, 0, -1)
    with pytest.raises(ValueError):
        R.mt_jumped(key[:100], 0, 1)
    with pytest.raises(ValueError):
        R.mt_jump_poly(-3)
    with pytest.raises(ValueError):
        R.mt_poly_mul(R.mt_minpoly(), R.mt_jump_poly(1))  # phi itself is not reduced


def test_power_polynomials_are_additive(tw):
    from tuplewise import numpy_rng as R
    rng = np.random.RandomState(5)
    for _ in range(6):
        a, b = (int(v) for v in rng.randint(0, 2 ** 40, 2))
        assert np.array_equal(R.mt_poly_mul(R.mt_jump_poly(a), R.mt_jump_poly(b)),
                              R.mt_jump_poly(a + b))
    one = R.mt_jump_poly(0)
    assert np.array_equal(R.mt_poly_mul(one, R.mt_jump_poly(12345)), R.mt_jump_poly(12345))


def test_device_entries_validate_before_touching_a_device(tw):
    """No GPU here: bad arguments are refused first, and what randint_device does not serve
    returns None with nothing drawn."""
    from tuplewise import numpy_rng as R
    L = tw._lib
    lib = L.lib()
    with pytest.raises(ValueError, match="tw_mt_states"):
        L.call("tw_mt_states", None, 0, None, 0, None, None)
    with pytest.raises(ValueError, match="tw_mt_generate"):
        L.call("tw_mt_generate", None, 0, 1, 1, None, None, None, None, None)
    mask, rng = np.array([15], np.uint32), np.array([16], np.uint32)  # range above its mask
    with pytest.raises(ValueError, match="configuration 0"):
        L.call("tw_mt_generate", None, 1, 1, 1, mask.ctypes.data, rng.ctypes.data, None, None,
               None)
    with pytest.raises(ValueError, match="tw_np_randint_dev"):
        L.call("tw_np_randint_dev", None, None, None, 1, 1, 0, None, None, None, None, 1,
               mask.ctypes.data, mask.ctypes.data, None, 0, None, None, None)
    assert lib.tw_np_randint_dev_work_bytes(0, 1, 1, 1) == -1
    assert lib.tw_np_randint_dev_work_bytes(1, 1, 1, 5) == -1
    assert lib.tw_np_randint_dev_work_bytes(2, 2, 3, 1) >= 2 * 2 * 624 * 4
    np.random.seed(3)
    st = np.random.get_state()
    before = dict(R.DEVICE_DRAWS_STATS)
    assert R.randint_device([(0, b, 10) for b in (3, 100, 1000, 70000, 300000)]) is None
    assert R.randint_device([(5, 5, 10)]) is None  # an empty range
    assert R.randint_device([(0, 2 ** 32, 10)]) is None  # the unmasked 32-bit path
    assert R.randint_device([(0, 100, 10)], add=[2 ** 31]) is None  # beyond int32
    assert R.DEVICE_DRAWS_STATS == before
    assert np.random.get_state()[2] == st[2] and np.array_equal(np.random.get_state()[1], st[1])
    with pytest.raises(ValueError):
        R.randint_device([(0, 10, 5)], add=[1, 2])


def test_standalone_sanitized_driver(tmp_path):
    """tests/native/mtjump_driver.cpp with mtjump.cpp and numpy_rng.cpp under ASan + UBSan, as a
    program of its own (nothing sanitized is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path / "mtjump_driver"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-pthread",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", str(exe),
                        str(ROOT / "tests" / "native" / "mtjump_driver.cpp"),
                        str(CSRC / "mtjump.cpp"), str(CSRC / "numpy_rng.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = r.stdout.split("\n")
    for name in ["minpoly", "additivity", "arguments", "jump"]:
        assert f"ok {name}" in lines, r.stdout
