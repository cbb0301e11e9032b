"""Bulk replay of NumPy's legacy global RNG through libtuplewise.so (tw_np_randint_batch).

randint_batch([(low, high, size), ...]) returns exactly what the same sequence of
np.random.randint(low, high, size) calls would return, and leaves np.random in exactly the
state those calls would leave it — in one native call instead of one Python call each.
Only the MT19937-backed legacy global RandomState is supported (what the reference uses).
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np

from . import _lib as L

_RK_STATE_LEN = 624
_MT = {"bg": None, "ptrs": None}


def _mt_state():
    """(key, pos) pointers into the global legacy RandomState's MT19937 state — NumPy's own
    mt19937_state struct (uint32 key[624]; int pos), which the native draws then advance IN
    PLACE, with no get_state/set_state copies (~40 us a pair).  The layout is checked once
    against get_state.  None when the global generator is not an MT19937."""
    bg = getattr(np.random.mtrand._rand, "_bit_generator", None)
    if type(bg) is not np.random.MT19937:
        return None
    if _MT["bg"] is not bg:
        addr = int(bg.ctypes.state_address)
        key = np.ctypeslib.as_array((ctypes.c_uint32 * _RK_STATE_LEN).from_address(addr))
        pos = ctypes.c_int.from_address(addr + 4 * _RK_STATE_LEN)
        name, k, p = np.random.get_state(legacy=True)[:3]
        if name != "MT19937" or p != pos.value or not np.array_equal(k, key):
            return None
        _MT.update(bg=bg, ptrs=(ctypes.c_void_p(addr),
                                ctypes.c_void_p(addr + 4 * _RK_STATE_LEN)))
    return _MT["ptrs"]


class _CopiedState:
    """get_state/set_state around a native call: the fallback when _mt_state() is None."""

    def __init__(self):
        st = np.random.get_state(legacy=False)  # (a dict whatever the bit generator)
        if st["bit_generator"] != "MT19937":
            raise NotImplementedError("only the MT19937 legacy RandomState is supported")
        key, pos = st["state"]["key"], st["state"]["pos"]
        self.has_gauss, self.gauss = st["has_gauss"], st["gauss"]
        self.key = np.ascontiguousarray(key, dtype=np.uint32).copy()
        self.pos = ctypes.c_int32(int(pos))

    def ptrs(self):
        return ctypes.c_void_p(self.key.ctypes.data), ctypes.byref(self.pos)

    def commit(self):
        np.random.set_state(("MT19937", self.key, self.pos.value, self.has_gauss, self.gauss))


def _native_draws(fn):
    """Run fn(key_ptr, pos_ptr) on the global MT19937 state (in place when possible) and
    return its status; the state is committed even on error (NumPy would have consumed the
    draws made before the failing call)."""
    ptrs = _mt_state()
    if ptrs is not None:
        return fn(*ptrs)
    st = _CopiedState()
    rc = fn(*st.ptrs())
    st.commit()
    return rc


def randint_batch(calls) -> list:
    """[np.random.randint(lo, hi, n) for lo, hi, n in calls], one native call."""
    calls = list(calls)
    if not calls:
        return []
    low = np.array([c[0] for c in calls], dtype=np.int64)
    high = np.array([c[1] for c in calls], dtype=np.int64)
    cnt = np.array([int(c[2]) for c in calls], dtype=np.int64)
    out = np.empty(int(cnt.sum()), dtype=np.int64)
    rc = _native_draws(lambda key, pos: L.lib().tw_np_randint_batch(
        key, pos, len(calls), low.ctypes.data, high.ctypes.data, cnt.ctypes.data,
        out.ctypes.data))
    if rc:
        raise ValueError("high <= low")
    offs = np.concatenate([[0], np.cumsum(cnt)])
    return [out[offs[i]:offs[i + 1]] for i in range(len(cnt))]


# ----------------------------------------------------------------- MT19937 jump-ahead (host)
_POLY_WORDS = 312  # a polynomial over GF(2) of degree <= 19937, bit-packed in uint64


def mt_minpoly() -> np.ndarray:
    """phi(t), the degree-19937 minimal polynomial of the MT19937 word recurrence (bit k of
    the 312 uint64 = coefficient of t^k), by Berlekamp-Massey in csrc/mtjump.cpp."""
    out = np.zeros(_POLY_WORDS, dtype=np.uint64)
    if L.lib().tw_mt_minpoly(out.ctypes.data):
        raise RuntimeError("tw_mt_minpoly failed")
    return out


@functools.lru_cache(maxsize=256)
def mt_jump_poly(J: int) -> np.ndarray:
    """t^J mod phi(t) (read-only, cached): applied to an MT19937 state it advances it J words."""
    out = np.zeros(_POLY_WORDS, dtype=np.uint64)
    if J < 0 or L.lib().tw_mt_jump_poly(int(J), out.ctypes.data):
        raise ValueError(f"mt_jump_poly: bad jump {J}")
    out.flags.writeable = False
    return out


def mt_poly_mul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a * b mod phi for reduced polynomials."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    out = np.zeros(_POLY_WORDS, dtype=np.uint64)
    if a.shape != (_POLY_WORDS,) or b.shape != (_POLY_WORDS,) or L.lib().tw_mt_poly_mulmod(
            a.ctypes.data, b.ctypes.data, out.ctypes.data):
        raise ValueError("mt_poly_mul: operands must be reduced 312-word polynomials")
    return out


def mt_jumped(key, pos: int, J: int):
    """(key, pos) of np.random.get_state() advanced by exactly J words: what J genrand_int32
    calls (RandomState.randint(0, 2**32, J, dtype=np.uint32)) leave, in NumPy's representation."""
    k = np.array(key, dtype=np.uint32)  # a copy
    p = ctypes.c_int32(int(pos))
    if k.shape != (_RK_STATE_LEN,) or L.lib().tw_mt_jump_host(k.ctypes.data, ctypes.byref(p),
                                                              int(J)):
        raise ValueError(f"mt_jumped: bad state or jump (pos={pos}, J={J})")
    return k, p.value


# ------------------------------------------------------- randint streams drawn on the device
# words per sub-stream = 624 * STREAM_BLOCKS (tools/time_unnbt_dropin.py sweeps it); words per
# round (the word buffer's cap: 4 bytes each)
STREAM_BLOCKS = 420
ROUND_WORDS = 1 << 28
# rounds made / calls served by randint_device (tests tell from it that the device path ran)
DEVICE_DRAWS_STATS = {"rounds": 0, "calls": 0}
_MAX_CONFIGS = 4
_LEVEL_POLYS = {}  # stream_blocks -> [(t^(2^v L - 1), t^(2^v L)) for v = 0, 1, ...]
_LEVEL_POLYS_DEV = {}  # (device, stream_blocks, levels) -> int32 device tensor [levels, 2, 19968]
_POLY_CAP, _POLY_PAD = 19952, 20560  # listed positions a polynomial, the zero word's position


def _poly_list(g: np.ndarray) -> np.ndarray:
    """A bit-packed polynomial as tw_mt_states reads it: the count of listed positions (a
    multiple of 16) in word 0, the positions of its set coefficients from word 16 on, padded
    with the position of a zero word."""
    at = np.nonzero(np.unpackbits(np.ascontiguousarray(g).view(np.uint8), bitorder="little"))[0]
    row = np.full(16 + _POLY_CAP, _POLY_PAD, dtype=np.uint32)
    row[0] = -(-len(at) // 16) * 16
    row[16:16 + len(at)] = at
    return row


def _level_polys(stream_blocks: int, levels: int):
    """The doubling's polynomials on the device: level v jumps by 2^v L words (successive
    squarings of t^L), and by one word less from row 0 (the host key is a window AT its
    offset, the other rows one word before theirs): that is the same polynomial divided by t."""
    host = _LEVEL_POLYS.setdefault(stream_blocks, [])
    if len(host) < levels:
        phi = mt_minpoly()
        while len(host) < levels:
            g = (mt_poly_mul(host[-1][1], host[-1][1]) if host
                 else np.array(mt_jump_poly(_RK_STATE_LEN * stream_blocks)))
            h = g ^ phi if int(g[0]) & 1 else g  # g / t: phi's constant term is 1
            h = (h >> np.uint64(1)) | (np.append(h[1:], np.uint64(0)) << np.uint64(63))
            host.append((h, g))
    dev = L.device()
    key = (dev.index, stream_blocks, levels)
    if key not in _LEVEL_POLYS_DEV:
        flat = np.stack([np.stack([_poly_list(g) for g in p])
                         for p in host[:levels]]).view(np.int32)
        _LEVEL_POLYS_DEV[key] = L.to_device(flat)
    return _LEVEL_POLYS_DEV[key]


def mt_states(key, n_states: int, stream_blocks: int):
    """The (n_states, 624) int32 device table of tw_mt_states for a host key (624 uint32)."""
    k = np.ascontiguousarray(key, dtype=np.uint32)
    return _mt_states_ptr(ctypes.c_void_p(k.ctypes.data), n_states, stream_blocks)


def _mt_states_ptr(key_ptr, n_states: int, stream_blocks: int):
    t = L.torch()
    levels = max(0, int(n_states) - 1).bit_length()
    polys = _level_polys(stream_blocks, levels) if levels else None
    table = L.empty((int(n_states), _RK_STATE_LEN), t.int32)
    L.call("tw_mt_states", key_ptr, int(n_states), L.ptr(polys), levels, L.ptr(table),
           L.stream_handle())
    return table


def _masked_call(lo: int, hi: int, a: int):
    """(range, mask) of one supported randint call, or None."""
    rng = hi - 1 - lo
    if rng < 0 or rng >= 0xFFFFFFFF or lo + a < -(1 << 31) or hi + a > (1 << 31):
        return None
    return rng, (1 << rng.bit_length()) - 1


def randint_device(calls, add=None, *, stream_blocks=None, round_words=None, out_offsets=None):
    """[np.random.randint(lo, hi, n) + add[c] for lo, hi, n in calls] drawn ON THE DEVICE from
    NumPy's own legacy MT19937 stream (csrc/mtdraw.hip): returns (out, offsets)
    — an int32 device tensor and the int64 start of every call's values in it (len(calls) + 1
    entries; call order unless out_offsets places the calls) — and leaves np.random in exactly
    the state those calls would leave it.  Returns None, having drawn nothing, for what the
    device path does not serve: a global generator that is not the legacy MT19937, an empty
    range, high-1-low >= 2^32-1, values beyond int32, more than 4 distinct (mask, range) pairs.
    stream_blocks / round_words: key blocks per sub-stream and words per round (tuning and
    tests)."""
    t = L.torch()
    calls = [(int(lo), int(hi), int(n)) for lo, hi, n in calls]
    add = [0] * len(calls) if add is None else [int(a) for a in add]
    if len(add) != len(calls) or any(n < 0 for _, _, n in calls):
        raise ValueError("randint_device: one add per call, sizes >= 0")
    if _mt_state() is None and np.random.get_state(legacy=False)["bit_generator"] != "MT19937":
        return None
    sb = int(STREAM_BLOCKS if stream_blocks is None else stream_blocks)
    cap = int(ROUND_WORDS if round_words is None else round_words)
    if sb < 1 or cap < 1:
        raise ValueError("randint_device: stream_blocks and round_words must be positive")
    Lw = _RK_STATE_LEN * sb
    cnt = np.array([n for _, _, n in calls], dtype=np.int64)
    if out_offsets is None:
        offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        starts = offsets[:-1]
    else:
        starts = offsets = np.asarray(out_offsets, dtype=np.int64)
        order = np.argsort(starts, kind="stable")
        ends = (starts + cnt)[order]
        if starts.shape != cnt.shape or (len(cnt) and (
                starts[order][0] != 0 or np.any(starts[order][1:] != ends[:-1]))):
            raise ValueError("randint_device: out_offsets must tile the output")
    total = int(cnt.sum())
    configs, draws, fills = [], [], []
    for c, ((lo, hi, n), a) in enumerate(zip(calls, add)):
        mc = _masked_call(lo, hi, a)
        if mc is None:
            return None
        if n == 0:
            continue
        if mc[0] == 0:  # randint(low, low + 1): no draw
            fills.append((c, lo + a))
            continue
        if mc not in configs:
            configs.append(mc)
        draws.append((configs.index(mc), n, lo + a, int(starts[c]), mc[0] / (mc[1] + 1.0)))
    if len(configs) > _MAX_CONFIGS:
        return None
    out = L.empty((total,), t.int32)
    for c, v in fills:
        out[int(starts[c]):int(starts[c]) + int(cnt[c])] = v
    DEVICE_DRAWS_STATS["calls"] += len(calls)
    if not draws:
        return out, offsets
    cfg = np.array([d[0] for d in draws], dtype=np.int32)
    rem = np.array([d[1] for d in draws], dtype=np.int64)
    base = np.array([d[2] for d in draws], dtype=np.int64).astype(np.int32)
    at = np.array([d[3] for d in draws], dtype=np.int64)
    pacc = np.array([d[4] + 1.0 / (configs[d[0]][1] + 1.0) for d in draws])  # (range+1)/(mask+1)
    cmask = np.array([m for _, m in configs], dtype=np.uint32)
    crng = np.array([r for r, _ in configs], dtype=np.uint32)
    lib = L.lib()
    progress = (ctypes.c_int64 * 3)()

    def rounds(key, pos):
        pos_p = ctypes.cast(pos, ctypes.POINTER(ctypes.c_int32))
        ci = 0
        while ci < len(cfg):
            # words this round: the expected number for every remaining draw plus six standard
            # deviations of the rejected count, after the pos words of the current key block
            want = float(np.sum(rem[ci:] / pacc[ci:]))
            var = float(np.sum(rem[ci:] * (1.0 - pacc[ci:]) / pacc[ci:] ** 2))
            p0 = int(pos_p[0])
            S = int(math.ceil((p0 + want + 6.0 * math.sqrt(var) + 64.0) / Lw))
            S = max(1, min(S, cap // Lw), p0 // Lw + 1)
            table = _mt_states_ptr(key, S, sb)
            n = len(cfg) - ci
            work = L.empty((int(lib.tw_np_randint_dev_work_bytes(S, sb, n, len(configs))),),
                           t.uint8)
            c_cfg, c_rem = np.ascontiguousarray(cfg[ci:]), np.ascontiguousarray(rem[ci:])
            c_base, c_at = np.ascontiguousarray(base[ci:]), np.ascontiguousarray(at[ci:])
            L.call("tw_np_randint_dev", key, pos, L.ptr(table), S, sb, n, c_cfg.ctypes.data,
                   c_rem.ctypes.data, c_base.ctypes.data, c_at.ctypes.data, len(configs),
                   cmask.ctypes.data, crng.ctypes.data, L.ptr(out), total, L.ptr(work),
                   ctypes.addressof(progress), L.stream_handle())
            DEVICE_DRAWS_STATS["rounds"] += 1
            ci += int(progress[0])
            if ci < len(cfg):
                rem[ci] -= int(progress[1])
                at[ci] += int(progress[1])
        return 0

    _native_draws(rounds)
    return out, offsets


def _shuffle_items(a):
    """(items, item bytes) when np.random.shuffle(a) is the buffer path this module restates:
    a C-contiguous, writeable, non-object ndarray (rows of a 2-D array are items); else None
    (np.random.shuffle itself raises ValueError for a read-only array)."""
    if not isinstance(a, np.ndarray) or a.ndim == 0 or a.dtype.hasobject:
        return None
    if not a.flags.c_contiguous or not a.flags.writeable or a.size == 0:
        return None
    return a.shape[0], a.itemsize * (a.size // a.shape[0])


def shuffle_pair(X, Z) -> None:
    """np.random.shuffle(X); np.random.shuffle(Z) (compute_stats.py:66-67, estimation-experiment/
    main.py:46-47): the same index draws from the same legacy MT19937 stream, the same swaps,
    the same final RNG state — the swaps of X on a second native thread while Z's draws and
    swaps run.  Arrays the buffer path does not cover (views, object arrays, other RNGs) go
    to np.random.shuffle itself."""
    ix, iz = _shuffle_items(X), _shuffle_items(Z)
    # aliasing X and Z (the same array or overlapping views): the second shuffle must see the
    # first one's swaps, which the concurrent native path does not give
    if ix is None or iz is None or np.shares_memory(X, Z) or (
            _mt_state() is None and np.random.get_state(legacy=True)[0] != "MT19937"):
        np.random.shuffle(X)
        np.random.shuffle(Z)
        return
    jbuf = np.empty(ix[0] + iz[0], dtype=np.int64)
    rc = _native_draws(lambda key, pos: L.lib().tw_np_shuffle_pair(
        key, pos, X.ctypes.data, ix[0], ix[1], Z.ctypes.data, iz[0], iz[1], jbuf.ctypes.data))
    if rc:
        raise RuntimeError(f"tw_np_shuffle_pair failed ({rc})")


def shuffle_draws32(n: int, out=None) -> np.ndarray:
    """The index draws np.random.shuffle makes on n items (n <= 2^31), without the swaps: a
    uint32 array j with j[i] for i = n-1 down to 1 (j[0] = 0), the global legacy state advanced
    exactly as the shuffle would advance it (the host half of _engine.DeviceShuffles).
    out: a C-contiguous 4-byte array of n entries to draw into (e.g. pinned memory)."""
    if out is None:
        j = np.zeros(max(int(n), 0), dtype=np.uint32)
    else:
        j = out.view(np.uint32)
        if j.shape != (max(int(n), 0),) or not j.flags.c_contiguous:
            raise ValueError("shuffle_draws32: out must be a contiguous array of n 4-byte items")
        if n > 0:
            j[0] = 0
    rc = _native_draws(lambda key, pos: L.lib().tw_np_shuffle_draws32(key, pos, int(n),
                                                                       j.ctypes.data))
    if rc:
        raise ValueError(f"tw_np_shuffle_draws32 failed ({rc}) for n = {n}")
    return j


def shuffle_draws32_range(n: int, hi: int, lo: int, out) -> None:
    """shuffle_draws32's draws for i = hi down to lo only (1 <= lo <= hi < n), into out (the
    shuffle's whole n-entry 4-byte array; other entries untouched), the global legacy state
    advanced past them: consecutive ranges from hi = n - 1 down to lo = 1 make exactly
    shuffle_draws32(n)'s draws (_engine.DeviceShuffles streams the drop-in's last shuffle)."""
    j = out.view(np.uint32)
    if j.shape != (int(n),) or not j.flags.c_contiguous:
        raise ValueError("shuffle_draws32_range: out must be a contiguous array of n items")
    rc = _native_draws(lambda key, pos: L.lib().tw_np_shuffle_draws32_range(
        key, pos, int(n), int(hi), int(lo), j.ctypes.data))
    if rc:
        raise ValueError(f"tw_np_shuffle_draws32_range failed ({rc}) for n={n}, [{lo}, {hi}]")


class Session:
    """NumPy's legacy global MT19937 state held in native code for a run of draws.

    The draws advance NumPy's own MT19937 state in place (_mt_state), so foreign draws between
    them need nothing; where that is unavailable the session holds a copy, nothing else may
    draw from np.random while it is open, commit() writes it back (and is called on exit) and
    acquire() re-reads it after foreign draws.  Every draw equals the corresponding
    np.random.randint call bit for bit."""

    def __init__(self):
        self.acquire()

    def acquire(self):
        ptrs = _mt_state()
        self._copy = None if ptrs is not None else _CopiedState()
        self._key, self._pos = ptrs if ptrs is not None else self._copy.ptrs()

    def commit(self):
        if self._copy is not None:
            self._copy.commit()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.commit()
        return False

    def randint_flat(self, low, high, cnt, out=None) -> np.ndarray:
        """Consecutive randint(low[c], high[c], cnt[c]) calls, concatenated."""
        low = np.ascontiguousarray(low, dtype=np.int64)
        high = np.ascontiguousarray(high, dtype=np.int64)
        cnt = np.ascontiguousarray(cnt, dtype=np.int64)
        if out is None:
            out = np.empty(int(cnt.sum()), dtype=np.int64)
        rc = L.lib().tw_np_randint_batch(self._key, self._pos, len(cnt), low.ctypes.data,
                                         high.ctypes.data, cnt.ctypes.data, out.ctypes.data)
        if rc:
            raise ValueError("high <= low")
        return out

    def pairs(self, N, kx, kz, B, ix, iz):
        """grad_inc_block's draws of all N shards into int64 arrays ix, iz of shape (N, B)."""
        assert ix.flags.c_contiguous and iz.flags.c_contiguous
        rc = L.lib().tw_np_randint_pairs(self._key, self._pos, int(N), int(kx), int(kz),
                                         int(B), ix.ctypes.data, iz.ctypes.data)
        if rc:
            raise ValueError("high <= low")

    def pairs_steps_u16(self, S, N, kx, kz, B, out):
        """pairs_steps into a uint16 array (kx, kz <= 65536): the same indices, narrowed."""
        assert out.flags.c_contiguous and out.shape[0] >= S
        assert out.shape[1:] == (2, N, B) and out.dtype == np.uint16
        rc = L.lib().tw_np_randint_pairs_steps_u16(self._key, self._pos, int(S), int(N),
                                                   int(kx), int(kz), int(B), out.ctypes.data)
        if rc:
            raise ValueError("high <= low or an index range beyond 65536")

    def pairs_steps_u8(self, S, N, kx, kz, B, out):
        """pairs_steps into a uint8 array (kx, kz <= 256): the same indices, narrowed."""
        assert out.flags.c_contiguous and out.shape[0] >= S
        assert out.shape[1:] == (2, N, B) and out.dtype == np.uint8
        rc = L.lib().tw_np_randint_pairs_steps_u8(self._key, self._pos, int(S), int(N),
                                                  int(kx), int(kz), int(B), out.ctypes.data)
        if rc:
            raise ValueError("high <= low or an index range beyond 256")

    def pairs_steps(self, S, N, kx, kz, B, out):
        """S consecutive steps of grad_inc_block's draws: out[s, 0] and out[s, 1] ((N, B)
        int64 each) receive step s's X and Z indices, in the reference's draw order."""
        assert out.flags.c_contiguous and out.shape[0] >= S
        assert out.shape[1:] == (2, N, B) and out.dtype == np.int64
        rc = L.lib().tw_np_randint_pairs_steps(self._key, self._pos, int(S), int(N), int(kx),
                                               int(kz), int(B), out.ctypes.data)
        if rc:
            raise ValueError("high <= low")
