"""The chain emission's round tables (tw_chain_emit_ws, tw_chain_set_emit_tables; csrc/chain.hip
k_chain_emit, csrc/feistel.h): a table holds exactly the values of the Feistel
round functions, so an emission that looks its rounds up must equal the arithmetic one bit for
bit.  Every test runs the hook at 1 (off) against 2 (on wherever a table fits) and against 0
(automatic) and asserts exact equality: the chain state (xpos / zpos), the cursors, every
(step, shard) bag as a sorted array; in exchange mode every bucket's count word, its sorted
records and the overflow flag.  Shapes: every half_bits the tables serve and the one above
(the fallback), classes of different domains, 1 / 2 / 32 steps, a second chunk continuing the
first, every kernel form of tw_chain_set_emit and the unstaged form, half ties, simulated
ranks, an overflowing capacity, shard size 0, a tail bucket, the oracle's chain, and the
workspace contract (one byte short, two streams)."""
import numpy as np
import pytest

import test_gpu_plan_sweep as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu
M64 = 2 ** 64 - 1
MODES = (1, 2, 0)


@pytest.fixture(autouse=True)
def _hooks_back():
    yield
    from tuplewise import _lib as L
    L.lib().tw_chain_set_emit_tables(0)
    L.call("tw_chain_set_emit", 0, 0)


def _set_tables(L, mode):
    assert L.lib().tw_chain_set_emit_tables(mode) in (0, 1, 2)
    assert L.lib().tw_chain_set_emit_tables(-1) == mode


def _half_bits(N):
    bits = 2
    while (1 << bits) < N:
        bits += 1
    return (bits + 1) // 2


def _records(rng, n, half):
    """Records as the emission reads them: the low word is the image, the high word h(x) under
    half ties and otherwise an index the emission must ignore."""
    import torch
    lo = rng.randint(0, 1 << 24, n).astype(np.uint64)
    hi = rng.randint(0, 1 << 24, n).astype(np.uint64)
    return torch.from_numpy((lo | (hi << np.uint64(32))).view(np.int64)).cuda()


def _keys(T, salt=0):
    ks = [(1000003 * (c + 1) + salt) & M64 for c in range(T)]
    return [(2 * k) & M64 for k in ks], [(2 * k + 1) & M64 for k in ks]


def _emit_bags(ops, xr, zr, half, N, kx, kz, kxs, kzs, chunk=32):
    """One process: the emission in chunks of `chunk` steps through the chain state; the chain
    state, each chunk's cursors, and the canonical bags."""
    import torch
    n, m, T = int(xr.numel()), int(zr.numel()), len(kxs)
    x_bag = torch.zeros((T, n), dtype=torch.int64 if half else torch.int32, device="cuda")
    z_bag = torch.zeros((T, m), dtype=torch.int32, device="cuda")
    xpos = torch.zeros(n, dtype=torch.int32, device="cuda")
    zpos = torch.zeros(m, dtype=torch.int32, device="cuda")
    curs = []
    for t0 in range(0, T, chunk):
        t1 = min(T, t0 + chunk)
        cur = torch.full(((t1 - t0) * 2 * (N + 1),), -1, dtype=torch.int32, device="cuda")
        ops.chain_emit(xr, zr, half, xpos, zpos, t0 == 0, 0, 1, kxs[t0:t1], kzs[t0:t1], kx, kz,
                       N, x_bag=x_bag[t0:], z_bag=z_bag[t0:], cursors=cur)
        curs.append(cur)
    rx = torch.from_numpy(S.bag_regions(n, kx, N)).cuda()
    rz = torch.from_numpy(S.bag_regions(m, kz, N)).cuda()
    return dict(xpos=xpos, zpos=zpos, cur=torch.cat(curs), xb=S._bag_canon_dev(x_bag, rx),
                zb=S._bag_canon_dev(z_bag, rz))


def _same(a, b):
    import torch
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _all_modes(L, run):
    """run() under the hook at 1, 2 and 0: the results of 2 and 0 equal those of 1."""
    out = {}
    for mode in MODES:
        _set_tables(L, mode)
        out[mode] = run()
    _same(out[1], out[2])
    _same(out[1], out[0])
    return out[1]


def _oracle_positions(base, n, N_tot, keys):
    p = np.arange(base, base + n)
    for k in keys:
        p = O.feistel_perm(p, N_tot, int(k))
    return p


# (n per class, shards); the domains hit half_bits 1, 2, 5, 6, 10, 11
TABLE_SHAPES = [(3, 1), (16, 2), (1000, 7), (1025, 7), (262145, 64), (1048577, 64)]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("n,N", TABLE_SHAPES)
def test_tables_equal_arithmetic_one_process(gpu, n, N, half):
    """Steps 1, 2 and 32 at the small domains (the chain state also against the oracle's
    chain), 2 and 32 steps at the large ones."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    hbs = {3: 1, 16: 2, 1000: 5, 1025: 6, 262145: 10, 1048577: 11}
    assert _half_bits(n) == hbs[n]
    ops = HipOps()
    rng = np.random.RandomState(n)
    xr, zr = _records(rng, n, half), _records(rng, n, False)
    k = n // N
    for T in ((1, 2, 32) if n <= 1025 else (2, 32)):
        kxs, kzs = _keys(T, n)
        _set_tables(L, 0)
        assert L.lib().tw_chain_emit_work_bytes(T, n, n) >= T * 2 * (6 << hbs[n]) * 2
        for mode, want in ((1, 0), (2, 1)):
            _set_tables(L, mode)
            assert L.lib().tw_chain_emit_tables_of(n, n, 1, int(half), 0, N) == want
        got = _all_modes(L, lambda: _emit_bags(ops, xr, zr, half, N, k, k, kxs, kzs))
        if n <= 1025:
            assert np.array_equal(got["xpos"].cpu().numpy().view(np.uint32),
                                  _oracle_positions(0, n, n, kxs))
            assert np.array_equal(got["zpos"].cpu().numpy().view(np.uint32),
                                  _oracle_positions(0, n, n, kzs))


def test_classes_of_different_domains(gpu):
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(2)
    n, m, N = 1000, 5000, 9
    assert (_half_bits(n), _half_bits(m)) == (5, 7)
    xr, zr = _records(rng, n, False), _records(rng, m, False)
    kxs, kzs = _keys(5)
    got = _all_modes(L, lambda: _emit_bags(ops, xr, zr, False, N, n // N, m // N, kxs, kzs))
    assert np.array_equal(got["xpos"].cpu().numpy().view(np.uint32),
                          _oracle_positions(0, n, n, kxs))
    assert np.array_equal(got["zpos"].cpu().numpy().view(np.uint32),
                          _oracle_positions(0, m, m, kzs))


def test_fallback_above_the_largest_table(gpu):
    """n = 4194305 (half_bits 12): no table; the hook forced on runs the arithmetic rounds."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(3)
    n, m, N = 4194305, 1000, 64
    assert _half_bits(n) == 12
    xr, zr = _records(rng, n, False), _records(rng, m, False)
    kxs, kzs = _keys(2)
    for mode in MODES:
        _set_tables(L, mode)
        assert L.lib().tw_chain_emit_tables_of(n, m, 1, 0, 0, N) == 0
    assert L.lib().tw_chain_emit_work_bytes(2, n, m) == 0
    _all_modes(L, lambda: _emit_bags(ops, xr, zr, False, N, n // N, m // N, kxs, kzs))


@pytest.mark.parametrize("n", [1000, 777])
def test_oracle_chain_and_second_chunk(gpu, n):
    """Positions after 5 steps equal oracle.feistel_perm's chain; a second chunk continuing the
    first (first = 0) equals one 64-step oracle chain."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(n)
    m, N = n - 100, 5
    xr, zr = _records(rng, n, False), _records(rng, m, False)
    for T in (5, 64):
        kxs, kzs = _keys(T, 7)
        got = _all_modes(L, lambda: _emit_bags(ops, xr, zr, False, N, n // N, m // N, kxs, kzs))
        assert np.array_equal(got["xpos"].cpu().numpy().view(np.uint32),
                              _oracle_positions(0, n, n, kxs))
        assert np.array_equal(got["zpos"].cpu().numpy().view(np.uint32),
                              _oracle_positions(0, m, m, kzs))
        # the cursors of the last chunk: every shard's bag is full
        x_off = np.minimum(np.arange(N + 2) * (n // N), n)
        x_off[-1] = n
        cur = got["cur"].cpu().numpy().reshape(T, 2, N + 1)
        assert (cur[:, 0, :] == np.diff(x_off)).all()


FORMS = [(2, 8), (2, 1), (4, 4), (4, 1), (8, 1), (8, 2)]


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("epr,spr", FORMS)
def test_every_kernel_form(gpu, epr, spr, half):
    """Every tw_chain_set_emit form, one process (7 shards; 600 shards: the unstaged form;
    shard size 0; a shard size that leaves a tail bucket) — 5 steps, 2 tiles and a ragged one."""
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(epr * 16 + spr)
    n, m = 2 * 256 * epr + 77, 256 * epr + 1
    xr, zr = _records(rng, n, half), _records(rng, m, False)
    kxs, kzs = _keys(5, epr)
    L.call("tw_chain_set_emit", epr, spr)
    for N, kx, kz in ((7, n // 7, m // 7), (600, n // 600, m // 600), (4, 0, 0),
                      (3, n // 4, m // 5)):
        _all_modes(L, lambda: _emit_bags(ops, xr, zr, half, N, kx, kz, kxs, kzs))


def _emit_send(ops, xr, zr, half, r, G, N, kx, kz, kxs, kzs, cap):
    """One rank of G into send buckets: the chain state, the flag, every bucket's count word
    and (where nothing overflowed) every bucket's records sorted."""
    import torch
    n, m, T, W = int(xr.numel()), int(zr.numel()), len(kxs), 2 if half else 1
    send = torch.zeros(G * T * (cap + 1) * W, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    xpos = torch.zeros(n, dtype=torch.int32, device="cuda")
    zpos = torch.zeros(m, dtype=torch.int32, device="cuda")
    ops.chain_emit(xr, zr, half, xpos, zpos, True, r, G, kxs, kzs, kx, kz, N, send=send, cap=cap,
                   flag=flag)
    b = send.view(G * T, cap + 1, W)
    counts = b[:, 0, 0].clone()
    out = dict(xpos=xpos, zpos=zpos, flag=flag, counts=counts)
    if int(flag.item()) == 0:
        recs = b[:, 1:, :].clone()
        live = torch.arange(cap, device="cuda")[None, :] < counts[:, None]
        recs[~live] = 0  # slots past a bucket's count are not the emission's
        # sort every bucket's records: by the last word, then stably by the first
        for w in range(W - 1, -1, -1):
            idx = torch.sort(recs[:, :, w], dim=1, stable=True)[1]
            recs = torch.gather(recs, 1, idx[:, :, None].expand(-1, -1, W))
        out["recs"] = recs
    return out


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("r,G", [(0, 1), (1, 3), (2, 3)])
def test_exchange_mode(gpu, r, G, half):
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(10 * G + r)
    n, m, N = 3000, 2100, 4
    xr, zr = _records(rng, n, half), _records(rng, m, False)
    kx, kz = n // N, m // N
    tot = n + m
    cap = tot // G + tot // (8 * G) + 1024
    for T, forms in ((3, [(0, 0)] + FORMS), (32, [(0, 0)])):
        kxs, kzs = _keys(T, r)
        for epr, spr in forms:
            L.call("tw_chain_set_emit", epr, spr)
            got = _all_modes(L, lambda: _emit_send(ops, xr, zr, half, r, G, N, kx, kz, kxs, kzs,
                                                   cap))
            assert int(got["flag"].item()) == 0
            assert int(got["counts"].sum().item()) == T * tot
            assert np.array_equal(got["xpos"].cpu().numpy().view(np.uint32),
                                  _oracle_positions(r * n, n, G * n, kxs))
    # a capacity too small: both paths raise the flag and count the same attempts
    L.call("tw_chain_set_emit", 0, 0)
    kxs, kzs = _keys(3, r)
    got = _all_modes(L, lambda: _emit_send(ops, xr, zr, half, r, G, N, kx, kz, kxs, kzs,
                                           tot // (2 * G)))
    assert int(got["flag"].item()) == 1 and "recs" not in got


def test_workspace_one_byte_short(gpu):
    """An undersized workspace is TW_ERR_ARG before any launch, under every setting."""
    import torch
    from tuplewise import _lib as L
    rng = np.random.RandomState(5)
    n, N, T = 1000, 4, 3
    xr, zr = _records(rng, n, False), _records(rng, n, False)
    kxs, kzs = _keys(T)
    kxa, kza = np.array(kxs, dtype=np.uint64), np.array(kzs, dtype=np.uint64)
    wb = int(L.lib().tw_chain_emit_work_bytes(T, n, n))
    assert wb == T * 2 * (6 << 5) * 2
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")

    def call(bytes_given):
        s = {k: torch.full((sz,), -7, dtype=torch.int32, device="cuda")
             for k, sz in (("xpos", n), ("zpos", n), ("cur", T * 2 * (N + 1)), ("xb", T * n),
                           ("zb", T * n))}
        L.call("tw_chain_emit_ws", xr, n, zr, n, 0, s["xpos"], s["zpos"], 1, 0, 1,
               kxa.ctypes.data, kza.ctypes.data, T, n // N, n // N, N, s["xb"], s["zb"],
               s["cur"], None, 0, None, work, bytes_given, L.stream_handle())
        return s

    for mode in MODES:
        _set_tables(L, mode)
        with pytest.raises(ValueError, match="workspace"):
            call(wb - 1)
    # off: the workspace is not written; on: the launch wrote the chunk's tables into it (the
    # table path ran), entry (i << half_bits) + R of (step, class) = the oracle's round value
    _set_tables(L, 1)
    call(wb)
    assert bool((work == 0).all())
    _set_tables(L, 2)
    ok = call(wb)
    assert np.array_equal(ok["xpos"].cpu().numpy().view(np.uint32),
                          _oracle_positions(0, n, n, kxs))
    got = work.cpu().numpy().view(np.uint16).reshape(T, 2, 6, 32)
    R = np.arange(32, dtype=np.uint64)
    for c in range(T):
        for cls, key in ((0, kxs[c]), (1, kzs[c])):
            half, ks = O._feistel_keys(n, key)
            assert half == 5
            for i, k in enumerate(ks):
                arg = (R * np.uint64(0x9E3779B1) + np.uint64(k)) & O._M32
                want = O._mix32(arg) & np.uint64(31)
                assert np.array_equal(got[c, cls, i], want.astype(np.uint16)), (c, cls, i)


def test_hook_refuses_other_values(gpu):
    """A value other than -1, 0, 1, 2 is TW_ERR_ARG and changes nothing."""
    from tuplewise import _lib as L
    for mode in MODES:
        _set_tables(L, mode)
        for bad in (3, -2, 7, 2 ** 31 - 1):
            assert L.lib().tw_chain_set_emit_tables(bad) == L.TW_ERR_ARG
            assert b"tw_chain_set_emit_tables" in L.lib().tw_last_error()
            assert L.lib().tw_chain_set_emit_tables(-1) == mode
            with pytest.raises(ValueError):
                L.call("tw_chain_set_emit_tables", bad)


def test_refused_call_launches_nothing(gpu):
    import torch
    from tuplewise import _lib as L
    rng = np.random.RandomState(6)
    n, N, T = 1000, 4, 2
    xr, zr = _records(rng, n, False), _records(rng, n, False)
    kxs, kzs = _keys(T)
    kxa, kza = np.array(kxs, dtype=np.uint64), np.array(kzs, dtype=np.uint64)
    wb = int(L.lib().tw_chain_emit_work_bytes(T, n, n))
    work = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    bufs = [torch.full((sz,), -7, dtype=torch.int32, device="cuda")
            for sz in (n, n, T * 2 * (N + 1), T * n, T * n)]
    xpos, zpos, cur, xb, zb = bufs
    with pytest.raises(ValueError, match="workspace"):
        L.call("tw_chain_emit_ws", xr, n, zr, n, 0, xpos, zpos, 1, 0, 1, kxa.ctypes.data,
               kza.ctypes.data, T, n // N, n // N, N, xb, zb, cur, None, 0, None, work, wb - 1,
               L.stream_handle())
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == -7).all())
    assert bool((work == 0).all())


def test_two_streams_with_their_own_workspaces(gpu):
    """Two emissions on two streams, each with its stream's buffer, give what each gives alone
    on one stream."""
    import torch
    from tuplewise import _lib as L
    from tuplewise.device import HipOps
    ops = HipOps()
    rng = np.random.RandomState(8)
    n, m, N = 20000, 15000, 7
    xr, zr = _records(rng, n, False), _records(rng, m, False)
    jobs = [_keys(32, 1), _keys(32, 2)]
    _set_tables(L, 2)
    alone = [_emit_bags(ops, xr, zr, False, N, n // N, m // N, kxs, kzs) for kxs, kzs in jobs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    both = []
    for st, (kxs, kzs) in zip(streams, jobs):
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            both.append(_emit_bags(ops, xr, zr, False, N, n // N, m // N, kxs, kzs))
    torch.cuda.synchronize()
    assert len(ops._emit_pool) >= 3  # the current stream's buffer and one per side stream
    for a, b in zip(alone, both):
        _same(a, b)
