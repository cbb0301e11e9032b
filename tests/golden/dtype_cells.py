"""The dtype / layout contract matrix of the drop-in API.

One list, CELLS, read by three parties: tests/golden/make_golden_dtypes.py runs every cell
through the REFERENCE and stores inputs and outcomes (golden_dtypes.npz / .json);
tests/test_oracle_dtypes.py runs the oracle on the stored inputs; tests/test_gpu_dtypes.py
runs the drop-in.  render_tables() prints the INTEGRATION.md tables from the same list.

A cell is one call: fn names the function, args its scalar arguments, make() builds the input
buffers (seeded legacy RandomState, so a buffer too large to store is rebuilt bit for bit),
view names how the call's X / Z are cut from those buffers, and contract says what the drop-in
owes the reference for it:
  "exact"   the reference's value and dtype, identical
  "rtol"    within 1e-12 relative (float kernels; another summation order only)
  "rtol32"  within 1e-5 relative (float32 inputs: NumPy accumulates in float32)
  an exception class name: the drop-in raises it instead of returning another number.
"""
from __future__ import annotations

import collections
import hashlib
import json
import pathlib
import zlib

import numpy as np

Cell = collections.namedtuple("Cell", "id group row col fn args make view contract stored")

NX, NZ, N, B = 37, 23, 4, 16
BIG = 1 << 16  # _blocks.DEVICE_SHUFFLE_MIN: the strided layout case must reach it
RTOL = {"rtol": 1e-12, "rtol32": 1e-5}
SHARDED = ("est.UnN", "cs.UnN", "cs.UnNB", "est.replicate")  # state after the call is stored

CELLS: list = []


def _rng(cid):
    return np.random.RandomState(zlib.crc32(cid.encode()))


def _add(cid, group, row, col, fn, args, make, contract, view=("whole", "whole"), stored=True):
    assert all(c.id != cid for c in CELLS), cid
    CELLS.append(Cell(cid, group, row, col, fn, args, make, view, contract, stored))


def _vals(dtype, n, rng):
    """Small values with ties inside and across dtypes (quarter steps are exact in float16)."""
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.rand(n) > 0.5
    if dt.kind == "u":
        return rng.randint(0, 12, n).astype(dt)
    if dt.kind == "i":
        return rng.randint(-6, 7, n).astype(dt)
    return (rng.randint(-24, 49, n) / 4).astype(dt)


def _name(dtype):
    dt = np.dtype(dtype)
    return dt.str if dt.byteorder == ">" else dt.name


# ------------------------------------------------------------------------- comparisons
CMP_FNS = (("est.Un", "est.Un", {}),
           ("est.UnN", "est.UnN prop-SWOR", {"N": N, "sampling": "prop-SWOR"}),
           ("cs.Un", "cs.Un AUC", {"kernel": "AUC"}))


def _cmp_cells(tag, row, make, contracts=None, fns=CMP_FNS):
    for fn, col, args in fns:
        contract = (contracts or {}).get(col, "exact")
        _add(f"cmp/{tag}/{col.replace(' ', '_')}", "comparisons", row, col, fn, args, make,
             contract)


def _pair_maker(cid, dx, dz):
    def make():
        rng = _rng(cid)
        return {"X": _vals(dx, NX, rng), "Z": _vals(dz, NZ, rng)}
    return make


for _d in ("bool", "int8", "int16", "int32", "uint8", "uint16", "uint32", "uint64", "float16",
           "float32"):
    for _p in (_d, "int64", "float64"):
        _cmp_cells(f"{_d}-{_p}", f"{_d} / {_p}", _pair_maker(f"cmp/{_d}-{_p}", _d, _p),
                   {"cs.Un AUC": "TypeError"} if (_d, _p) == ("bool", "bool") else None)


def _make_f64_i64_big():
    rng = _rng("f64-i64-big")
    X = 2.0 ** 53 + 2.0 * rng.randint(0, 6, NX)  # doubles above 2^53 are even
    Z = 2 ** 53 + rng.randint(0, 12, NZ).astype(np.int64)  # odd ones round in `X > Z`
    return {"X": X, "Z": Z}


_cmp_cells("float64-int64-above2^53", "float64 / int64, values above 2^53", _make_f64_i64_big)


def _make_u64_i64(variant):
    def make():
        rng = _rng("u64-i64-" + variant)
        if variant == "small":
            X = rng.randint(0, 12, NX).astype(np.uint64)
            Z = rng.randint(-6, 12, NZ).astype(np.int64)
        elif variant == "mid":  # neighbours in (2^53, 2^63): equal after a float64 cast
            X = (2 ** 53 + 1 + rng.randint(0, 8, NX)).astype(np.uint64)
            Z = (2 ** 53 + rng.randint(0, 8, NZ)).astype(np.int64)
            X[0], Z[0] = 2 ** 53 + 1, 2 ** 53
        else:
            pool_x = np.array([2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1, 2 ** 63 - 1, 0, 5],
                              dtype=np.uint64)
            pool_z = np.array([2 ** 63 - 1, -2 ** 63, -1, 0, 2 ** 63 - 2, 5], dtype=np.int64)
            X = pool_x[rng.randint(0, len(pool_x), NX)]
            Z = pool_z[rng.randint(0, len(pool_z), NZ)]
        return {"X": X, "Z": Z}
    return make


for _v, _label in (("small", "values below 2^53"), ("mid", "neighbours in (2^53, 2^63)"),
                   ("top", "uint64 >= 2^63 against int64 max / min")):
    _cmp_cells(f"uint64-int64-{_v}", f"uint64 / int64, {_label}", _make_u64_i64(_v))

BYTEORDER_FNS = CMP_FNS + (
    ("est.replicate", "replicate(est.Un)", {"estimator": "Un", "n_tries": 3}),
    ("est.replicate", "replicate(est.UnN)",
     {"estimator": "UnN", "n_tries": 3, "N": N, "sampling": "prop-SWOR"}))
for _d in (">f8", ">i8"):
    _cmp_cells(f"{_d}-{_d}", f"{_d} / {_d}", _pair_maker(f"cmp/{_d}", _d, _d),
               fns=BYTEORDER_FNS)
_cmp_cells("int8-int8-wrap", "int8 / int8, X - Z wraps",
           lambda: {"X": np.array([100, -100, 3], np.int8), "Z": np.array([-100, 100], np.int8)},
           {"cs.Un AUC": "NotImplementedError"}, fns=CMP_FNS[2:])

# ------------------------------------------------------------------------- float kernels
FLOAT_FNS = (("cs.Un", "cs.Un prod", {"kernel": "prod"}, "prod"),
             ("cs.Un", "cs.Un gini", {"kernel": "gini"}, "gini"),
             ("cs.conv_AUC", "conv_AUC(1)", {"margin": 1}, "hinge"),
             ("cs.conv_AUC", "conv_AUC(0.5)", {"margin": 0.5}, "hinge"),
             ("cs.UB_indices", "UB_indices prod", {"kernel": "prod"}, "prod"),
             ("cs.UB_indices", "UB_indices gini", {"kernel": "gini"}, "gini"),
             ("cs.UnN", "cs.UnN prod", {"N": N, "sampling": "prop-SWOR", "kernel": "prod"},
              "prod"))


def _with_indices(d, rng):
    d["ix"] = rng.randint(0, len(d["X"]), 40)
    d["iz"] = rng.randint(0, len(d["Z"]), 40)
    return d


def _make_int_kernel(cid, dtype, wraps, op):
    """Integer inputs of a float kernel.  wraps=False: every difference, product and sum stays
    inside the dtype and below 2^53, so NumPy's integer arithmetic equals the float64 device
    path; wraps=True: the reference's arithmetic wraps around (or leaves 2^53's exact range)."""
    dt = np.dtype(dtype)

    def make():
        rng = _rng(cid)
        if not wraps and dt.kind == "u":
            lo_x, lo_z = rng.randint(1, 16, NX), rng.randint(1, 16, NZ)
            hi_x, hi_z = rng.randint(100, 120, NX), rng.randint(100, 120, NZ)
            X, Z = {"prod": (lo_x, lo_z), "gini": (hi_x, lo_z), "hinge": (lo_x, hi_z)}[op]
        elif not wraps and dt == np.int64:
            X, Z = rng.randint(2 ** 25, 2 ** 26, NX), rng.randint(1, 2 ** 26, NZ)
        elif not wraps:
            X, Z = rng.randint(-50, 51, NX), rng.randint(-50, 51, NZ)
        elif dt == np.uint8:  # the uint8 rows of the issue's table, then more of the kind
            X = np.concatenate([[1, 200], rng.randint(100, 256, NX - 2)])
            Z = np.concatenate([[2, 3], rng.randint(100, 256, NZ - 2)])
        elif dt == np.uint64:  # gini / hinge wrap where x < z / z < x; 2^62 * 4 wraps in prod
            X, Z = rng.randint(0, 50, NX).astype(dt), rng.randint(0, 50, NZ).astype(dt)
            X[0], Z[0] = 2 ** 62, 4
        else:
            big = 2 ** 62 if dt == np.int64 else 2 ** 30
            X, Z = rng.randint(-50, 51, NX).astype(dt), rng.randint(-50, 51, NZ).astype(dt)
            X[:2] = [big, -big]
            Z[:3] = [4, -big - 1, big]
        return _with_indices({"X": np.asarray(X).astype(dt), "Z": np.asarray(Z).astype(dt)}, rng)
    return make


def _make_float_kernel(cid, dtype):
    def make():
        rng = _rng(cid)
        dt = np.dtype(dtype)
        if dt.kind == "b":
            X, Z = rng.rand(NX) > 0.4, rng.rand(NZ) > 0.6
        elif dt == np.float16:
            X, Z = _vals(dt, NX, rng), _vals(dt, NZ, rng)
            X[0] = Z[0] = 300  # 300 * 300 is beyond float16's 65504: NumPy returns inf
        else:  # float32, away from zero: the mean does not cancel
            X = rng.normal(1.0, 0.3, NX).astype(dt)
            Z = rng.normal(0.5, 0.3, NZ).astype(dt)
        return _with_indices({"X": X, "Z": Z}, rng)
    return make


for _d in ("int64", "int32", "uint8", "uint64"):
    for _wraps in (False, True):
        _row = f"{_d}, " + ("reference wraps" if _wraps else "no wrap, below 2^53")
        for _fn, _col, _args, _op in FLOAT_FNS:
            _cid = f"flt/{_d}-{'wrap' if _wraps else 'safe'}/{_col.replace(' ', '_')}"
            _add(_cid, "float kernels", _row, _col, _fn, _args,
                 _make_int_kernel(_cid if _d.startswith("u") else f"flt/{_d}-{_wraps}", _d,
                                  _wraps, _op),
                 "NotImplementedError" if _wraps else "rtol")
for _d, _row, _contract in (("float16", "float16, a product beyond 65504", "NotImplementedError"),
                            ("float32", "float32", "rtol32"), ("bool", "bool", None)):
    for _fn, _col, _args, _op in FLOAT_FNS:
        _c = _contract or ("rtol" if _op == "prod" else "TypeError")  # bool - bool: as NumPy
        _add(f"flt/{_d}/{_col.replace(' ', '_')}", "float kernels", _row, _col, _fn, _args,
             _make_float_kernel(f"flt/{_d}", _d), _c)

# ------------------------------------------------------------------------- layouts
LAYOUT_FNS = (("est.UnN", "est.UnN prop-SWOR", {"N": N, "sampling": "prop-SWOR"}),
              ("cs.UnN", "cs.UnN AUC SWOR", {"N": N, "sampling": "SWOR", "kernel": "AUC"}),
              ("cs.UnNB", "cs.UnNB AUC prop-SWOR",
               {"N": N, "B": B, "sampling": "prop-SWOR", "kernel": "AUC"}))
VIEWS = {"step2": "A[::2]", "rev": "A[::-1]", "col1": "M[:, 1] of a C-ordered matrix",
         "fcol": "Fortran-ordered (n, 1)", "readonly": "read-only"}


def _buffer(vals, layout):
    """The buffer whose view(…, layout) holds vals."""
    n = len(vals)
    if layout == "step2":
        buf = np.zeros(2 * n, vals.dtype)
        buf[::2] = vals
        buf[1::2] = vals[::-1]
    elif layout == "col1":
        buf = np.stack([vals[::-1], vals, vals[::-1]], axis=1)
    elif layout == "fcol":
        buf = np.asfortranarray(vals.reshape(n, 1))
    else:
        buf = vals.copy()
    return buf


def view(buf, layout):
    """The call's argument: a view of the stored buffer (never a copy)."""
    if layout == "whole":
        return buf
    if layout == "step2":
        return buf[::2]
    if layout == "rev":
        return buf[::-1]
    if layout == "col1":
        return buf[:, 1]
    if layout == "fcol":
        assert buf.flags.f_contiguous and buf.ndim == 2
        return buf
    if layout == "readonly":
        v = buf.view()
        v.setflags(write=False)
        return v
    raise ValueError(layout)


def _make_layout(cid, dtype, lx, lz, nx=NX, nz=NZ):
    def make():
        rng = _rng(cid)
        if np.dtype(dtype).kind == "f":
            X, Z = rng.normal(0.5, 1, nx).round(1), rng.normal(0, 1, nz).round(1)
        else:
            X, Z = rng.randint(-9, 10, nx), rng.randint(-9, 10, nz)
        return {"X": _buffer(X.astype(dtype), lx), "Z": _buffer(Z.astype(dtype), lz)}
    return make


for _d in ("float64", "int64"):
    for _lay, _label in VIEWS.items():
        sides = (("readonly", "whole", "X"), ("whole", "readonly", "Z")) \
            if _lay == "readonly" else ((_lay, _lay, "X and Z"),)
        for _lx, _lz, _who in sides:
            for _fn, _col, _args in LAYOUT_FNS:
                _tag = f"{_d}-{_lay}" + (f"-{_who}" if _lay == "readonly" else "")
                _add(f"lay/{_tag}/{_col.replace(' ', '_')}", "layouts",
                     f"{_d}, {_who}: {_label}", _col, _fn, _args,
                     _make_layout(f"lay/{_tag}", _d, _lx, _lz),
                     "ValueError" if _lay == "readonly" else "exact", view=(_lx, _lz))
for _fn, _col, _args in LAYOUT_FNS:  # inputs rebuilt by make(), only hashes stored
    _add(f"lay/float64-step2-big/{_col.replace(' ', '_')}", "layouts",
         f"float64, X: A[::2] of {BIG} items (the device-shuffle size), Z contiguous", _col, _fn,
         _args, _make_layout("lay/float64-step2-big", "float64", "step2", "whole", nx=BIG),
         "exact", view=("step2", "whole"), stored=False)

# ------------------------------------------------------------------------- index arrays
INDEX_FNS = (("cs.UB_indices", "UB_indices AUC", {"kernel": "AUC"}),
             ("cs.UB_indices", "UB_indices prod", {"kernel": "prod"}),
             ("cs.conv_AUC_deter_pairs", "conv_AUC_deter_pairs(1)", {"margin": 1}))


def _make_index(cid, kind, pairs):
    def make():
        rng = _rng(cid)
        d = {"X": rng.normal(0.5, 1, NX).round(1), "Z": rng.normal(0, 1, NZ).round(1)}
        P = 30
        if kind == "negative":
            ix, iz = rng.randint(-NX, NX, P), rng.randint(-NZ, NZ, P)
        elif kind == "float64":
            ix, iz = rng.randint(0, NX, P).astype(float), rng.randint(0, NZ, P).astype(float)
        elif kind == "uint64 >= 2^63":
            ix = rng.randint(0, NX, P).astype(np.uint64)
            iz = rng.randint(0, NZ, P).astype(np.uint64)
            ix[3] = 2 ** 63 + 1
        elif kind == "bool mask" and not pairs:  # masks over X and Z with 9 True each
            ix, iz = np.zeros(NX, bool), np.zeros(NZ, bool)
            ix[rng.permutation(NX)[:9]] = True
            iz[rng.permutation(NZ)[:9]] = True
        elif kind == "bool mask":
            ix, iz = rng.rand(P) > 0.5, rng.rand(P) > 0.5
        else:
            ix, iz = rng.randint(0, NZ, P).astype(kind), rng.randint(0, NZ, P).astype(kind)
        d["ix"], d["iz"] = ix, iz
        return d
    return make


for _kind, _contract in (("int32", None), ("uint8", None), ("negative", None),
                         ("float64", "IndexError"), ("uint64 >= 2^63", "IndexError"),
                         ("bool mask", "NotImplementedError")):
    for _fn, _col, _args in INDEX_FNS:
        _tag = _kind.split(" ")[0]
        _pairs = _fn.endswith("pairs")
        _add(f"idx/{_tag}/{_col.replace(' ', '_')}", "index arrays", f"{_kind} indices", _col,
             _fn, _args, _make_index(f"idx/{_tag}/{_pairs}", _kind, _pairs),
             _contract or ("exact" if _col.endswith("AUC") else "rtol"))

BY_ID = {c.id: c for c in CELLS}

# the closed list of what may raise: exception -> the cells it is for
RAISING = {
    "TypeError": "bool - bool subtraction, as NumPy",
    "NotImplementedError": "integer kernel whose reference arithmetic wraps; float16 float "
                           "kernel; boolean mask as pair indices",
    "IndexError": "float or out-of-range index array, as NumPy",
    "ValueError": "read-only array in a shuffling call, as NumPy",
}


# ------------------------------------------------------------------------- running a cell
def arguments(cell, buffers):
    """(X, Z) as the call receives them: views of the buffers."""
    return view(buffers["X"], cell.view[0]), view(buffers["Z"], cell.view[1])


def run(api, cell, buffers):
    """Call cell.fn of `api` (a dict of the reference's, the oracle's or the drop-in's
    functions under the names used in CELLS) on views of `buffers`; returns the value."""
    a = cell.args
    X, Z = arguments(cell, buffers)
    if cell.fn == "est.Un":
        return api["est.Un"](X, Z)
    if cell.fn == "est.UnN":
        return api["est.UnN"](X, Z, a["N"], a["sampling"])
    if cell.fn == "cs.Un":
        return api["cs.Un"](X, Z, kernel=a["kernel"])
    if cell.fn == "cs.UnN":
        return api["cs.UnN"](X, Z, a["N"], a["sampling"], kernel=a["kernel"])
    if cell.fn == "cs.UnNB":
        return api["cs.UnNB"](X, Z, a["N"], a["B"], a["sampling"], kernel=a["kernel"])
    if cell.fn == "cs.conv_AUC":
        return api["cs.conv_AUC"](a["margin"])(X, Z)
    if cell.fn == "cs.UB_indices":
        return api["cs.UB_indices"](X, Z, buffers["ix"], buffers["iz"], a["kernel"])
    if cell.fn == "cs.conv_AUC_deter_pairs":
        pairs = list(zip(list(buffers["ix"]), list(buffers["iz"])))
        return api["cs.conv_AUC_deter_pairs"](a["margin"])(X, Z, pairs)
    if cell.fn == "est.replicate":
        extra = () if a["estimator"] == "Un" else (a["N"], a["sampling"])
        est = api["est." + a["estimator"]]
        if "est.replicate" in api:
            return np.array(api["est.replicate"](est, X.copy, Z.copy, a["n_tries"], *extra))
        return np.array([est(X.copy(), Z.copy(), *extra) for _ in range(a["n_tries"])])
    raise ValueError(cell.fn)


def seed_of(cell) -> int:
    return zlib.crc32(("seed/" + cell.id).encode()) % (2 ** 31)


def outcome(api, cell, buffers):
    """Run the cell under its seed: {"value"} or {"raises": class name}, and for every cell
    the RNG probe after the call (the buffers are changed in place, as the call leaves them)."""
    import warnings
    np.random.seed(seed_of(cell))
    out = {}
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        try:
            out["value"] = np.asarray(run(api, cell, buffers))
        except Exception as e:  # the class is the outcome
            out["raises"] = type(e).__name__
    out["probe"] = int(np.random.randint(0, 2 ** 31 - 1))
    return out


# ------------------------------------------------------------------------- stored fixtures
HERE = pathlib.Path(__file__).resolve().parent


def load_index() -> dict:
    return json.loads((HERE / "golden_dtypes.json").read_text())


def load_arrays() -> dict:
    with np.load(HERE / "golden_dtypes.npz", allow_pickle=False) as g:
        return {k: g[k] for k in g.files}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def same(a, b) -> bool:
    a, b = np.asarray(a), np.asarray(b)
    return (a.dtype == b.dtype and a.shape == b.shape
            and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"))


def load_buffers(arrays, entry, cell) -> dict:
    """The cell's input buffers: fresh copies with the stored dtype and byte order (a
    cell too large to store is rebuilt by make() and checked against the stored digests)."""
    if not cell.stored:
        buffers = cell.make()
        assert all(sha(a) == entry[f"sha_{k}"] for k, a in buffers.items())
        return buffers
    return {k: arrays[f"{cell.id}/{k}"].copy(order="K") for k in ("X", "Z", "ix", "iz")
            if f"{cell.id}/{k}" in arrays}


def check_state(arrays, entry, cell, buffers, probe) -> None:
    """The reference's side effects: the RNG probe after the call and, for sharded calls, the
    buffers — the original memory, not the views the call received."""
    assert probe == entry["probe"], "RNG consumption differs from the reference's"
    if cell.fn in SHARDED:
        for k in ("X", "Z"):
            if cell.stored:
                assert same(buffers[k], arrays[f"{cell.id}/{k}_after"]), f"{k} after the call"
            else:
                assert sha(buffers[k]) == entry[f"sha_{k}_after"], f"{k} after the call"


# ------------------------------------------------------------------------- INTEGRATION.md
def render_tables() -> str:
    """The contract tables of INTEGRATION.md §4, one per group: rows are dtype pairs (or
    layouts / index kinds), columns the functions, every entry one cell's contract."""
    out = []
    for group in dict.fromkeys(c.group for c in CELLS):
        cells = [c for c in CELLS if c.group == group]
        cols = list(dict.fromkeys(c.col for c in cells))
        out.append(f"**{group}** (X / Z)\n")
        out.append("| | " + " | ".join(f"`{c}`" for c in cols) + " |")
        out.append("|---|" + "---|" * len(cols))
        for row in dict.fromkeys(c.row for c in cells):
            by_col = {c.col: c.contract for c in cells if c.row == row}
            out.append(f"| {row} | " + " | ".join(by_col.get(c, "") for c in cols) + " |")
        out.append("")
    return "\n".join(out)
