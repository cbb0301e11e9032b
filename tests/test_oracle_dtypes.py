"""The oracle pinned to REFERENCE runs over the dtype / layout matrix (CPU).

tests/golden/make_golden_dtypes.py ran every cell of tests/golden/dtype_cells.py through the
reference and stored inputs and outcomes; here the oracle's restatements run on the stored
inputs and must give the same outcome: value and dtype, the buffers after a sharded call, the
RNG probe, or the exception's class.  That pins the oracle for these dtypes and shows that
the fixtures hold for the NumPy installed where the tests run.  The GPU twin is
test_gpu_dtypes.py; the matrix bookkeeping (INTEGRATION.md's tables, the closed list of
raising cells) is checked here too.
"""
import pathlib

import numpy as np
import pytest

from oracle import oracle as O
from golden import dtype_cells as DC

HERE = pathlib.Path(__file__).resolve().parent / "golden"
ROOT = HERE.parents[1]
INDEX = DC.load_index()
IDS = [c.id for c in DC.CELLS]

ORACLE_API = {
    "est.Un": O.est_Un, "est.UnN": O.est_UnN, "cs.Un": O.cs_Un, "cs.UnN": O.cs_UnN,
    "cs.UnNB": O.cs_UnNB, "cs.conv_AUC": O.conv_AUC, "cs.UB_indices": O.UB_indices,
    "cs.conv_AUC_deter_pairs": O.conv_AUC_deter_pairs,
}


@pytest.fixture(scope="module")
def stored():
    return DC.load_arrays()


def test_index_matches_cell_list():
    assert list(INDEX) == IDS
    for c in DC.CELLS:
        e = INDEX[c.id]
        assert (e["fn"], e["args"], tuple(e["view"]), e["contract"], e["seed"]) == (
            c.fn, c.args, c.view, c.contract, DC.seed_of(c)), c.id


@pytest.mark.parametrize("cid", IDS)
def test_oracle_restates_reference(stored, cid):
    cell = DC.BY_ID[cid]
    entry = INDEX[cid]
    buffers = DC.load_buffers(stored, entry, cell)
    assert [DC._name(buffers[k].dtype) for k in ("X", "Z")] == entry["dtypes"]
    out = DC.outcome(ORACLE_API, cell, buffers)
    assert out.get("raises") == entry.get("raises")
    if "raises" not in entry:
        assert DC.same(out["value"], stored[f"{cid}/value"]), (out["value"], stored[f"{cid}/value"])
    DC.check_state(stored, entry, cell, buffers, out["probe"])


# ------------------------------------------------------------------ the matrix's own rules
def test_a_returning_contract_means_the_reference_returned():
    for c in DC.CELLS:
        if c.contract in ("exact", "rtol", "rtol32"):
            assert "raises" not in INDEX[c.id], c.id


def test_raising_cells_are_the_closed_list():
    """Only the kinds of cell INTEGRATION.md §4 names may raise, and every integer float-kernel
    cell that raises has a sibling of the same dtypes and function that must return."""
    for c in DC.CELLS:
        if c.contract in ("exact", "rtol", "rtol32"):
            continue
        assert c.contract in DC.RAISING, c.id
        dx, dz = INDEX[c.id]["dtypes"]
        if c.contract == "TypeError":  # bool - bool, where NumPy raises the same
            assert dx == dz == "bool" and INDEX[c.id]["raises"] == "TypeError", c.id
        elif c.contract == "ValueError":
            assert "readonly" in c.view and INDEX[c.id]["raises"] == "ValueError", c.id
        elif c.contract == "IndexError":
            assert c.group == "index arrays" and INDEX[c.id]["raises"] == "IndexError", c.id
        elif c.group == "index arrays":
            assert c.row == "bool mask indices", c.id
        elif "float16" in (dx, dz):
            assert c.group == "float kernels", c.id
        else:  # an integer kernel whose reference arithmetic wraps
            assert np.dtype(dx).kind in "iu" and np.dtype(dz).kind in "iu", c.id
            siblings = [s for s in DC.CELLS if s.fn == c.fn and s.args == c.args
                        and INDEX[s.id]["dtypes"] == [dx, dz]
                        and s.contract in ("exact", "rtol")]
            assert siblings, c.id


def test_integration_md_tables_agree_with_the_cell_list():
    text = (ROOT / "INTEGRATION.md").read_text()
    for line in DC.render_tables().splitlines():
        assert line in text, line
    # and no contract row of the document is left over from an older list
    start = text.index("<!-- dtype contract: begin -->")
    stop = text.index("<!-- dtype contract: end -->")
    rows = [ln for ln in text[start:stop].splitlines() if ln.startswith("|")]
    assert rows == [ln for ln in DC.render_tables().splitlines() if ln.startswith("|")]
