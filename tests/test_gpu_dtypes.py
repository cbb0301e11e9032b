"""The drop-in API's dtype and layout contract against the reference (MI355X).

Every cell of tests/golden/dtype_cells.py (the list INTEGRATION.md §4 prints) is one call of
the drop-in on inputs the reference was run on (tests/golden/golden_dtypes.npz, made by
make_golden_dtypes.py; test_oracle_dtypes.py is the CPU twin).  The drop-in must do exactly
one of two things:

  return the reference's result: identical in value and dtype where the value derives from
  a count ("exact"), within the suite's FLOAT_RTOL for float kernels on float64 or exactly
  representable integers ("rtol"), within the suite's 1e-5 for float32 ("rtol32"); after a
  sharded call the caller's buffers, read through the original memory, and the RNG probe are
  identical;

  or raise the exception the contract names.  Where the reference raised that exception too
  (read-only arrays, float indices), buffers and RNG are as the reference left them.

A different number is never accepted.
"""
import numpy as np
import pytest

from golden import dtype_cells as DC

pytestmark = pytest.mark.gpu

INDEX = DC.load_index()
FLOAT_RTOL = 1e-12  # test_gpu_parity.py's bars, not new ones
FLOAT32_RTOL = 1e-5
assert DC.RTOL == {"rtol": FLOAT_RTOL, "rtol32": FLOAT32_RTOL}


@pytest.fixture(scope="module")
def stored():
    return DC.load_arrays()


@pytest.fixture(scope="module")
def dropin(gpu):
    import tuplewise.compute_stats as cs
    import tuplewise.estimation as est
    return {"est.Un": est.Un, "est.UnN": est.UnN, "est.replicate": est.replicate,
            "cs.Un": cs.Un, "cs.UnN": cs.UnN, "cs.UnNB": cs.UnNB, "cs.conv_AUC": cs.conv_AUC,
            "cs.UB_indices": cs.UB_indices, "cs.conv_AUC_deter_pairs": cs.conv_AUC_deter_pairs}


@pytest.mark.parametrize("cid", [c.id for c in DC.CELLS])
def test_cell(dropin, stored, cid):
    cell = DC.BY_ID[cid]
    entry = INDEX[cid]
    assert entry["contract"] == cell.contract
    buffers = DC.load_buffers(stored, entry, cell)
    out = DC.outcome(dropin, cell, buffers)
    if cell.contract not in DC.RTOL and cell.contract != "exact":
        assert out.get("raises") == cell.contract, out
        if entry.get("raises") == cell.contract:  # the reference's own exception: its state too
            DC.check_state(stored, entry, cell, buffers, out["probe"])
        return
    assert "raises" not in out, out
    got, want = out["value"], stored[f"{cid}/value"]
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype)
    if cell.contract == "exact":
        assert np.array_equal(got, want), (got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=DC.RTOL[cell.contract], atol=0)
    DC.check_state(stored, entry, cell, buffers, out["probe"])


def test_strided_sample_of_device_shuffle_size_is_not_device_shuffled(gpu):
    """The big strided cell is the device-shuffle path's own eligibility check at work: the
    same sample, contiguous, takes that path; as a strided view it must not."""
    from tuplewise import _blocks as Bk, _multi as M
    cell = DC.BY_ID["lay/float64-step2-big/est.UnN_prop-SWOR"]
    X, Z = DC.arguments(cell, cell.make())
    spec = Bk.CompleteCount(literal_sub=False)
    assert X.shape[0] >= Bk.DEVICE_SHUFFLE_MIN
    if len(M.devices()) < 2:  # (several devices: the path also weighs a multi-device split)
        assert Bk._device_shuffle_ok(np.ascontiguousarray(X), Z, spec)
    assert not Bk._device_shuffle_ok(X, Z, spec)
