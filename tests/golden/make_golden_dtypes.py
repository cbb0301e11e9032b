"""Generate the dtype / layout fixtures by running the REFERENCE implementation (CPU only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dtypes.py

Imports the reference read-only (as make_golden.py does) and runs every cell of
tests/golden/dtype_cells.py through it.  golden_dtypes.npz receives, per cell, the input
buffers with their exact dtype and byte order, the reference's return value with its dtype
and, for sharded calls, the buffers after the call; golden_dtypes.json the index: function,
arguments, contract, seed, RNG probe after the call, and the exception's class name where the
reference raises.  The cells whose X is too large to store keep SHA-256 digests instead
(their buffers are rebuilt by the seeded make()).  golden.npz is not touched.
"""
from __future__ import annotations

import hashlib
import json
import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import dtype_cells as DC  # noqa: E402
from make_golden import REF, _load  # noqa: E402


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def reference_api():
    sys.dont_write_bytecode = True
    est = _load("ref_est_main", REF / "estimation-experiment" / "main.py")
    cs = _load("ref_compute_stats", REF / "learning-experiment" / "compute_stats.py")
    return {"est.Un": est.Un, "est.UnN": est.UnN, "cs.Un": cs.Un, "cs.UnN": cs.UnN,
            "cs.UnNB": cs.UnNB, "cs.conv_AUC": cs.conv_AUC, "cs.UB_indices": cs.UB_indices,
            "cs.conv_AUC_deter_pairs": cs.conv_AUC_deter_pairs}


def main():
    api = reference_api()
    arrays, index = {}, {}
    for cell in DC.CELLS:
        buffers = cell.make()
        entry = {"fn": cell.fn, "args": cell.args, "view": list(cell.view),
                 "contract": cell.contract, "seed": DC.seed_of(cell),
                 "dtypes": [DC._name(buffers["X"].dtype), DC._name(buffers["Z"].dtype)]}
        for k, a in buffers.items():
            if cell.stored:
                arrays[f"{cell.id}/{k}"] = a.copy(order="K")
            else:
                entry[f"sha_{k}"] = sha(a)
        out = DC.outcome(api, cell, buffers)
        entry["probe"] = out["probe"]
        if "raises" in out:
            entry["raises"] = out["raises"]
        else:
            arrays[f"{cell.id}/value"] = out["value"]
        if cell.fn in DC.SHARDED:
            for k in ("X", "Z"):
                if cell.stored:
                    arrays[f"{cell.id}/{k}_after"] = buffers[k]
                else:
                    entry[f"sha_{k}_after"] = sha(buffers[k])
        index[cell.id] = entry
    np.savez_compressed(HERE / "golden_dtypes.npz", **arrays)
    (HERE / "golden_dtypes.json").write_text(json.dumps(index, indent=1))
    print(f"wrote {len(arrays)} arrays for {len(index)} cells to {HERE / 'golden_dtypes.npz'}")


if __name__ == "__main__":
    main()
