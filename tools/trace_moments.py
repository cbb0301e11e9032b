"""The moments' sorted path and the sorted count, a few launches each at 64 x 15625^2, 1 x 1e6^2
and 1 x 1e5^2, as the program of a kernel trace (GPU box):
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/trace_moments.py
    python tools/kernel_seq_stats.py OUT/.../run_kernel_trace.csv > profiles/time_moments_kernel_trace.txt"""
import pathlib
import sys

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tuplewise import _engine as E  # noqa: E402
from tuplewise import _lib as L  # noqa: E402

torch.cuda.set_device(0)
for blocks, n, reps in ((64, 15625, 10), (1, 1_000_000, 4), (1, 100_000, 10)):
    rng = np.random.RandomState(1)
    xs = [rng.normal(0.5, 1, n) for _ in range(blocks)]
    zs = [rng.normal(0.0, 1, n) for _ in range(blocks)]
    sh = E.Shards.from_blocks(xs, zs, L.TW_F64)
    xo, zo = sh.offsets_dev()
    for _ in range(reps):
        out = E.moments_launch(sh.x, xo, sh.z, zo, blocks, n, n, blocks * n, blocks * n,
                               L.TW_F64, L.TW_PRED_GT, "sorted")
    torch.cuda.synchronize()
    for _ in range(reps):
        cnt = E.count_launch(sh.x, xo, sh.z, zo, blocks, n, n, L.TW_F64, L.TW_PRED_GT, "sorted")
    torch.cuda.synchronize()
print("done")
