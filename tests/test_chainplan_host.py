"""csrc/chainplan.h (the work items of the plane-reading chain count) checked on
the host: for (nx, nz) over {0, 1, 63, 2047, 2048, 2049, 4101, 15625, 100000}^2, R in {2, 3, 4}
and z chunks of 8, 600 and automatic, every item of the plan is enumerated and the rectangles
must tile nx x nz exactly once (alone and as a ragged bag of a larger launch), the swap rule
must pick the side with fewer slots, and the padded slots must equal the closed form; the plane
layout helpers are checked against bits_transpose32 on random images at every plane count;
chain_count_sliced (which bounded launches run bit-sliced, which packed) is pinned at the
thresholds of its padding rule, under every forced plan, half ties and a bound of 2^24.
tests/native/chainplan_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "chainplan_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("chainplan") / "chainplan_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o",
                        str(exe), str(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_chainplan_items_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert any(l.startswith("ok plans") for l in lines), r.stdout
    assert "ok decision" in lines, r.stdout
    for nb in (16, 18, 20, 22, 24):
        assert f"ok layout NB={nb}" in lines, r.stdout
