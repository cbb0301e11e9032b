"""csrc/bitcount.h (the bit-sliced compare-and-count of DESIGN §4.1e) checked on the host: the
32 x 32 bit transpose, the carry chain against x > z (exhaustively at 8 planes, randomly with
ties, 0 and 2^NB - 1 at every instantiated plane count), the popcount accumulate and the image
conversions.  tests/native/bitcount_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "bitcount_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("bitcount") / "bitcount_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=undefined",
                        "-fno-sanitize-recover=all", f"-I{CSRC}", "-o", str(exe), str(SRC)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_bitcount_helpers_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for name in ["transpose", "exhaustive NB=8", "random NB=16", "random NB=18", "random NB=20",
                 "random NB=22", "random NB=24", "images"]:
        assert f"ok {name}" in lines, r.stdout
