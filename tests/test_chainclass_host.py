"""csrc/chainclass.h (the class-run form of the plane-reading chain count) checked
on the host: at NB in {16, 20, 24} and k in {1, 2, 6, 8} class bits, bits_carry(G, P, c_low)
must equal bits_gt32's carry bit for bit on random and boundary images (0, 2^NB - 1, multiples
of 2^(NB - k) and one less, x = z), x slots of 0 must count nothing, and a padded scalar slot
must be seen to count G (the reason the class loop takes exactly a run's images); the run table
of ragged class histograms under z chunks of 8, 600 and automatic must tile every class's range
exactly once with runs no longer than the chunk, within the stated capacity and the sized
regions; whole bags counted through the class form must equal the brute-force count.
tests/native/chainclass_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "chainclass_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("chainclass") / "chainclass_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o",
                        str(exe), str(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_chainclass_arithmetic_and_run_tables_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert any(l.startswith("ok tables") for l in lines), r.stdout
    for nb in (16, 20, 24):
        for k in (1, 2, 6, 8):
            assert any(l.startswith(f"ok arith NB={nb} k={k} ") for l in lines), r.stdout
            assert f"ok bags NB={nb} k={k}" in lines, r.stdout
