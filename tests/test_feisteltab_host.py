"""The Feistel round tables of the chain emission (csrc/feistel.h feistel_round_table,
feistel_once32_tab) checked on the host: for half_bits 1 .. 11 and keys {0, 1,
2^64 - 1, three fixed random} every table entry is <= mask and the table-driven round network
equals feistel_once for every v of the domain.  tests/native/feisteltab_driver.cpp is compiled
host-only with the address and undefined-behaviour sanitizers (the table is a heap block of
exactly 6 << half_bits entries, so a lookup outside it is a finding) and run — no GPU needed.

The emission keeps fast_div32's f64 form (an exact 32-bit division was not built: DESIGN
§4.1c), so there is no integer-division check here."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "feisteltab_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("feisteltab") / "feisteltab_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{CSRC}", "-o", str(exe), str(SRC)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_round_tables_equal_the_arithmetic_rounds_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for hb in range(1, 12):
        assert f"ok tables half_bits={hb}" in lines, r.stdout
    assert "done" in lines
