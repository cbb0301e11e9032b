"""The digit-table form of the class loop (csrc/chainclass.h class_digit_table,
class_digit_tables, class_digit_encode / class_digit_of, class_gt32_digits) checked
on the host: for every (NB, K) the tables take (4 <= NB - K <= 12: NB = 16 at K = 4 .. 8, 18 at
6 .. 8, 20 at 8) and random and extreme plane words (all 0, all ones, one x per word, ties, all x
at the bound) and z images (0, the bound, every digit boundary), the table lookup must equal
class_gt32_masked word for word and a padded x slot must count nothing; the digit-ready encoding
must reproduce the low NL bits with every digit below 2^w and class_digit_of of any word below
8; the digit split must fit the device loop's 36 table registers per group; and the regions of
a launch must be disjoint with the over-read past the last run of the last bag inside the
workspace.  tests/native/classdigit_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "classdigit_driver.cpp"
FORM3 = {16: range(4, 9), 18: range(6, 9), 20: range(8, 9)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("classdigit") / "classdigit_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o",
                        str(exe), str(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_digit_tables_equal_the_masked_planes_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for name in ("split", "encoding", "layout"):
        assert f"ok {name}" in lines, r.stdout
    for nb in (16, 18, 20):
        for k in range(1, 9):
            if k in FORM3[nb]:
                assert any(l.startswith(f"ok words NB={nb} k={k} ") for l in lines), r.stdout
            else:
                assert f"ok skip NB={nb} k={k} (form 2)" in lines, r.stdout
    assert "done" in lines
