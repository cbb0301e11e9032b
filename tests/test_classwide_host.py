"""The wide-digit split of the class loop (csrc/chainclass.h class_wide_encode / class_wide_of,
class_wide_tables, class_gt32_wide, the wide register map) checked on the host
under AddressSanitizer and UBSan: for (NB, K) = (16, 4), (18, 6) and (20, 8) and random and
extreme plane words (all 0, all ones, one x per word, all x at the bound) and z images (0, the
bound, m 16^j + {-1, 0, 1} for every j and m = 1 .. 15) the wide lookup must equal
class_gt32_masked — and so the four-digit lookup — word for word and a padded x slot must count
nothing; the encoding must give digits below 16 with byte 3 zero and reproduce the low 12 bits,
and class_wide_of of any word must be below 16; the register map must be 50 per group and end at
v123 for two groups; and the plan's regions must be disjoint and those of the four-digit plan.
tests/native/classwide_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "classwide_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("classwide") / "classwide_driver"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", f"-I{CSRC}", "-o", str(exe), str(SRC)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_wide_digits_equal_the_masked_planes_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for name in ("map", "encoding", "plan"):
        assert f"ok {name}" in lines, r.stdout
    for nb, k in ((16, 4), (18, 6), (20, 8)):
        assert any(l.startswith(f"ok words NB={nb} k={k} ") for l in lines), r.stdout
    assert "done" in lines
