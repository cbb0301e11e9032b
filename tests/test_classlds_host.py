"""The LDS-table form of the class loop (csrc/chainclass.h class_lds_encode / class_lds_decode,
class_lds_entry, class_gt32_lds, class_lds_runs) checked on the host under
AddressSanitizer and UBSan: for (NB, K) = (16, 4), (18, 6) and (20, 8) and random and extreme
plane words (all 0, all ones, one x per word, all x at the bound) and z images (0, the bound,
m 16^j + {-1, 0, 1} for every j and m = 1 .. 15) the table entry of the encoded word, carried
through the top-digit step, must equal class_gt32_wide and class_gt32_masked word for word, and
a zero-plane group must count nothing; the encoding must give a top digit below 16, an offset
that is a multiple of 512 and at most 255 * 512 and no other bit, and decode must reproduce the
low 12 bits; the 256-entry table of two groups must end at byte 131072; and the plan's regions
must be those of the wide plan.  tests/native/classlds_driver.cpp is compiled host-only and run
- no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "classlds_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("classlds") / "classlds_driver"
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", f"-I{CSRC}", "-o", str(exe), str(SRC)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_lds_table_equals_the_wide_digits_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for name in ("encoding", "table", "plan"):
        assert f"ok {name}" in lines, r.stdout
    for nb, k in ((16, 4), (18, 6), (20, 8)):
        assert any(l.startswith(f"ok words NB={nb} k={k} ") for l in lines), r.stdout
    assert "done" in lines
