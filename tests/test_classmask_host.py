"""The masked-plane form of the class loop (csrc/chainclass.h class_equal_mask,
class_mask_planes, class_gt32_masked) checked on the host: at NB in {16, 20, 24}
and every k from 1 to 8, for random and adversarial plane words (all x equal to z; x equal in
the top field and -1 / +1 in the low field; x = 0 padded slots against z image 0; all x at the
bound) and every z, the class-constant term popc(G) plus the word from the planes ANDed with
E = P & ~G must give the count of class_gt32 and of a per-image integer compare, bit for bit;
runs of length 1, 2 and 3 — the class of three z beside the class of one included — must count
len * popc(G) + the words with len the exact length, and one slot more must be seen to
over-count.  tests/native/classmask_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "classmask_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("classmask") / "classmask_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o",
                        str(exe), str(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_masked_planes_and_constant_term_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for nb in (16, 20, 24):
        for k in range(1, 9):
            assert any(l.startswith(f"ok words NB={nb} k={k} ") for l in lines), r.stdout
            assert f"ok runs NB={nb} k={k}" in lines, r.stdout
    assert "done" in lines
