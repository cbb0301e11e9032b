"""The fused pre-pass grid of the chain count (csrc/chainclass.h prepass_grid / prepass_role,
DESIGN §4.1l) checked on the host: at 1, 2, 63, 64 and 2048 bags and gx + gz of 1, 8 and 9
every block of the computed grid has exactly one role, every bag exactly one z-class block, and
every (bag, group, side) of k_chain_planes' own grid exactly one wave, at the workspace group it
had; the grid bound fires where the summed grid passes 2^31 - 1; the register-resident sort's
images per thread at its thresholds; class_run32 equals class_run.
tests/native/chainprepass_driver.cpp is compiled host-only under UBSan and ASan and run — no
GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "chainprepass_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("chainprepass") / "chainprepass_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{CSRC}", "-o", str(exe), str(SRC)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_prepass_grid_roles_and_bound_on_the_host(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for bags in (1, 2, 63, 64, 2048):
        for gx, gz in ((1, 0), (0, 1), (8, 0), (5, 3), (8, 1), (4, 5)):
            assert any(l.startswith(f"ok roles bags={bags} gx={gx} gz={gz} ") for l in lines), \
                r.stdout
    for tag in ("ok bound", "ok forms", "ok runs32"):
        assert tag in lines, r.stdout
