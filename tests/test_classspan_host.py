"""The span items of the class count (csrc/chainclass.h class_span_clamp, class_spans,
class_span_entries, class_span_item, class_span_auto, class_plan's span) checked
on the host: the slots of a launch visit every run-table entry of every bag exactly once per x
tile and none past the bag's count, for entry counts 0, 1, M - 1, M, M + 1 and cap, every M in
1 .. cap and tables built from class histograms (classes of several runs, only the first or only
the last class non-empty, bags of different counts in one launch); one lane's walk over a span
— low digit tables once, G, P, E and the top digit per run of a new class, len * popc(G) per
run, u32 lane sums — adds up to the brute-force count for random and edge images and every M;
and the plan carries the clamped span, with the automatic rule 1 for small launches.
tests/native/classspan_driver.cpp is compiled host-only and run — no GPU needed."""
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "trade-offs-in-distributed-tuplewise-estimation-and-learning_amd" / "csrc"
SRC = ROOT / "tests" / "native" / "classspan_driver.cpp"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed"
    exe = tmp_path_factory.mktemp("classspan") / "classspan_driver"
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-fsanitize=undefined", "-fno-sanitize-recover=all", f"-I{CSRC}", "-o",
                        str(exe), str(SRC)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return exe


def test_spans_visit_every_entry_once_and_walk_to_the_brute_force_count(driver):
    r = subprocess.run([str(driver)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    for name in ("decode", "plan"):
        assert f"ok {name}" in lines, r.stdout
    for nb, k in ((20, 8), (16, 4), (16, 8), (18, 6)):
        assert f"ok walk NB={nb} k={k}" in lines, r.stdout
    assert "done" in lines
