"""The forward's host decisions (3dgs_amd/csrc/gs_forward_plan.h: compacted walk, sort class, redone tail, tile order,
forward split, segment room, figure slots, the host record) on hand-worked cases: tests/cpp/forward_plan_test.cpp, built
by the host compiler alone with the address and undefined-behaviour sanitizers and run as a stand-alone program."""
import os
import subprocess

from conftest import ROOT


def test_forward_plan_header_on_worked_cases(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "forward_plan_test.cpp")
    exe = str(tmp_path / "forward_plan_test")
    # (the sanitizer runtimes linked into the program: it then runs whatever else the loader brings in first)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-I", os.path.join(ROOT, "3dgs_amd", "csrc"), src, "-o", exe],
                        capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stderr[-3000:]
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "all checks passed" in out.stdout
