"""The convertor's host arithmetic: the staged tile's planning
(ompi_amd/csrc/ddt_plan.h: the settings' accepted ranges, the period
choice, periods per tile and the LDS request) checked by
tests/harness/ddt_plan_check.cpp: a stand-alone host program, built with the
address and undefined-behaviour sanitizers where their runtimes link (without
them otherwise), then run.  Every accepted
setting must give a launch a gfx950 workgroup can hold (160 KiB of LDS).
The same program checks make_fdiv with fdiv_q (the multiply-high division of
OMPI_AMD_DDT_FASTDIV=1, restated for the host) against integer division."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "ddt_plan_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


@pytest.fixture(scope="module")
def check_run(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("ddt_plan")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ddt_plan_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe]
    errs = []
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        cc = subprocess.run(base + extra, capture_output=True, text=True)
        if cc.returncode == 0:
            break
        errs.append(cc.stderr[-1500:])
    assert cc.returncode == 0, "\n".join(errs)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return run


def test_ddt_tile_plans(check_run):
    run = check_run
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "ddt plans ok" in run.stdout


def test_fast_division_exact(check_run):
    run = check_run
    assert "fdiv ok" in run.stdout, run.stdout[-2000:] + run.stderr[-4000:]
