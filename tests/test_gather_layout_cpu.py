"""The landing layouts of allgatherv / gather(v) / scatter(v)
(ompi_amd/csrc/coll_landing.h) checked by tests/harness/gather_layout_check.cpp:
a stand-alone host program, built with the address and undefined-behaviour
sanitizers where their runtimes link (without them otherwise), then run."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "gather_layout_check.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_gather_layouts(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "gather_layout_check")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe]
    errs = []
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE, []):
        cc = subprocess.run(base + extra, capture_output=True, text=True)
        if cc.returncode == 0:
            break
        errs.append(cc.stderr[-1500:])
    assert cc.returncode == 0, "\n".join(errs)
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "gather layouts ok" in run.stdout
