"""The granule and walk rule of the copies with a datatype on both ends (coll_typed.h's
typed_granule2 / typed_walk64_2), checked on the host by a stand-alone program."""
import os
import shutil
import subprocess


def test_typed_rule2(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe, src = str(tmp_path / "typed_rule2_check"), os.path.join(os.path.dirname(os.path.abspath(__file__)), "harness",
                                                                 "typed_rule2_check.cpp")
    cc = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", src, "-o", exe], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-1500:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout[-1500:]
