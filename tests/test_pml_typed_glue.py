"""pml/rocm's typed point-to-point route (ROCM_HAVE_TYPED_P2P) compiles against the
harness's stand-in headers with the pml harness's own warning flags, with the macro and without."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = os.path.join(ROOT, "tests", "mca_harness")


@pytest.mark.parametrize("macro", [[], ["-DROCM_HAVE_TYPED_P2P"]])
def test_pml_rocm_compiles(macro):
    src = os.path.join(ROOT, "ompi_amd", "mca", "pml", "rocm")
    inc = [os.path.join(H, d) for d in ("pml_include", "coll_include", "include")] + [os.path.join(ROOT, "include"), src]
    cmd = ["gcc", "-fsyntax-only", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
           "-Wno-missing-field-initializers", "-DHARNESS_COLL"] + macro
    r = subprocess.run(cmd + [f"-I{d}" for d in inc] + [os.path.join(src, "pml_rocm.c")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
