"""coll/rocm's allgatherv / gather(v) / scatter(v) slots through
tests/mca_harness_gather: the glue compiled with HARNESS_COLL +
HARNESS_COLL_GATHER against the stand-in coll.h that has the fifteen slots,
and driven through module_enable with recording saved functions.  (The same
file against the framework's real coll.h: tests/test_real_headers.py.)"""
import os
import subprocess

import pytest

from test_mca_glue import _assert_all, _run_coll_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "mca_harness_gather", "build.sh")


def test_glue_compiles_clean_with_gather_slots():
    """-Wall -Wextra -Werror, no diagnostics."""
    r = subprocess.run(["bash", BUILD, "--syntax"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


@pytest.fixture(scope="module")
def gather_harness(tmp_path_factory):
    from ompi_amd import _lib
    _lib.load()
    out = str(tmp_path_factory.mktemp("mca_gather") / "gather_harness")
    subprocess.run(["bash", BUILD, out], check=True)
    return out


def test_gather_slots_offered(gather_harness):
    _assert_all(_run_coll_harness(gather_harness, 2, False, 60), "ok")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_gather_component_device_path(gather_harness, n):
    """Device buffers take the device path through all fifteen slots (saved
    function not called, exact, 4-byte and 16-byte elements, the root in
    place, requests complete and free); host buffers reach the saved
    function."""
    _assert_all(_run_coll_harness(gather_harness, n, True, 120), "ok gpu")
