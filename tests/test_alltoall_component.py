"""coll/rocm's alltoall / alltoallv slots through tests/mca_harness_alltoall:
the glue compiled with HARNESS_COLL + HARNESS_COLL_ALLTOALL against the
stand-in coll.h that has the six slots, and driven through module_enable
with recording saved functions."""
import os
import subprocess

import pytest

from test_mca_glue import _assert_all, _run_coll_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "mca_harness_alltoall", "build.sh")


def test_glue_compiles_clean_with_alltoall_slots():
    """-Wall -Wextra -Werror, no diagnostics."""
    r = subprocess.run(["bash", BUILD, "--syntax"], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


@pytest.fixture(scope="module")
def a2a_harness(tmp_path_factory):
    from ompi_amd import _lib
    _lib.load()
    out = str(tmp_path_factory.mktemp("mca_a2a") / "a2a_harness")
    subprocess.run(["bash", BUILD, out], check=True)
    return out


def test_alltoall_slots_offered(a2a_harness):
    _assert_all(_run_coll_harness(a2a_harness, 2, False, 60), "ok")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_alltoall_component_device_path(a2a_harness, n):
    """Device buffers take the device path (saved function not called, exact);
    host buffers and unequal byte counts reach the saved function; a
    vector-typed send operand is packed and exact; ialltoallv and the
    persistent forms complete through their requests."""
    _assert_all(_run_coll_harness(a2a_harness, n, True, 120), "ok gpu")
