"""coll/rocm's typed exchange path (ROCM_HAVE_TYPED_XCH) through
tests/mca_harness_typed: the glue compiled with the macro and both groups of
exchange slots against stand-in headers whose gapped datatype carries a
device program (a stand-in opal_rocm_device_ddt), and driven through
module_enable with recording saved functions."""
import os
import subprocess

import pytest

from test_mca_glue import _assert_all, _run_coll_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "mca_harness_typed", "build.sh")


@pytest.mark.parametrize("mode", ["--syntax", "--syntax-without"])
def test_glue_compiles_clean_with_and_without_typed_xch(mode):
    """-Wall -Wextra -Werror, no diagnostics, with ROCM_HAVE_TYPED_XCH and,
    against the same headers, without it."""
    r = subprocess.run(["bash", BUILD, mode], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr


@pytest.fixture(scope="module")
def typed_harness(tmp_path_factory):
    from ompi_amd import _lib
    _lib.load()
    out = str(tmp_path_factory.mktemp("mca_typed") / "typed_harness")
    subprocess.run(["bash", BUILD, out], check=True)
    return out


def test_typed_build_offers_the_exchange_slots(typed_harness):
    _assert_all(_run_coll_harness(typed_harness, 2, False, 60), "ok")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [2, 3])
def test_typed_component_device_path(typed_harness, n):
    """Seven collectives x three forms: a non-contiguous device operand (send
    side, receive side, both, odd ranks only, in place) completes exactly,
    leaves every gap of a typed receive operand untouched, never reaches the
    saved function and moves the module's typed_calls counter; a type without
    a device program takes the packed path, exact, counter unmoved."""
    _assert_all(_run_coll_harness(typed_harness, n, True, 120), "ok gpu")
