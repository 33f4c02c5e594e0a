"""One-sided calls with a derived datatype on the origin or result side.  N ranks run
tests/osc_ddt2_worker.py: put + get through two programs (one granule; two programs in LDS; 1 MiB + 64 over more
than 32 workgroups into a base 8 mod 16; a 300-element program walked from global memory; a contiguous target; the
caller's own window; param osc_ddt_fuse = 0), then accumulate and get_accumulate through up to three programs (one
element; 256 x 4 + 1; three different types; fp64; a one-byte type on the global walk; REPLACE and NO_OP; every
rank onto rank 0).  Every rank compares whole buffers byte for byte with numpy and asserts the osc_ddt_* counters.
The second environment is the 64-bit walk on a two-workgroup grid."""
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402


@pytest.mark.parametrize("env", [{}, {"OMPI_AMD_OSC_DDT_FAST": "0", "OMPI_AMD_OSC_MAX_BLOCKS": "2"}],
                         ids=["fast", "walk64_two_groups"])
@pytest.mark.parametrize("n", [2, 3])
def test_osc_ddt2(n, env):
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "osc_ddt2_worker.py")
    res = run_ranks(n, timeout=120, worker=worker, tag=f"oscddt2_{len(env)}", extra_env=env)
    assert not any(rc for rc, _ in res), [(r, rc, out[-1500:]) for r, (rc, out) in enumerate(res) if rc]
