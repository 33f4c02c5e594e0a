"""The typed rendezvous of point-to-point.  N ranks run tests/p2p_typed_rndv_worker.py under
each trigger, p2p_user_ipc = 1 and a pool that gives no stage (p2p_stage_mib = 0); every rank compares whole
buffers byte for byte with numpy and asserts the counters of the path each case names."""
import os

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402


@pytest.mark.parametrize("trigger", ["user_ipc", "no_stage"])
@pytest.mark.parametrize("n", [2, 3])
def test_p2p_typed_rndv(n, trigger):
    """8 KiB v64 -> v4; 1 MiB + 24 into a base 8 mod 16; 4100 B into a byte receive, and a byte rendezvous into a
    typed one (ANY_SOURCE / ANY_TAG); a stream ending inside a receive element; a 300-element program (a stage under
    p2p_user_ipc, UNSUPPORTED without one); 4096 B, still eager; MPI_Ssend; sendrecv_typed; a truncating receive."""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p2p_typed_rndv_worker.py")
    res = run_ranks(n, timeout=120, worker=worker, tag=f"p2prndv_{trigger}",
                    extra_env={"OMPI_AMD_RNDV_TRIGGER": trigger})
    assert not any(rc for rc, _ in res), [(r, rc, out[-1500:]) for r, (rc, out) in enumerate(res) if rc]
