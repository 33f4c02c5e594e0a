"""MPI_Alltoall / MPI_Alltoallv on device buffers (ompi_amd_alltoall*).

N ranks run tests/alltoall_worker.py, launched as tests/test_coll_gpu.py
launches its worker; N == 1 runs in this process.  Every rank computes its
expected rbuf in closed form and compares byte for byte.
"""
import json
import os
import secrets

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "alltoall_worker.py")
CASES = {"sizes", "misaligned", "inplace", "alltoallv_variants", "reuse", "nonblocking",
         "no_rendezvous", "persistent", "wait"}


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_alltoall_ranks(n):
    outs = run_ranks(n, timeout=240, worker=WORKER, tag="a2a")
    failures = []
    for r, (rc, out) in enumerate(outs):
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        bad = [ln for ln in lines if not ln["ok"]]
        missing = CASES - {ln["case"] for ln in lines}
        if rc != 0 or bad or missing:
            failures.append((r, rc, bad[:3], sorted(missing), out[-1500:] if rc not in (0, 1) or not lines else ""))
    assert not failures, failures


def test_alltoall_single_rank():
    """N == 1: a local copy of the rank's own block; in place a no-op."""
    from ompi_amd import coll
    comm = coll.Communicator(f"a2a1_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)
    try:
        src = torch.arange(1003, dtype=torch.int32, device="cuda").to(torch.uint8)
        dst = torch.full((1003 + 128,), 0xA5, dtype=torch.uint8, device="cuda")
        comm.alltoall(src, dst.data_ptr() + 64, 1003, blocking=True)
        got = dst.cpu().numpy()
        assert np.array_equal(got[64:64 + 1003], src.cpu().numpy())
        assert (got[:64] == 0xA5).all() and (got[64 + 1003:] == 0xA5).all()
        # alltoallv: 700 bytes from offset 5 of src to offset 9 of dst
        dst.fill_(0x5A)
        comm.alltoallv(src, [700], [5], dst, [700], [9], blocking=True)
        got = dst.cpu().numpy()
        assert np.array_equal(got[9:709], src.cpu().numpy()[5:705])
        assert (got[:9] == 0x5A).all() and (got[709:] == 0x5A).all()
        # in place: nothing moves
        keep = dst.clone()
        comm.alltoall(coll.IN_PLACE, dst, 1003, blocking=True)
        comm.alltoallv(coll.IN_PLACE, None, None, dst, [700], [9], blocking=True)
        r = comm.ialltoall(coll.IN_PLACE, dst, 1003)
        r.wait()
        r.free()
        assert torch.equal(dst, keep)
        plan = comm.alltoall_init(src, dst.data_ptr() + 64, 1003)
        plan.start()
        plan.wait()
        plan.free()
        assert np.array_equal(dst.cpu().numpy()[64:64 + 1003], src.cpu().numpy())
    finally:
        comm.free()


def test_alltoall_bad_params():
    """With a live communicator: NULL rbuf with bytes > 0 and NULL count
    arrays return BAD_PARAM from all six entry points, and no request or
    plan comes back; a zero-byte call with NULL buffers is legal."""
    import ctypes
    from ompi_amd import _lib, coll
    comm = coll.Communicator(f"a2abad_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)
    lib, h, BAD = comm._lib, comm._h, _lib.ERR_BAD_PARAM
    try:
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        s, r = buf.data_ptr(), buf.data_ptr() + 32
        cnt, dsp = (ctypes.c_size_t * 1)(8), (ctypes.c_size_t * 1)(0)
        zero = (ctypes.c_size_t * 1)(0)
        none = ctypes.POINTER(ctypes.c_size_t)()
        req, plan = ctypes.c_void_p(), ctypes.c_void_p()
        rq, pl = ctypes.byref(req), ctypes.byref(plan)
        # NULL rbuf with bytes > 0
        assert lib.ompi_amd_alltoall(h, s, None, 8, None) == BAD
        assert lib.ompi_amd_ialltoall(h, s, None, 8, None, rq) == BAD
        assert lib.ompi_amd_alltoall_init(h, s, None, 8, pl) == BAD
        assert lib.ompi_amd_alltoallv(h, s, cnt, dsp, None, cnt, dsp, None) == BAD
        assert lib.ompi_amd_ialltoallv(h, s, cnt, dsp, None, cnt, dsp, None, rq) == BAD
        assert lib.ompi_amd_alltoallv_init(h, s, cnt, dsp, None, cnt, dsp, pl) == BAD
        # NULL count arrays: each of the four, and the receive side in place
        for args in ((s, none, dsp, r, cnt, dsp), (s, cnt, none, r, cnt, dsp),
                     (s, cnt, dsp, r, none, dsp), (s, cnt, dsp, r, cnt, none),
                     (1, none, none, r, none, dsp), (1, none, none, r, cnt, none)):
            assert lib.ompi_amd_alltoallv(h, *args, None) == BAD, args
            assert lib.ompi_amd_ialltoallv(h, *args, None, rq) == BAD, args
            assert lib.ompi_amd_alltoallv_init(h, *args, pl) == BAD, args
        # NULL request / plan pointer
        assert lib.ompi_amd_ialltoall(h, s, r, 8, None, None) == BAD
        assert lib.ompi_amd_ialltoallv(h, s, cnt, dsp, r, cnt, dsp, None, None) == BAD
        assert lib.ompi_amd_alltoall_init(h, s, r, 8, None) == BAD
        assert lib.ompi_amd_alltoallv_init(h, s, cnt, dsp, r, cnt, dsp, None) == BAD
        assert not req.value and not plan.value
        assert comm.error() == 0
        # zero bytes: NULL buffers are fine
        assert lib.ompi_amd_alltoall(h, None, None, 0, None) == 0
        assert lib.ompi_amd_alltoallv(h, None, zero, dsp, None, zero, dsp, None) == 0
    finally:
        comm.free()
