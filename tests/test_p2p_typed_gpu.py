"""Typed point-to-point on the device (ompi_amd_isend_typed and its kin): the
kernels that move a message walk its derived datatype.  N ranks run tests/p2p_typed_worker.py;
every rank compares whole buffers byte for byte with a numpy pack / unpack and asserts the
counter of the path each case names."""
import ctypes
import os
import secrets

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "p2p_typed_worker.py")


@pytest.mark.parametrize("n", [1, 2, 3])
def test_p2p_typed(n):
    """The worker's table: 4 B in one lane; 4096 B (the eager limit) out of 16-B runs into a
    struct of the same signature at G 4 — {4 B, gap, 8 B, gap, 4 B}, since {4 B, gap, 8 B} is
    12 B and does not divide 4096; 4100 B (the first staged size) from a 1-B indexed type into
    bytes and from bytes into 2-B runs, received with ANY_SOURCE / ANY_TAG; 1 MiB + 24 in 33
    workgroups into a base that is 8 mod 16, ending 8 B into a 16-B run; a 65532-B stream of
    12-B structs that ends inside a receiver element of two of them, capacity 96 KiB; a
    300-element program walked from global memory, two messages received in order; the forced
    64-bit walk; a message longer than the receive (TRUNCATE)."""
    res = run_ranks(n, timeout=120, worker=WORKER, tag="p2ptyped")
    assert not any(rc for rc, _ in res), [(r, rc, out[-1500:]) for r, (rc, out) in enumerate(res) if rc]


def test_p2p_typed_refusals():
    """BAD_PARAM for what the byte forms refuse, a host buffer, a datatype with a negative
    extent, and count * size past SIZE_MAX; UNSUPPORTED under p2p_user_ipc = 1 and from a pool
    without a stage, from sendrecv_typed too, which then has matched no message.  After every
    refusal no request came back and no counter has moved; count 0 is a zero-byte message.
    (A datatype handle that is no valid device program is not among them: both create calls
    refuse an empty or malformed element list, so no test can hold such a handle.)"""
    from ompi_amd import _lib, coll, datatype as dt
    comm = coll.Communicator(f"p2ptbad_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)
    lib, h, BAD = comm._lib, comm._h, _lib.ERR_BAD_PARAM
    try:
        buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")  # holds every span named below
        host = torch.zeros(4096, dtype=torch.uint8)
        V = dt.from_runs("v12", [(0, 4)], 12)
        NEG = dt.type_create_resized(V, 0, -12)  # (named: a Datatype destroys its program when collected)
        v, neg = (t.commit()._handle for t in (V, NEG))
        d, hp = buf.data_ptr(), host.data_ptr()
        # buf, count, ddt, peer, tag
        bad = [(hp, 3, v, 0, 1), (d, 3, neg, 0, 1), (d, 1 << 62, v, 0, 1), (None, 3, v, 0, 1),
               (d, 3, v, 1, 1), (d, 3, v, 0, -2), (hp, 3, None, 0, 1)]

        def calls(args, mode=4):
            b, cnt, t, peer, tag = args
            req = [ctypes.c_void_p(0), ctypes.c_void_p(0)]
            got = (lib.ompi_amd_isend_typed(h, b, cnt, t, peer, tag, mode, None, ctypes.byref(req[0])),
                   lib.ompi_amd_irecv_typed(h, b, cnt, t, peer, tag, None, ctypes.byref(req[1])),
                   lib.ompi_amd_send_typed(h, b, cnt, t, peer, tag, mode, None),
                   lib.ompi_amd_sendrecv_typed(h, b, cnt, t, peer, tag, b, cnt, t, peer, tag, None, None))
            return got, [r.value for r in req]

        def unmoved():
            return comm.error() == 0 and all(comm.get_param(k) == 0 for k in (
                "p2p_typed_eager", "p2p_typed_staged", "p2p_typed_recv", "p2p_typed_lds", "p2p_typed_granule",
                "p2p_typed_walk64", "p2p_staged_sends", "p2p_direct_sends", "p2p_stage_bytes"))

        for args in bad:
            got, reqs = calls(args)
            assert got == (BAD,) * 4 and not any(reqs) and unmoved(), (got, reqs, args)
        assert lib.ompi_amd_isend_typed(h, d, 3, v, 0, 1, 9, None, ctypes.byref(ctypes.c_void_p())) == BAD
        assert lib.ompi_amd_isend_typed(h, d, 3, v, 0, 1, 4, None, None) == BAD
        # a message to self is waiting when the typed sends are refused as UNSUPPORTED: sendrecv_typed's
        # receive would match it, and must not have
        from ompi_amd import pml
        pml.send(comm, buf[:12], 0, 1)
        st, UNS = _lib.Status(), _lib.ERR_UNSUPPORTED
        for key, on, off, counts in (("p2p_user_ipc", 1, 0, (3, 2000)), ("p2p_stage_mib", 0, 1024, (2000,))):
            comm.set_param(key, on)
            for cnt in counts:  # (3: an eager size, 2000: a staged one)
                req, at = ctypes.c_void_p(0), d + 1024
                got = (lib.ompi_amd_isend_typed(h, at, cnt, v, 0, 1, 4, None, ctypes.byref(req)),
                       lib.ompi_amd_send_typed(h, at, cnt, v, 0, 1, 4, None),
                       lib.ompi_amd_sendrecv_typed(h, at, cnt, v, 0, 1, d, 3, v, 0, 1, None, ctypes.byref(st)))
                assert got == (UNS,) * 3 and not req.value and unmoved(), (key, cnt, got)
                assert pml.iprobe(comm, 0, 1).bytes == 12, "the waiting message was consumed"
            comm.set_param(key, off)
        assert pml.recv(comm, buf[:12], 0, 1).bytes == 12
        # nothing moves: the type is ignored, and the message is one of zero bytes
        assert lib.ompi_amd_sendrecv_typed(h, None, 0, neg, 0, 5, None, 0, neg, 0, 5, None, ctypes.byref(st)) == 0
        assert (st.source, st.tag, st.bytes) == (0, 5, 0) and comm.get_param("p2p_typed_recv") == 0
    finally:
        comm.free()
