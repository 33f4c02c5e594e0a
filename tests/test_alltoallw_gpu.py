"""MPI_Alltoallw on the device (ompi_amd_alltoallw): one datatype per peer on
either side.  N ranks run tests/alltoallw_worker.py on one forced path; every rank compares its
buffers byte for byte with a numpy gather / scatter."""
import ctypes
import os
import secrets

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402

WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "alltoallw_worker.py")
PATHS = ("fused", "staged", "landing")


@pytest.mark.parametrize("n,path", [(1, "local")] + [(n, p) for n in (2, 3) for p in PATHS])
def test_alltoallw(n, path):
    """Per-peer datatypes (4-B vector, 16-B struct, 1-B indexed that bisects,
    bytes, one empty pair), byte displacements off every extent, in the
    blocking, nonblocking and persistent forms, in place, with programs past
    the LDS budget, and on the landing path in five passes."""
    env = {"A2AW_PATH": str(PATHS.index(path))} if n > 1 else {}
    res = run_ranks(n, timeout=120, extra_env=env, worker=WORKER, tag=f"a2aw_{path}")
    assert not any(rc for rc, _ in res), [(r, rc, out[-1500:]) for r, (rc, out) in enumerate(res) if rc]


def test_alltoallw_bad_params():
    """Every refusal of the header comment returns BAD_PARAM from all three
    forms with no request or plan; nothing reaches the device and no counter
    moves; a pair of count 0 ignores its datatype and displacement."""
    from ompi_amd import _lib, coll, datatype as dt
    comm = coll.Communicator(f"a2awbad_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)
    lib, h, BAD = comm._lib, comm._h, _lib.ERR_BAD_PARAM
    try:
        buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
        V, W = dt.from_runs("v12", [(0, 4)], 12), dt.from_runs("w", [(0, 2), (4, 4)], 8)  # sizes 4 and 6
        NEG = dt.type_create_resized(V, 0, -12)
        v, w, neg = ((ctypes.c_void_p * 1)(t.commit()._handle) for t in (V, W, NEG))
        cnt, dsp, zero, huge = ((ctypes.c_size_t * 1)(x) for x in (3, 0, 0, 1 << 62))  # huge * 4 > SIZE_MAX
        none, notypes = ctypes.POINTER(ctypes.c_size_t)(), ctypes.POINTER(ctypes.c_void_p)()
        # sbuf, scounts, sdispls, sddts, rbuf, rcounts, rdispls, rddts
        good = (buf.data_ptr(), cnt, dsp, v, buf.data_ptr() + 128, cnt, dsp, v)
        swap = lambda *at: tuple(dict(at).get(i, a) for i, a in enumerate(good))  # noqa: E731
        # one argument wrong: NULL (as alltoallv_typed), 3 * 4 != 3 * 6 on the own pair, a negative extent
        bad = [swap((i, x)) for i, x in ((0, None), (1, none), (2, none), (3, notypes), (4, None), (5, none),
                                         (6, none), (7, notypes), (7, w), (3, neg), (7, neg))]
        bad += [swap((0, 1), (3, notypes), (7, notypes)),  # in place still needs the receive datatypes
                swap((1, huge), (5, huge)),
                swap((0, None), (4, None), (1, zero), (5, zero), (2, none), (6, none))]  # empty, yet no displs
        f, fi, fp = (getattr(lib, f"ompi_amd_{x}") for x in ("alltoallw", "ialltoallw", "alltoallw_init"))
        for args in bad:
            req, plan = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead)
            got = f(h, *args, None), fi(h, *args, None, ctypes.byref(req)), fp(h, *args, ctypes.byref(plan))
            assert got == (BAD, BAD, BAD) and not req.value and not plan.value, (got, args)
        assert f(None, *good, None) == fi(h, *good, None, None) == fp(h, *good, None) == BAD
        assert comm.error() == 0 and all(comm.get_param(k) == 0 for k in (
            "alltoallw_calls", "alltoallw_lds_programs", "typed_fused", "typed_staged", "typed_landing",
            "typed_granule", "typed_walk64", "alltoall_fused", "alltoall_staged", "alltoall_landing"))
        # nothing moves: the types are ignored
        assert f(h, None, zero, dsp, neg, None, zero, dsp, neg, None) == 0 and comm.error() == 0
    finally:
        comm.free()
