"""MPI_Allgatherv / MPI_Gather(v) / MPI_Scatter(v) on device buffers.

N ranks run tests/gather_worker.py, launched as tests/test_coll_gpu.py
launches its worker; N == 1 runs in this process.  Every rank computes its
expected buffers in closed form and compares byte for byte.
"""
import ctypes
import json
import os
import secrets

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "gather_worker.py")
CASES = {"sizes", "ragged", "inplace", "reuse", "nonblocking", "no_rendezvous", "persistent", "args"}
NAMES = ("allgatherv", "gather", "scatter", "gatherv", "scatterv")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_gather_ranks(n):
    outs = run_ranks(n, timeout=240, worker=WORKER, tag="gather")
    failures = []
    for r, (rc, out) in enumerate(outs):
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        bad = [ln for ln in lines if not ln["ok"]]
        missing = CASES - {ln["case"] for ln in lines}
        if rc != 0 or bad or missing:
            failures.append((r, rc, bad[:3], sorted(missing), out[-1500:] if rc not in (0, 1) or not lines else ""))
    assert not failures, failures


def _comm(tag):
    from ompi_amd import coll
    return coll.Communicator(f"{tag}_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)


def test_gather_single_rank():
    """N == 1: one local copy of the rank's block; in place nothing moves."""
    from ompi_amd import coll
    comm = _comm("gth1")
    try:
        src = torch.arange(1003, dtype=torch.int32, device="cuda").to(torch.uint8)
        want = src.cpu().numpy()
        dst = torch.empty(1003 + 128, dtype=torch.uint8, device="cuda")

        def landed(at, lo, n):
            got = dst.cpu().numpy()
            keep = np.ones(got.size, dtype=bool)
            keep[at:at + n] = False
            return np.array_equal(got[at:at + n], want[lo:lo + n]) and (got[keep] == 0xA5).all()

        forms = {
            "allgatherv": lambda f: f(src, 700, dst, [700], [9]),
            "gather": lambda f: f(src, dst.data_ptr() + 9, 700, 0),
            "gatherv": lambda f: f(src, 700, dst, [700], [9], 0),
            "scatter": lambda f: f(src.data_ptr() + 5, dst.data_ptr() + 9, 700, 0),
            "scatterv": lambda f: f(src, [700], [5], dst.data_ptr() + 9, 700, 0),
        }
        for name, call in forms.items():
            lo = 5 if name.startswith("scatter") else 0
            dst.fill_(0xA5)
            call(lambda *a: getattr(comm, name)(*a, blocking=True))
            assert landed(9, lo, 700), name
            dst.fill_(0xA5)
            req = call(getattr(comm, "i" + name))
            req.wait()
            req.free()
            assert landed(9, lo, 700), "i" + name
            dst.fill_(0xA5)
            plan = call(getattr(comm, name + "_init"))
            assert plan.kind == 4
            plan.start()
            plan.wait()
            plan.free()
            assert landed(9, lo, 700), name + "_init"
        # in place: nothing moves
        dst.fill_(0x33)
        keep = dst.clone()
        comm.allgatherv(coll.IN_PLACE, 0, dst, [700], [9], blocking=True)
        comm.allgatherv(dst.data_ptr() + 9, 700, dst, [700], [9], blocking=True)
        comm.gather(coll.IN_PLACE, dst, 700, 0, blocking=True)
        comm.gatherv(coll.IN_PLACE, 0, dst, [700], [9], 0, blocking=True)
        comm.scatter(dst, coll.IN_PLACE, 700, 0, blocking=True)
        comm.scatterv(dst, [700], [9], coll.IN_PLACE, 0, 0, blocking=True)
        assert torch.equal(dst, keep)
    finally:
        comm.free()


def test_gather_bad_params():
    """With a live communicator: every argument error of the header comment
    returns BAD_PARAM from all three forms and no request or plan comes back;
    zero-byte calls with NULL buffers are legal."""
    from ompi_amd import _lib
    comm = _comm("gthbad")
    lib, h, BAD = comm._lib, comm._h, _lib.ERR_BAD_PARAM
    try:
        buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
        s, r = buf.data_ptr(), buf.data_ptr() + 32
        cnt, dsp = (ctypes.c_size_t * 1)(8), (ctypes.c_size_t * 1)(0)
        zero = (ctypes.c_size_t * 1)(0)
        none = ctypes.POINTER(ctypes.c_size_t)()
        bad = {
            "allgatherv": [(None, 8, r, cnt, dsp), (s, 8, None, cnt, dsp), (s, 8, r, none, dsp),
                           (s, 8, r, cnt, none), (s, 7, r, cnt, dsp)],
            "gather": [(s, r, 8, 1), (s, r, 8, -1), (None, r, 8, 0), (s, None, 8, 0)],
            "scatter": [(s, r, 8, 1), (s, r, 8, -1), (None, r, 8, 0), (s, None, 8, 0)],
            "gatherv": [(s, 8, r, cnt, dsp, 1), (s, 8, r, cnt, dsp, -1), (None, 8, r, cnt, dsp, 0),
                        (s, 8, None, cnt, dsp, 0), (s, 8, r, none, dsp, 0), (s, 8, r, cnt, none, 0),
                        (s, 7, r, cnt, dsp, 0)],
            "scatterv": [(s, cnt, dsp, r, 8, 1), (s, cnt, dsp, r, 8, -1), (None, cnt, dsp, r, 8, 0),
                         (s, cnt, dsp, None, 8, 0), (s, none, dsp, r, 8, 0), (s, cnt, none, r, 8, 0),
                         (s, cnt, dsp, r, 7, 0)],
        }
        good = {"allgatherv": (s, 8, r, cnt, dsp), "gather": (s, r, 8, 0), "scatter": (s, r, 8, 0),
                "gatherv": (s, 8, r, cnt, dsp, 0), "scatterv": (s, cnt, dsp, r, 8, 0)}
        nothing = {"allgatherv": (None, 0, None, zero, dsp), "gather": (None, None, 0, 0),
                   "scatter": (None, None, 0, 0), "gatherv": (None, 0, None, zero, dsp, 0),
                   "scatterv": (None, zero, dsp, None, 0, 0)}
        for name in NAMES:
            f, fi, fp = (getattr(lib, f"ompi_amd_{x}") for x in (name, "i" + name, name + "_init"))
            for args in bad[name]:
                req, plan = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead)
                assert f(h, *args, None) == BAD, (name, args)
                assert fi(h, *args, None, ctypes.byref(req)) == BAD, (name, args)
                assert fp(h, *args, ctypes.byref(plan)) == BAD, (name, args)
                assert not req.value and not plan.value, (name, args)
            # a NULL request / plan pointer
            assert fi(h, *good[name], None, None) == BAD, name
            assert fp(h, *good[name], None) == BAD, name
            assert comm.error() == 0
            # zero bytes: NULL buffers are fine
            assert f(h, *nothing[name], None) == 0, name
            req = ctypes.c_void_p()
            assert fi(h, *nothing[name], None, ctypes.byref(req)) == 0 and req.value, name
            assert lib.ompi_amd_request_wait(req) == 0 and lib.ompi_amd_request_free(req) == 0
        assert all(comm.get_param(k) == 0 for k in ("gather_fused", "gather_staged", "gather_landing"))
    finally:
        comm.free()
