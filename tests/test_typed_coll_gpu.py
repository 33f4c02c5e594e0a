"""The exchange collectives over derived datatypes on the device
(ompi_amd_<name>_typed: alltoall(v), allgatherv, gather(v), scatter(v)).

N ranks run tests/typed_worker.py, launched as tests/test_gather_gpu.py
launches its worker; N == 1 runs in this process.  Every rank computes its
expected buffers with oracle.pack / oracle.unpack and compares byte for byte.
"""
import ctypes
import json
import os
import secrets
import sys

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from test_coll_gpu import run_ranks  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "typed_worker.py")
CASES = {"shapes", "mixed", "inplace", "forms", "force64", "interleave", "layouts"}
NAMES = ("alltoall", "alltoallv", "allgatherv", "gather", "scatter", "gatherv", "scatterv")


@pytest.mark.parametrize("n", [2, 3, 4, 8])
def test_typed_ranks(n):
    outs = run_ranks(n, timeout=240, worker=WORKER, tag="typed")
    failures, granules, seconds = [], set(), {}
    for r, (rc, out) in enumerate(outs):
        lines = [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]
        for ln in lines:
            granules |= set(ln.get("granules", []))
            seconds[ln["case"]] = max(seconds.get(ln["case"], 0), ln["s"])
        bad = [ln for ln in lines if not ln["ok"]]
        missing = CASES - {ln["case"] for ln in lines}
        if rc != 0 or bad or missing:
            failures.append((r, rc, bad[:3], sorted(missing), out[-1500:] if rc not in (0, 1) or not lines else ""))
    assert not failures, failures
    print(f"typed worker N = {n}: seconds per case (slowest rank) {seconds}")
    # the generated calls of `layouts` took every granule on some rank
    assert granules == {1, 2, 4, 8, 16}, granules


def _comm(tag):
    from ompi_amd import coll
    return coll.Communicator(f"{tag}_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)


def test_typed_single_rank():
    """N == 1: one typed copy when one side has a datatype, pack and unpack
    through a scratch half when both have; the three forms of all seven."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import typed_worker as tw
    comm = _comm("typ1")
    try:
        T = tw.make_types()
        v12, c4, st, idx = (T[k][0] for k in ("v12", "c4", "struct", "idx"))
        for k, kind in enumerate(tw.KINDS):
            for a, b in ((v12, c4), (tw.BYTES, st), (st, st), (idx, idx)):
                x = tw.Call(comm, kind, a, b, n0=37, row=[41], seed=k)
                ok, msg = x.run()
                assert ok, (kind, msg)
                assert comm.get_param("typed_granule") == (1 if a is idx else 4), kind
                ok, msg = x.run("post")
                assert ok, ("i" + kind, msg)
                plan = x.init()
                assert plan.kind == 4
                for start in range(2):
                    x.refill(100 + start)
                    torch.cuda.synchronize()
                    plan.start()
                    plan.wait()
                    ok, msg = x.check()
                    assert ok, (kind + "_init", start, msg)
                plan.free()
        # in place: nothing moves
        x = tw.Call(comm, "alltoall", st, st, n0=5, seed=9, inplace=True)
        ok, msg = x.run()
        assert ok, msg
        assert comm.error() == 0
    finally:
        comm.free()


def test_typed_bad_params():
    """With a live communicator: every argument error of the header comment
    (a datatype with a negative extent on either side among them)
    returns BAD_PARAM from all three forms and no request or plan comes back;
    nothing reaches the device (comm.error() stays 0, no path counter moves);
    zero-element calls with NULL buffers are legal."""
    from ompi_amd import _lib
    from ompi_amd import datatype as dt
    comm = _comm("typbad")
    lib, h, BAD = comm._lib, comm._h, _lib.ERR_BAD_PARAM
    try:
        buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
        s, r = buf.data_ptr(), buf.data_ptr() + 128
        # the Datatype objects stay referenced: dropping one frees its device program
        V, W = dt.from_runs("v12", [(0, 4)], 12), dt.from_runs("w", [(0, 2), (4, 4)], 8)
        v, w = V.commit()._handle, W.commit()._handle   # sizes 4 and 6
        # v12's typemap with a negative extent: displacement * extent is a size_t, so it is refused
        NEG = dt.type_create_resized(V, 0, -12)
        neg = NEG.commit()._handle
        cnt, dsp = (ctypes.c_size_t * 1)(3), (ctypes.c_size_t * 1)(0)
        zero = (ctypes.c_size_t * 1)(0)
        none = ctypes.POINTER(ctypes.c_size_t)()
        bad = {
            # NULL buffers with data; packed bytes that differ: 3 * 4 != 3 * 6, 3 * 4 != 2 * 1
            "alltoall": [(None, r, 3, 3, v, v), (s, None, 3, 3, v, v), (s, r, 3, 3, v, w), (s, r, 3, 2, v, None)],
            "alltoallv": [(s, cnt, dsp, r, none, dsp, v, v), (s, cnt, dsp, r, cnt, none, v, v),
                          (s, none, dsp, r, cnt, dsp, v, v), (s, cnt, none, r, cnt, dsp, v, v),
                          (None, cnt, dsp, r, cnt, dsp, v, v), (s, cnt, dsp, None, cnt, dsp, v, v)],
            "allgatherv": [(None, 3, r, cnt, dsp, v, v), (s, 3, None, cnt, dsp, v, v), (s, 3, r, none, dsp, v, v),
                           (s, 3, r, cnt, none, v, v), (s, 2, r, cnt, dsp, v, v), (s, 3, r, cnt, dsp, v, w)],
            "gather": [(s, r, 3, 3, 1, v, v), (s, r, 3, 3, -1, v, v), (None, r, 3, 3, 0, v, v),
                       (s, None, 3, 3, 0, v, v), (s, r, 3, 3, 0, v, w), (s, r, 3, 4, 0, v, v)],
            "scatter": [(s, r, 3, 3, 1, v, v), (s, r, 3, 3, -1, v, v), (None, r, 3, 3, 0, v, v),
                        (s, None, 3, 3, 0, v, v), (s, r, 3, 3, 0, v, w), (s, r, 3, 4, 0, v, v)],
            "gatherv": [(s, 3, r, cnt, dsp, 1, v, v), (s, 3, r, cnt, dsp, -1, v, v), (None, 3, r, cnt, dsp, 0, v, v),
                        (s, 3, None, cnt, dsp, 0, v, v), (s, 3, r, none, dsp, 0, v, v),
                        (s, 3, r, cnt, none, 0, v, v), (s, 2, r, cnt, dsp, 0, v, v), (s, 3, r, cnt, dsp, 0, v, w)],
            "scatterv": [(s, cnt, dsp, r, 3, 1, v, v), (s, cnt, dsp, r, 3, -1, v, v),
                         (None, cnt, dsp, r, 3, 0, v, v), (s, cnt, dsp, None, 3, 0, v, v),
                         (s, none, dsp, r, 3, 0, v, v), (s, cnt, none, r, 3, 0, v, v),
                         (s, cnt, dsp, r, 2, 0, v, v), (s, cnt, dsp, r, 3, 0, v, w)],
        }
        good = {"alltoall": (s, r, 3, 3, v, v), "alltoallv": (s, cnt, dsp, r, cnt, dsp, v, v),
                "allgatherv": (s, 3, r, cnt, dsp, v, v), "gather": (s, r, 3, 3, 0, v, v),
                "scatter": (s, r, 3, 3, 0, v, v), "gatherv": (s, 3, r, cnt, dsp, 0, v, v),
                "scatterv": (s, cnt, dsp, r, 3, 0, v, v)}
        nothing = {"alltoall": (None, None, 0, 0, v, v), "alltoallv": (None, zero, dsp, None, zero, dsp, v, v),
                   "allgatherv": (None, 0, None, zero, dsp, v, v), "gather": (None, None, 0, 0, 0, v, v),
                   "scatter": (None, None, 0, 0, 0, v, v), "gatherv": (None, 0, None, zero, dsp, 0, v, v),
                   "scatterv": (None, zero, dsp, None, 0, 0, v, v)}
        for name in NAMES:
            bad[name] += [good[name][:-2] + (neg, v), good[name][:-2] + (v, neg), good[name][:-2] + (neg, neg)]
        for name in NAMES:
            f, fi, fp = (getattr(lib, f"ompi_amd_{x}") for x in
                         (name + "_typed", "i" + name + "_typed", name + "_typed_init"))
            for args in bad[name]:
                req, plan = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead)
                assert f(h, *args, None) == BAD, (name, args)
                assert fi(h, *args, None, ctypes.byref(req)) == BAD, (name, args)
                assert fp(h, *args, ctypes.byref(plan)) == BAD, (name, args)
                assert not req.value and not plan.value, (name, args)
            # a NULL communicator, a NULL request / plan pointer
            assert f(None, *good[name], None) == BAD, name
            assert fi(h, *good[name], None, None) == BAD, name
            assert fp(h, *good[name], None) == BAD, name
            assert comm.error() == 0
            # zero elements: NULL buffers are fine
            assert f(h, *nothing[name], None) == 0, name
            req = ctypes.c_void_p()
            assert fi(h, *nothing[name], None, ctypes.byref(req)) == 0 and req.value, name
            assert lib.ompi_amd_request_wait(req) == 0 and lib.ompi_amd_request_free(req) == 0
        assert all(comm.get_param(k) == 0 for k in ("typed_fused", "typed_staged", "typed_landing",
                                                    "typed_granule", "typed_walk64"))
        assert comm.error() == 0
    finally:
        comm.free()
