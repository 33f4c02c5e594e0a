"""The alltoall surface without a GPU: the symbols, their prototypes, the
NULL-communicator check and the Python methods."""
import ctypes
import os
import re

import pytest

from ompi_amd import _lib, coll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ompi_amd_alltoall", "ompi_amd_alltoallv", "ompi_amd_ialltoall", "ompi_amd_ialltoallv",
           "ompi_amd_alltoall_init", "ompi_amd_alltoallv_init"]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_declared_and_prototyped(lib, name):
    assert getattr(lib, name, None) is not None, f"{name} not exported by libompi_amd.so"
    header = open(os.path.join(ROOT, "include", "ompi_amd_coll.h")).read()
    assert re.search(rf"\bint {name}\(", header), f"{name} not declared in ompi_amd_coll.h"
    assert name in {p[0] for p in _lib.PROTOTYPES}, f"{name} missing from _lib.PROTOTYPES"


def test_bad_params_without_a_device(lib):
    """A NULL comm is refused by all six entry points before any device call,
    whatever else is passed.  The other two argument errors (NULL rbuf with
    bytes > 0, NULL count arrays) need a communicator and so a device:
    tests/test_alltoall_gpu.py::test_alltoall_bad_params."""
    BAD = _lib.ERR_BAD_PARAM
    req, plan = ctypes.c_void_p(), ctypes.c_void_p()
    counts = (ctypes.c_size_t * 2)(8, 8)
    displs = (ctypes.c_size_t * 2)(0, 8)
    none = ctypes.POINTER(ctypes.c_size_t)()
    buf = ctypes.create_string_buffer(64)
    s, r = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    assert lib.ompi_amd_alltoall(None, s, r, 8, None) == BAD
    assert lib.ompi_amd_alltoallv(None, s, counts, displs, r, counts, displs, None) == BAD
    assert lib.ompi_amd_alltoallv(None, s, none, none, r, none, none, None) == BAD
    assert lib.ompi_amd_ialltoall(None, s, r, 8, None, ctypes.byref(req)) == BAD
    assert lib.ompi_amd_ialltoallv(None, s, counts, displs, r, counts, displs, None,
                                   ctypes.byref(req)) == BAD
    assert lib.ompi_amd_alltoall_init(None, s, r, 8, ctypes.byref(plan)) == BAD
    assert lib.ompi_amd_alltoallv_init(None, s, counts, displs, r, counts, displs,
                                       ctypes.byref(plan)) == BAD
    assert not req.value and not plan.value


def test_communicator_methods():
    for m in ("alltoall", "alltoallv", "ialltoall", "ialltoallv", "alltoall_init", "alltoallv_init"):
        assert callable(getattr(coll.Communicator, m, None)), m
