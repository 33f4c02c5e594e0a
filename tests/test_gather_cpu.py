"""The allgatherv / gather(v) / scatter(v) surface without a GPU: the
fifteen symbols, their prototypes, the NULL-communicator check and the Python
methods."""
import ctypes
import os
import re

import pytest

from ompi_amd import _lib, coll

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["allgatherv", "gather", "gatherv", "scatter", "scatterv"]
FORMS = [("", ""), ("i", ""), ("", "_init")]
SYMBOLS = [f"ompi_amd_{pre}{n}{post}" for n in NAMES for pre, post in FORMS]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_fifteen():
    assert len(set(SYMBOLS)) == 15


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_exported_declared_and_prototyped(lib, name):
    assert getattr(lib, name, None) is not None, f"{name} not exported by libompi_amd.so"
    header = open(os.path.join(ROOT, "include", "ompi_amd_coll.h")).read()
    assert re.search(rf"\bint {name}\(", header), f"{name} not declared in ompi_amd_coll.h"
    assert name in {p[0] for p in _lib.PROTOTYPES}, f"{name} missing from _lib.PROTOTYPES"


@pytest.mark.parametrize("name", NAMES)
def test_null_communicator_is_refused(lib, name):
    """A NULL comm is refused by all three forms before any device call, and
    no request or plan comes back (the out pointers start non-NULL here).  The
    other argument errors need a communicator: tests/test_gather_gpu.py, case
    `args`."""
    counts = (ctypes.c_size_t * 2)(8, 8)
    displs = (ctypes.c_size_t * 2)(0, 8)
    buf = ctypes.create_string_buffer(64)
    s, r = ctypes.addressof(buf), ctypes.addressof(buf) + 32
    ops = {"allgatherv": (s, 8, r, counts, displs), "gather": (s, r, 8, 0), "scatter": (s, r, 8, 0),
           "gatherv": (s, 8, r, counts, displs, 0), "scatterv": (s, counts, displs, r, 8, 0)}[name]
    req, plan = ctypes.c_void_p(0xdead), ctypes.c_void_p(0xdead)
    assert getattr(lib, f"ompi_amd_{name}")(None, *ops, None) == _lib.ERR_BAD_PARAM
    assert getattr(lib, f"ompi_amd_i{name}")(None, *ops, None, ctypes.byref(req)) == _lib.ERR_BAD_PARAM
    assert getattr(lib, f"ompi_amd_{name}_init")(None, *ops, ctypes.byref(plan)) == _lib.ERR_BAD_PARAM
    assert not req.value and not plan.value
    # a NULL request / plan pointer is refused too
    assert getattr(lib, f"ompi_amd_i{name}")(None, *ops, None, None) == _lib.ERR_BAD_PARAM
    assert getattr(lib, f"ompi_amd_{name}_init")(None, *ops, None) == _lib.ERR_BAD_PARAM


@pytest.mark.parametrize("name", NAMES)
def test_communicator_methods(name):
    for pre, post in FORMS:
        assert callable(getattr(coll.Communicator, pre + name + post, None)), pre + name + post
