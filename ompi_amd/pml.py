"""Point-to-point messages between device buffers (the PML surface for
device memory).

Mirrors the PML module entry points (ompi/mca/pml/pml.h):

    pml_isend(buf, count, dtype, dst, tag, mode, comm, request)   pml.h:317-326
    pml_irecv(buf, count, dtype, src, tag, comm, request)         pml.h:233-241
    pml_send / pml_recv                                           pml.h:341-349, 262-270
    pml_iprobe / pml_probe                                        pml.h:371-377, 398-403

with the message size in bytes, or, in the ``*_typed`` forms, a count of
elements of an ``ompi_amd.datatype.Datatype`` that the kernels moving the
message walk themselves (no packed copy; device buffers only).  The receiver
pulls the sender's buffer over xGMI through its IPC mapping
(include/ompi_amd_p2p.h); there is no host fallback for device buffers.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

from . import _lib
from .coll import Communicator, _ptr, _stream

ANY_SOURCE = -1   # MPI_ANY_SOURCE
ANY_TAG = -1      # MPI_ANY_TAG

# mca_pml_base_send_mode_t (ompi/mca/pml/pml_constants.h:30-37)
SEND_SYNCHRONOUS, SEND_COMPLETE, SEND_BUFFERED, SEND_READY, SEND_STANDARD = range(5)


@dataclass
class Status:
    """MPI_Status of a receive / probe: MPI_SOURCE, MPI_TAG, MPI_ERROR and
    the message size in bytes (MPI_Get_count's numerator)."""
    source: int
    tag: int
    error: int
    bytes: int


def _status(st: _lib.Status) -> Status:
    return Status(st.source, st.tag, st.error, st.bytes)


def _nbytes(buf, nbytes):
    if nbytes is not None:
        return int(nbytes)
    return buf.numel() * buf.element_size()


class P2PRequest:
    """MPI_Request of an isend / irecv."""

    def __init__(self, comm: Communicator, handle, what: str, ddt=None):
        self._comm, self._h, self._what = comm, handle, what
        self._ddt = ddt  # a typed request keeps its datatype's program alive
        self.status: Status | None = None

    def test(self) -> bool:
        done, st = ctypes.c_int(), _lib.Status()
        _lib.check(self._comm._lib.ompi_amd_p2p_test(self._h, ctypes.byref(done),
                                                     ctypes.byref(st)), "test " + self._what)
        if done.value:
            self.status = _status(st)
        return bool(done.value)

    def wait(self) -> Status:
        st = _lib.Status()
        rc = self._comm._lib.ompi_amd_p2p_wait(self._h, ctypes.byref(st))
        self.status = _status(st)
        _lib.check(rc, "wait " + self._what)
        return self.status

    def free(self) -> None:
        if self._h:
            h, self._h = self._h, None
            _lib.check(self._comm._lib.ompi_amd_p2p_free(h), "free " + self._what)


def isend(comm: Communicator, buf, dst: int, tag: int, nbytes: int | None = None,
          mode: int = SEND_STANDARD, stream=None) -> P2PRequest:
    h = ctypes.c_void_p()
    _lib.check(comm._lib.ompi_amd_isend(comm._h, _ptr(buf), _nbytes(buf, nbytes), dst, tag, mode,
                                        _stream(stream), ctypes.byref(h)), "isend")
    return P2PRequest(comm, h, f"isend(to {dst}, tag {tag})")


def irecv(comm: Communicator, buf, src: int = ANY_SOURCE, tag: int = ANY_TAG,
          nbytes: int | None = None, stream=None) -> P2PRequest:
    h = ctypes.c_void_p()
    _lib.check(comm._lib.ompi_amd_irecv(comm._h, _ptr(buf), _nbytes(buf, nbytes), src, tag,
                                        _stream(stream), ctypes.byref(h)), "irecv")
    return P2PRequest(comm, h, f"irecv(from {src}, tag {tag})")


def send(comm: Communicator, buf, dst: int, tag: int, nbytes: int | None = None,
         mode: int = SEND_STANDARD, stream=None) -> None:
    _lib.check(comm._lib.ompi_amd_send(comm._h, _ptr(buf), _nbytes(buf, nbytes), dst, tag, mode,
                                       _stream(stream)), "send")


def recv(comm: Communicator, buf, src: int = ANY_SOURCE, tag: int = ANY_TAG,
         nbytes: int | None = None, stream=None) -> Status:
    st = _lib.Status()
    _lib.check(comm._lib.ompi_amd_recv(comm._h, _ptr(buf), _nbytes(buf, nbytes), src, tag,
                                       _stream(stream), ctypes.byref(st)), "recv")
    return _status(st)


def sendrecv(comm: Communicator, sbuf, dst: int, stag: int, rbuf, src: int, rtag: int,
             sbytes: int | None = None, rbytes: int | None = None, stream=None) -> Status:
    st = _lib.Status()
    _lib.check(comm._lib.ompi_amd_sendrecv(comm._h, _ptr(sbuf), _nbytes(sbuf, sbytes), dst, stag,
                                           _ptr(rbuf), _nbytes(rbuf, rbytes), src, rtag,
                                           _stream(stream), ctypes.byref(st)), "sendrecv")
    return _status(st)


def _ddt(t):
    return None if t is None else t.commit()._handle


def isend_typed(comm: Communicator, buf, count: int, ddt, dst: int, tag: int,
                mode: int = SEND_STANDARD, stream=None) -> P2PRequest:
    """isend of `count` elements of `ddt` (None: bytes) based at `buf`."""
    h = ctypes.c_void_p()
    _lib.check(comm._lib.ompi_amd_isend_typed(comm._h, _ptr(buf), count, _ddt(ddt), dst, tag, mode,
                                              _stream(stream), ctypes.byref(h)), "isend_typed")
    return P2PRequest(comm, h, f"isend_typed(to {dst}, tag {tag})", ddt)


def irecv_typed(comm: Communicator, buf, count: int, ddt, src: int = ANY_SOURCE, tag: int = ANY_TAG,
                stream=None) -> P2PRequest:
    h = ctypes.c_void_p()
    _lib.check(comm._lib.ompi_amd_irecv_typed(comm._h, _ptr(buf), count, _ddt(ddt), src, tag,
                                              _stream(stream), ctypes.byref(h)), "irecv_typed")
    return P2PRequest(comm, h, f"irecv_typed(from {src}, tag {tag})", ddt)


def send_typed(comm: Communicator, buf, count: int, ddt, dst: int, tag: int,
               mode: int = SEND_STANDARD, stream=None) -> None:
    _lib.check(comm._lib.ompi_amd_send_typed(comm._h, _ptr(buf), count, _ddt(ddt), dst, tag, mode,
                                             _stream(stream)), "send_typed")


def recv_typed(comm: Communicator, buf, count: int, ddt, src: int = ANY_SOURCE, tag: int = ANY_TAG,
               stream=None) -> Status:
    st = _lib.Status()
    _lib.check(comm._lib.ompi_amd_recv_typed(comm._h, _ptr(buf), count, _ddt(ddt), src, tag,
                                             _stream(stream), ctypes.byref(st)), "recv_typed")
    return _status(st)


def sendrecv_typed(comm: Communicator, sbuf, scount: int, sddt, dst: int, stag: int, rbuf, rcount: int,
                   rddt, src: int, rtag: int, stream=None) -> Status:
    st = _lib.Status()
    _lib.check(comm._lib.ompi_amd_sendrecv_typed(comm._h, _ptr(sbuf), scount, _ddt(sddt), dst, stag,
                                                 _ptr(rbuf), rcount, _ddt(rddt), src, rtag,
                                                 _stream(stream), ctypes.byref(st)), "sendrecv_typed")
    return _status(st)


def iprobe(comm: Communicator, src: int = ANY_SOURCE, tag: int = ANY_TAG) -> Status | None:
    flag, st = ctypes.c_int(), _lib.Status()
    _lib.check(comm._lib.ompi_amd_iprobe(comm._h, src, tag, ctypes.byref(flag), ctypes.byref(st)),
               "iprobe")
    return _status(st) if flag.value else None


def probe(comm: Communicator, src: int = ANY_SOURCE, tag: int = ANY_TAG) -> Status:
    st = _lib.Status()
    _lib.check(comm._lib.ompi_amd_probe(comm._h, src, tag, ctypes.byref(st)), "probe")
    return _status(st)
