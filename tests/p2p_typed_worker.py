"""One rank of tests/test_p2p_typed_gpu.py.  Every rank sends to rank + 1 and receives from
rank - 1 (itself at N = 1).  The reference is numpy: pack gathers the runs of Datatype.runs per
element at multiples of the extent, unpack scatters into a buffer pre-filled with a sentinel,
and whole buffers are compared."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gather_worker import Buf, PREFILL  # noqa: E402
from ompi_amd import _lib, coll, datatype as dt, pml  # noqa: E402

COUNTERS = ("p2p_typed_eager", "p2p_typed_staged", "p2p_typed_recv", "p2p_typed_lds", "p2p_typed_walk64")


def offs(t, count):
    """Byte offsets, in packed order, of `count` elements of t (None: bytes)."""
    runs, extent = (t.runs, t.extent) if t else ([(0, 1)], 1)
    one = np.concatenate([np.arange(d, d + ln) for d, ln in runs])
    return (np.arange(count)[:, None] * extent + one).ravel()


def span(t, count):
    return count * t.extent + max(t.true_span, t.extent) if t else count


def image(rank, seed, nbytes):
    return np.random.default_rng([seed, rank, 0x7E]).integers(0, 256, nbytes, dtype=np.uint8)


def types():
    INT = dt.predefined("MPI_INT")
    lens = [1, 3, 2, 4]
    big = [1, 2] * 120 + [1, 3] * 30  # 300 elements, past the 256 the kernels stage in LDS
    runs = lambda ls: [(sum(ls[:i]) + i, ln) for i, ln in enumerate(ls)]  # noqa: E731
    s12 = dt.from_runs("s12", [(0, 4), (8, 8)], 16)
    T = dict(v4=dt.from_runs("v4", [(4, 4)], 12), v16=dt.type_vector(4, 4, 8, INT),     # sizes 4, 64
             s16=dt.from_runs("s16", [(0, 4), (8, 8), (20, 4)], 24),                    # size 16, G 4
             idx=dt.from_runs("idx", runs(lens), sum(lens) + len(lens) + 3),            # size 10, G 1
             v2=dt.type_vector(5, 1, 3, dt.predefined("MPI_SHORT")),                    # size 10, G 2
             v8=dt.type_vector(5, 2, 6, INT), w16=dt.type_vector(2, 4, 12, INT),        # sizes 40, 32
             s12=s12, s24=dt.type_contiguous(2, s12),                                   # two s12 per element
             big=dt.from_runs("big", runs(big), sum(big) + len(big) + 3),               # size 480
             v64=dt.type_vector(4, 1, 2, INT))                                          # size 16
    assert T["big"].nelems > 256 and T["s24"].size == 24
    return T


# name: send (type, count), receive (type, count), the receive buffer's offset from 256 B,
# the granules of the send and the receive launch, options
def cases(T):
    return [
        ("one_lane", ("v4", 1), ("v4", 1), 0, 4, 4, {}),
        ("eager_limit", ("v16", 64), ("s16", 256), 0, 16, 4, {}),                # 4096 B, one signature
        ("first_staged", ("idx", 410), (None, 4100), 0, 1, None, {}),            # 4100 B into bytes
        ("byte_send", (None, 4100), ("v2", 410), 0, None, 2, {"any": True}),
        # 1 MiB + 24: 33 workgroups; the receive base is 8 mod 16 and the stream ends 8 B into a 16-B run
        ("many_groups", ("v8", 26215), ("w16", 32769), 8, 8, 8, {}),
        # 65532 B end inside an s24, 8 B into its 12-B run [8, 20) (the two structs' runs that touch)
        ("partial", ("s12", 5461), ("s24", 4096), 0, 4, 4, {}),
        ("global_walk", ("big", 17), ("big", 17), 0, 1, 1, {"two": True}),      # 8160 B, twice, one tag
        ("force64", ("v64", 512), ("v64", 512), 0, 4, 4, {"force64": True}),     # 8 KiB
        ("truncate", ("v64", 512), ("v64", 500), 0, 4, 4, {"truncate": True}),
    ]


def run(comm, T, seed, case):
    name, (st, sc), (rt, rc), roff, gs, gr, opt = case
    st, rt = T.get(st), T.get(rt)
    n, me = comm.size, comm.rank
    to, frm = (me + 1) % n, (me - 1) % n
    k = 2 if opt.get("two") else 1
    comm.set_param("typed_force64", int(bool(opt.get("force64"))))
    sbytes = sc * (st.size if st else 1)
    sbufs = [Buf(image(me, seed + i, span(st, sc)), 0) for i in range(k)]
    rbufs = [Buf(np.full(span(rt, rc), PREFILL, np.uint8), roff) for i in range(k)]
    for i, rb in enumerate(rbufs):  # what the receive must leave: the first bytes of the sender's stream
        stream = image(frm, seed + i, span(st, sc))[offs(st, sc)]
        want = np.full(rb.n, PREFILL, np.uint8)
        at = offs(rt, rc)[:stream.size]
        want[at] = stream[:at.size]
        rb.expect(want)
    torch.cuda.synchronize()
    before = [comm.get_param(c) for c in COUNTERS]
    # (one tag for every message of a case: only the order tells two of them apart)
    sreq = [pml.isend_typed(comm, b.ptr, sc, st, to, 40) if st else pml.isend(comm, b.ptr, to, 40, sc)
            for b in sbufs]
    assert st is None or comm.get_param("p2p_typed_granule") == gs, (name, "send granule")
    src, tag = (pml.ANY_SOURCE, pml.ANY_TAG) if opt.get("any") else (frm, None)
    rreq = [pml.irecv_typed(comm, b.ptr, rc, rt, src, 40 if tag is None else tag) if rt
            else pml.irecv(comm, b.ptr, src, 40, rc) for b in rbufs]
    for r in rreq:
        try:
            status = r.wait()
            assert not opt.get("truncate"), "a longer message must not pass"
        except _lib.OmpiAmdError as e:
            assert opt.get("truncate") and e.code == _lib.ERR_TRUNCATE, e
            status = r.status
        assert (status.source, status.tag, status.bytes) == (frm, 40, sbytes), (name, status)
        r.free()
    for r in sreq:
        r.wait()
        r.free()
    assert not comm.error(), f"device error {comm.error()}"
    for b, what in [(b, "rbuf") for b in rbufs] + [(b, "sbuf") for b in sbufs]:
        ok, msg = b.check(what)
        assert ok, (name, msg)
    eager = sbytes <= 4096
    want = [k * int(bool(st) and eager), k * int(bool(st) and not eager), k * int(bool(rt)),
            k * int(bool(rt) and rt.nelems <= 256), (bool(st) + bool(rt)) * int(bool(opt.get("force64")))]
    moved = [comm.get_param(c) - b for c, b in zip(COUNTERS, before)]
    assert moved == want, f"{name}: counters {COUNTERS} moved by {moved}, expected {want}"
    assert rt is None or comm.get_param("p2p_typed_granule") == gr, (name, "receive granule")


def main():
    rank, n, device = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "OMPI_AMD_DEVICE"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lost signal is an error line, not a kill
    T = types()
    for seed, case in enumerate(cases(T)):  # a failed assertion ends the rank: exit status 1
        print(f"rank {rank}: case {case[0]}", flush=True)
        run(comm, T, 10 * seed, case)
    comm.free()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
