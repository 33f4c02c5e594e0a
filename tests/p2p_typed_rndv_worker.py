"""One rank of tests/test_p2p_typed_rndv_gpu.py, under the trigger named in OMPI_AMD_RNDV_TRIGGER.  Every rank
sends to rank + 1 and receives from rank - 1; reference and buffers are tests/p2p_typed_worker.py's."""
import os

import numpy as np

from p2p_typed_worker import PREFILL, Buf, _lib, coll, dist, image, offs, pml, span, torch, types

COUNTERS = ("p2p_typed_rndv", "p2p_typed_sndrcv", "p2p_typed_staged", "p2p_typed_eager", "p2p_typed_recv")
TRIGGERS = {"user_ipc": ("p2p_user_ipc", 1), "no_stage": ("p2p_stage_mib", 0)}


class SendBuf(Buf):
    def __init__(self, host, off):  # in an allocation peers can map: >= 4 MiB, cut from a 20 MiB segment (§4.6)
        self.n, self.t = host.size, torch.empty(max(host.size + 1024, 4 << 20), dtype=torch.uint8, device="cuda")
        self.lo = (-self.t.data_ptr()) % 256 + 256 + off
        self.ptr = self.t.data_ptr() + self.lo
        self.set(host)


# name: send, receive (type, count), receive base offset, COUNTERS moved under (user_ipc, no_stage; None: UNSUPPORTED)
R = (1, 1, 0, 0, 1)  # a typed rendezvous into a typed receive
CASES = [
    ("small", ("v64", 512), ("v4", 2048), 0, (R, R), {}),                                   # 8 KiB
    ("many_groups", ("v8", 26215), ("w16", 32769), 8, (R, R), {}),                          # 1 MiB + 24
    ("to_bytes", ("idx", 410), (None, 4100), 0, ((1, 0, 0, 0, 0),) * 2, {}),
    ("from_bytes", (None, 4100), ("v2", 410), 0, ((0, 0, 0, 0, 1),) * 2, {"any": True}),    # a byte rendezvous
    ("partial", ("s12", 5461), ("s24", 4096), 0, (R, R), {}),                               # 65532 B
    ("long_program", ("big", 17), ("big", 17), 0, ((0, 0, 1, 0, 1), None), {}),             # 300 > 39 elements
    ("eager", ("v16", 64), ("s16", 256), 0, ((0, 0, 0, 1, 1),) * 2, {}),                    # 4096 B
    ("ssend", ("v64", 512), ("v4", 2048), 0, (R, R), {"mode": pml.SEND_SYNCHRONOUS}),
    ("sendrecv", ("v64", 512), ("v4", 2048), 0, (R, R), {"sendrecv": True}),
    ("truncate", ("v64", 512), ("v4", 2000), 0, (R, R), {"truncate": True}),
]


def run(comm, T, seed, case, which):
    name, (st, sc), (rt, rc), roff, moves, opt = case
    st, rt, want_moved, me = T.get(st), T.get(rt), moves[which], comm.rank
    to, frm = (me + 1) % comm.size, (me - 1) % comm.size
    sbytes = sc * (st.size if st else 1)
    sbuf, rbuf = SendBuf(image(me, seed, span(st, sc)), 0), Buf(np.full(span(rt, rc), PREFILL, np.uint8), roff)
    stream, want = image(frm, seed, span(st, sc))[offs(st, sc)], np.full(rbuf.n, PREFILL, np.uint8)
    at = offs(rt, rc)[:stream.size]
    want[at] = stream[:at.size]
    torch.cuda.synchronize()
    before = [comm.get_param(c) for c in COUNTERS]
    try:
        if opt.get("sendrecv"):
            status = pml.sendrecv_typed(comm, sbuf.ptr, sc, st, to, 40, rbuf.ptr, rc, rt, pml.ANY_SOURCE, pml.ANY_TAG)
        else:
            sreq = (pml.isend_typed(comm, sbuf.ptr, sc, st, to, 40, opt.get("mode", pml.SEND_STANDARD)) if st
                    else pml.isend(comm, sbuf.ptr, to, 40, sc))
            src, tag = (pml.ANY_SOURCE, pml.ANY_TAG) if opt.get("any") else (frm, 40)
            rreq = pml.irecv_typed(comm, rbuf.ptr, rc, rt, src, tag) if rt else pml.irecv(comm, rbuf.ptr, src, tag, rc)
            try:
                status = rreq.wait()
                assert not opt.get("truncate"), "a longer message must not pass"
            except _lib.OmpiAmdError as e:
                assert opt.get("truncate") and e.code == _lib.ERR_TRUNCATE, e
                status = rreq.status
            rreq.free()
            sreq.wait()
            sreq.free()
        assert want_moved and (status.source, status.tag, status.bytes) == (frm, 40, sbytes), (name, status)
        rbuf.expect(want)
    except _lib.OmpiAmdError as e:  # refused: no request, nothing received, no counter moved
        assert want_moved is None and e.code == _lib.ERR_UNSUPPORTED, (name, e)
        want_moved = (0,) * len(COUNTERS)
    assert not comm.error(), f"device error {comm.error()}"
    for ok, msg in (rbuf.check("rbuf"), sbuf.check("sbuf")):
        assert ok, (name, msg)
    moved = tuple(comm.get_param(c) - b for c, b in zip(COUNTERS, before))
    assert moved == want_moved, f"{name}: counters {COUNTERS} moved by {moved}, expected {want_moved}"


def main():
    rank, n, device = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "OMPI_AMD_DEVICE"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    T, trigger = types(), os.environ["OMPI_AMD_RNDV_TRIGGER"]
    for key, v in (("timeout_ms", 10000), ("p2p_timeout_ms", 10000), TRIGGERS[trigger]):  # bounded waits
        comm.set_param(key, v)
    for seed, case in enumerate(CASES):  # a failed assertion ends the rank: exit status 1
        print(f"rank {rank}: {trigger} case {case[0]}", flush=True)
        run(comm, T, 10 * seed, case, list(TRIGGERS).index(trigger))
    comm.free()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
