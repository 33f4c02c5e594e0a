"""One rank of tests/test_osc_ddt2_gpu.py: one-sided calls with a derived datatype on the origin (and result)
side, which run without a packed stream.  Rank r targets rank r + 1 inside lock(EXCLUSIVE) ..
unlock unless the case says otherwise.  The reference is numpy, stream = origin_image[offs(odt, oc)] scattered at
offs(tdt, tc); whole buffers (window, origin, result, gaps included) are compared byte for byte, and every case
asserts how far (osc_ddt_fused, osc_ddt_packed, osc_ddt_lds) moved."""
import os

import numpy as np

from p2p_typed_worker import PREFILL, Buf, coll, dist, image, offs, span, torch, types
from ompi_amd import op as mop, osc

COUNTERS = ("osc_ddt_fused", "osc_ddt_packed", "osc_ddt_lds")
WIN_BYTES = 4 << 20
F, FG, P = (1, 0, 1), (1, 0, 0), (0, 1, 0)  # fused with the programs in LDS; fused, a global walk; packed

# name: origin, target (type, count), target displacement, granule, counters per call, options
PUT_GET = [
    ("one_lane", ("v4", 1), ("v4", 1), 0, 4, F, {}),
    ("two_types", ("v64", 512), ("v4", 2048), 0, 4, F, {}),                      # 8 KiB
    ("many_groups", ("v8", 26216), ("w16", 32770), 8, 8, F, {}),                 # 1 048 640 B, target base 8 mod 16
    ("global_walk", ("big", 17), ("big", 17), 0, 1, FG, {}),                     # 300 elements, one table
    ("contig_target", ("idx", 410), (None, 4100), 0, 1, F, {}),
    ("self", ("v64", 512), ("v4", 2048), 0, 4, F, {"self": True}),
    ("knob_off", ("v64", 512), ("v4", 2048), 0, None, P, {"fuse": 0}),
]
# name: element type, op, origin, target, result (type, count; None: not fetched), counters, options
ACC = [
    ("n1", mop.MPI_INT, mop.MPI_SUM, ("v4", 1), ("v4", 1), None, F, {}),
    ("ragged", mop.MPI_INT, mop.MPI_SUM, ("v4", 1025), ("v4", 1025), (None, 1025), F, {}),  # 256 x 4 + 1
    ("three_types", mop.MPI_INT, mop.MPI_SUM, ("v64", 512), ("w16", 256), ("s16", 512), F, {}),
    ("fp64", mop.MPI_DOUBLE, mop.MPI_SUM, ("v8", 256), ("w16", 320), None, F, {}),            # 10 240 B
    ("bytes_global", mop.MPI_UINT8_T, mop.MPI_SUM, ("big", 17), ("big", 17), None, FG, {}),
    ("replace", mop.MPI_INT, mop.MPI_REPLACE, ("v64", 512), ("w16", 256), ("s16", 512), F, {}),
    ("no_op", mop.MPI_INT, mop.MPI_NO_OP, None, ("w16", 256), ("s16", 512), F, {}),
    ("contended", mop.MPI_INT, mop.MPI_SUM, ("v64", 512), ("w16", 256), None, F, {"contended": True}),
]


def img(prim, rank, seed, nbytes):
    """A buffer's bytes; of integer-valued doubles where the elements are fp64 (sums are exact)."""
    if prim is not mop.MPI_DOUBLE:
        return image(rank, seed, nbytes)
    v = np.random.default_rng([seed, rank, 0x7F]).integers(-1000, 1000, nbytes // 8 + 1).astype(np.float64)
    return v.view(np.uint8)[:nbytes].copy()


class Run:
    def __init__(self, comm, win):
        self.comm, self.win, self.T, self.me, self.n = comm, win, types(), comm.rank, comm.size
        self.back = torch.empty(WIN_BYTES, dtype=torch.uint8, device="cuda")

    def fill(self, host):
        """My window's first bytes (a contiguous put to myself), everywhere, before anyone's call."""
        src = Buf(host, 0)
        self.win.lock(self.me)
        self.win.put(src.ptr, self.me, 0, host.size)
        self.win.unlock(self.me)
        self.win.fence(blocking=True)

    def window_is(self, want, name):
        self.win.fence(blocking=True)  # every origin's epoch is closed
        self.win.lock(self.me, osc.LOCK_SHARED)
        self.win.get(self.back, self.me, 0, want.size)
        self.win.unlock(self.me)
        got = self.back[:want.size].cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: window differs at {bad.size} bytes, first {bad[:1]}"
        assert not self.comm.error(), f"device error {self.comm.error()}"

    def counted(self, name, want, call, *args):
        before = [self.comm.get_param(c) for c in COUNTERS]
        call(*args)
        moved = tuple(self.comm.get_param(c) - b for c, b in zip(COUNTERS, before))
        assert moved == want, f"{name}: counters {COUNTERS} moved by {moved}, expected {want}"

    def put_get(self, seed, case):
        name, (ot, oc), (tt, tc), disp, gran, moved, opt = case
        ot, tt, win, me, n = self.T[ot], self.T.get(tt), self.win, self.me, self.n
        tgt, frm = (me, me) if opt.get("self") else ((me + 1) % n, (me - 1) % n)
        W = disp + span(tt, tc) + 64
        self.comm.set_param("osc_ddt_fuse", opt.get("fuse", 1))
        self.fill(image(me, seed + 1, W))
        obuf = Buf(image(me, seed, span(ot, oc)), 0)
        back = Buf(np.full(span(ot, oc), PREFILL, np.uint8), 0)
        win.lock(tgt)
        self.counted(name, moved, win.put_ddt, obuf.ptr, oc, ot, tgt, disp, tc, tt)
        assert gran is None or self.comm.get_param("osc_ddt_granule") == gran, (name, "put granule")
        win.unlock(tgt)
        win.lock(tgt)  # what the put left there, back through the same two layouts
        self.counted(name, moved, win.get_ddt, back.ptr, oc, ot, tgt, disp, tc, tt)
        win.unlock(tgt)
        want = image(me, seed + 1, W)
        want[disp + offs(tt, tc)] = image(frm, seed, span(ot, oc))[offs(ot, oc)]
        self.window_is(want, name)
        got = np.full(back.n, PREFILL, np.uint8)
        got[offs(ot, oc)] = obuf.want[64:64 + obuf.n][offs(ot, oc)]
        back.expect(got)
        for b, what in ((obuf, "origin"), (back, "get origin")):
            ok, msg = b.check(what)
            assert ok, (name, msg)
        self.comm.set_param("osc_ddt_fuse", 1)

    def acc(self, seed, case, fill=True):
        """self.wins models every rank's window (all images are functions of rank and seed); fill=False goes on
        from what the previous case left."""
        name, prim, op, o, (tt, tc), r, moved, opt = case
        T, win, me, n, nd = self.T, self.win, self.me, self.n, prim.np_dtype
        tt, (ot, oc), (rt, rc) = T[tt], (T[o[0]], o[1]) if o else (None, 0), (T.get(r[0]), r[1]) if r else (None, 0)
        rbytes = rc * (1 if rt else prim.size)  # a contiguous result: rc elements
        W, at, shared = span(tt, tc) + 64, offs(tt, tc), opt.get("contended")
        if fill:
            self.fill(img(prim, me, seed + 1, W))
            self.wins = [img(prim, p, seed + 1, W) for p in range(n)]
        tgt = 0 if shared else (me + 1) % n
        held = self.wins[tgt][at].copy()  # what my target holds before its one origin's call (not contended)
        for p in range(n if o else 0):
            t, s = 0 if shared else (p + 1) % n, img(prim, p, seed, span(ot, oc))[offs(ot, oc)].view(nd)
            self.wins[t][at] = (s if op is mop.MPI_REPLACE else self.wins[t][at].view(nd) + s).view(np.uint8)
        obuf = Buf(img(prim, me, seed, span(ot, oc)), 0) if o else None
        rbuf = Buf(np.full(span(rt, rbytes if not rt else rc), PREFILL, np.uint8), 0) if r else None
        win.lock_all() if shared else win.lock(tgt)
        if r:
            self.counted(name, moved, win.get_accumulate_ddt, obuf.ptr if o else None, oc, ot, rbuf.ptr, rc, rt,
                         tgt, 0, tc, tt, prim, op)
        else:
            self.counted(name, moved, win.accumulate_ddt, obuf.ptr, oc, ot, tgt, 0, tc, tt, prim, op)
        win.unlock_all() if shared else win.unlock(tgt)
        self.window_is(self.wins[me], name)  # integer wrap, or exact fp64: one add per element and origin
        if r:
            got = np.full(rbuf.n, PREFILL, np.uint8)
            got[offs(rt, rbytes if not rt else rc)] = held
            rbuf.expect(got)
        for b, what in ((obuf, "origin"), (rbuf, "result")):
            ok, msg = b.check(what) if b else (True, "")
            assert ok, (name, msg)


def main():
    rank, n, device = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "OMPI_AMD_DEVICE"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lock that is never granted is an error line, not a kill
    win = osc.Window.allocate(comm, WIN_BYTES)
    run = Run(comm, win)
    for seed, case in enumerate(PUT_GET):  # a failed assertion ends the rank: exit status 1
        print(f"rank {rank}: put+get {case[0]}", flush=True)
        run.put_get(10 * seed, case)
    for seed, case in enumerate(ACC):
        print(f"rank {rank}: acc {case[0]}", flush=True)
        run.acc(100 + 10 * seed, case, fill=case[0] != "no_op")
    win.free()
    comm.free()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
