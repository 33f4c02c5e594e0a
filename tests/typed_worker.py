"""One rank of the typed exchange test (tests/test_typed_coll_gpu.py).

Launched N times like tests/gather_worker.py.  Every rank regenerates every
rank's seeded send image, computes the receive image it must end up with on
the CPU — oracle.pack through the sender's datatype, oracle.unpack through
its own — and compares the whole buffer byte for byte: the 64 sentinel bytes
on each side and the prefill of every byte its datatype does not own
included.  A source must come back unchanged.  The three paths are reached
with small data by setting fused_bytes / small_bytes (alltoall_chunk for
passes), and every case asserts the counters that prove its path.  Prints one
JSON line per case; exits 0 only if all passed.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import typed_random as tr  # noqa: E402
from gather_worker import Buf, PREFILL, force  # noqa: E402
from ompi_amd import coll  # noqa: E402
from ompi_amd import datatype as dt  # noqa: E402
from oracle import oracle  # noqa: E402

KINDS = ("alltoall", "alltoallv", "allgatherv", "gather", "gatherv", "scatter", "scatterv")
BYTES = None  # a side without a datatype


def make_types():
    """The datatypes of the issue: name -> (Datatype, granule the walk takes
    on a 16-B aligned buffer)."""
    f = dt.from_runs
    return {
        "v12": (f("v12", [(0, 4)], 12), 4),            # 4-B blocks at stride 12
        "v24": (f("v24", [(0, 8)], 24), 8),            # one double at stride 24
        "v48": (f("v48", [(0, 16)], 48), 16),          # 16-B blocks at stride 48
        "struct": (f("struct", [(0, 4), (8, 8)], 16), 4),        # struct {int, double}: two elements
        "idx": (f("idx", [(0, 3), (5, 5), (13, 1)], 16), 1),     # runs of 3, 5 and 1 bytes
        "resized": (f("resized", [(4, 4), (12, 8)], 32, lb=4), 4),  # lb 4, extent past the true span
        "contig": (f("contig", [(0, 8)], 8), 8),
        "c4": (f("c4", [(0, 4)], 4), 4),               # v12's signature, contiguous
    }


def runs_of(t):
    return [(0, 1)] if t is None else t.runs


def ext_of(t):
    return 1 if t is None else t.extent


def size_of(t):
    return 1 if t is None else t.size


def span_of(t):
    return 1 if t is None else max(t.true_span, t.extent)


def image(rank, seed, nbytes):
    """Rank `rank`'s seeded buffer image: every byte random, gaps included."""
    return np.random.default_rng([seed, rank, 0xD7]).integers(0, 256, nbytes, dtype=np.uint8)


def prefix_gap(counts):
    """Displacements (in elements) that leave one element between blocks."""
    d, at = [], 0
    for j, c in enumerate(counts):
        d.append(at)
        at += c + 1
    return d


class Call:
    """One typed collective on every rank's view: the count matrix, both
    layouts, the buffers of this rank and its expected receive image.

    n0: send elements per pair (uniform kinds); row: per-rank element counts
    (v kinds: alltoallv sends row[(p + q) % n] from p to q, the others
    row[sender] or row[receiver]).  Counts are in SEND elements; the receive
    side's are the same packed bytes in its own elements."""

    def __init__(self, comm, kind, st, rt, n0=0, row=None, root=0, seed=0, inplace=False, soff=0, roff=0):
        self.comm, self.kind, self.root, self.seed = comm, kind, root, seed
        self.n, self.me = comm.size, comm.rank
        self.inplace = inplace
        if inplace:  # one buffer, one datatype
            st = rt if kind not in ("scatter", "scatterv") else st
            rt = st if kind in ("scatter", "scatterv") else rt
        self.st, self.rt = st, rt
        n, me = self.n, self.me
        ssz, rsz = size_of(st), size_of(rt)
        # whole receive elements: counts in units of lcm(ssz, rsz) packed bytes
        mul = np.lcm(ssz, rsz) // ssz
        self.n0, self.row = n0 * mul, [c * mul for c in row] if row else None
        self.sends = kind not in ("scatter", "scatterv") or me == root
        self.recvs = kind not in ("gather", "gatherv") or me == root
        # the rank's own layouts (elements of its side's type)
        self.sc = [self.scount(me, q) for q in range(n)]
        self.rc = [self.scount(p, me) * ssz // rsz for p in range(n)]
        assert all(self.scount(p, me) * ssz % rsz == 0 for p in range(n))
        self.sd = self.sdispls(me)
        self.rd = self.rdispls(me)
        rbytes = (max([d + c for d, c in zip(self.rd, self.rc)] + [0]) + 1) * ext_of(rt) + span_of(rt) + 16
        if inplace and self.owns_inplace():
            init = image(me, seed, rbytes)  # my own block is in place; every other byte must survive or be received
            self.sbuf = None
        else:
            init = np.full(rbytes, PREFILL, dtype=np.uint8)
            self.sbuf = Buf(self.send_image(me), soff) if self.sends else None
        self.rbuf = Buf(init, roff) if self.recvs else None
        if self.rbuf:
            self.rbuf.expect(self.expected(init))

    # -- the count matrix and the layouts, as every rank can compute them --
    def scount(self, p, q):
        k, n = self.kind, self.n
        if k == "alltoall":
            return self.n0
        if k == "alltoallv":
            return self.row[(p + q) % n]
        if k == "allgatherv":
            return self.row[p]
        if k in ("gather", "gatherv"):
            return (self.n0 if k == "gather" else self.row[p]) if q == self.root else 0
        return (self.n0 if k == "scatter" else self.row[q]) if p == self.root else 0

    def sdispls(self, p):
        k, n = self.kind, self.n
        if k in ("alltoall", "scatter"):
            return [q * self.n0 for q in range(n)]
        if k in ("alltoallv", "scatterv"):
            return prefix_gap([self.scount(p, q) for q in range(n)])
        return [0] * n

    def rdispls(self, q):
        k, n = self.kind, self.n
        ssz, rsz = size_of(self.st), size_of(self.rt)
        rc = [self.scount(p, q) * ssz // rsz for p in range(n)]
        if k in ("alltoall", "gather"):
            return [p * rc[0] if k == "alltoall" else p * (self.n0 * ssz // rsz) for p in range(n)]
        if k in ("alltoallv", "allgatherv", "gatherv"):
            return prefix_gap(rc)
        return [0] * n

    def owns_inplace(self):
        return self.kind in ("alltoall", "alltoallv", "allgatherv") or self.me == self.root

    def send_bytes(self, p):
        sc = [self.scount(p, q) for q in range(self.n)]
        return (max([d + c for d, c in zip(self.sdispls(p), sc)] + [0]) + 1) * ext_of(self.st) \
            + span_of(self.st) + 16

    def send_image(self, p):
        """Rank p's source as the receivers see it.  In place it is p's
        initial rbuf, which this rank regenerates from the same seed."""
        if self.inplace:
            rc =[self.scount(s, p) * size_of(self.st) // size_of(self.rt) for s in range(self.n)]
            nbytes = (max([d + k for d, k in zip(self.rdispls(p), rc)] + [0]) + 1) * ext_of(self.rt) \
                + span_of(self.rt) + 16
            return image(p, self.seed, nbytes)
        return image(p, self.seed, self.send_bytes(p))

    def block_of(self, p, q):
        """(typed image, element displacement, datatype) of block p -> q at its sender."""
        if self.inplace:  # the block sits where the sender would receive it
            if self.kind == "allgatherv":
                return self.send_image(p), self.rdispls(p)[p], self.rt
            return self.send_image(p), self.rdispls(p)[q], self.rt
        return self.send_image(p), self.sdispls(p)[q], self.st

    def expected(self, init):
        want = init.copy()
        me = self.me
        for p in range(self.n):
            if self.inplace and p == me:
                continue
            cnt = self.scount(p, me)
            if not cnt:
                continue
            img, disp, t = self.block_of(p, me)
            nb = cnt * size_of(self.st)
            packed = oracle.pack(runs_of(t), ext_of(t), nb // size_of(t), img[disp * ext_of(t):], 0, nb)
            assert packed.size == nb
            oracle.unpack(runs_of(self.rt), ext_of(self.rt), self.rc[p], packed,
                          want[self.rd[p] * ext_of(self.rt):], 0)
        return want

    def refill(self, seed):
        """New input and expectation in the same buffers (persistent starts)."""
        self.seed = seed
        if self.sbuf:
            self.sbuf.set(self.send_image(self.me))
        if self.rbuf:
            init = image(self.me, seed, self.rbuf.n) if self.sbuf is None and self.inplace \
                else np.full(self.rbuf.n, PREFILL, dtype=np.uint8)
            self.rbuf.set(init)
            self.rbuf.expect(self.expected(init))

    def args(self):
        k, me, root = self.kind, self.me, self.root
        s = self.sbuf.ptr if self.sbuf else None
        r = self.rbuf.ptr if self.rbuf else None
        if self.inplace and self.owns_inplace():
            if k in ("scatter", "scatterv"):
                raise NotImplementedError
            s = coll.IN_PLACE
        at_root = me == root
        ts = (self.st, self.rt)
        if k == "alltoall":
            return (s, r, self.n0, self.rc[0]) + ts
        if k == "alltoallv":
            return (s, self.sc, self.sd, r, self.rc, self.rd) + ts
        if k == "allgatherv":
            return (s, self.sc[0], r, self.rc, self.rd) + ts
        if k == "gather":
            return (s, r, self.n0, self.rc[root] if at_root else 0, root) + ts
        if k == "gatherv":
            return (s, self.sc[root], r, self.rc if at_root else None, self.rd if at_root else None, root) + ts
        if k == "scatter":
            return (s, r, self.n0 if at_root else 0, self.rc[root], root) + ts
        return (s, self.sc if at_root else None, self.sd if at_root else None, r, self.rc[root], root) + ts

    def blocking(self, sync=True):
        getattr(self.comm, self.kind + "_typed")(*self.args(), blocking=sync)

    def post(self):
        return getattr(self.comm, "i" + self.kind + "_typed")(*self.args())

    def init(self):
        return getattr(self.comm, self.kind + "_typed_init")(*self.args())

    def run(self, form="blocking"):
        if form == "blocking":
            self.blocking()
        else:
            r = self.post()
            r.wait()
            r.free()
        return self.check()

    def check(self):
        what = f"{self.kind} {self.st.name if self.st else 'bytes'}->{self.rt.name if self.rt else 'bytes'}"
        for name, b in (("rbuf", self.rbuf), ("sbuf", self.sbuf)):
            if b is not None:
                ok, msg = b.check(f"{what} {name}")
                if not ok:
                    return ok, msg
        return True, ""


class OBuf:
    """A whole buffer image of a generated call (typed_random.Case: the 64
    guard bytes on each side and every byte the datatype skips included) on
    the device, with the buffer ORIGIN `off` bytes past a 256-B boundary:
    a datatype may own bytes below the pointer the call gets."""

    def __init__(self, image: np.ndarray, origin: int, off: int):
        self.n = image.size
        self.t = torch.empty(self.n + 768, dtype=torch.uint8, device="cuda")
        self.at = (off - origin - self.t.data_ptr()) % 256 + 256
        self.ptr = self.t.data_ptr() + self.at + origin
        self.set(image)

    def set(self, image: np.ndarray):
        self.want = image
        self.t[self.at:self.at + self.n].copy_(torch.from_numpy(image))

    def expect(self, image: np.ndarray):
        self.want = image

    def check(self, what):
        got = self.t[self.at:self.at + self.n].cpu().numpy()
        if np.array_equal(got, self.want):
            return True, ""
        bad = np.flatnonzero(got != self.want)
        return False, (f"{what}: {bad.size}/{got.size} bytes differ, first at image byte {int(bad[0])} "
                       f"(got {int(got[bad[0]])} want {int(self.want[bad[0]])}), last at {int(bad[-1])}")


class GenCall:
    """A typed_random.Case on this rank: its buffers, operands and checks."""

    def __init__(self, comm, case):
        self.comm, self.case, self.me = comm, case, comm.rank
        me = self.me
        self.sbuf = OBuf(case.send_image(me), case.origin(0, me), case.soff[me]) \
            if case.sends(me) and not case.inplace else None
        self.rbuf = OBuf(case.prefill(me), case.origin(1, me), case.roff[me]) if case.recvs(me) else None
        if self.rbuf:
            self.rbuf.expect(case.expected(me, oracle))

    def refill(self, epoch):
        """Other input and prefill in the same buffers (persistent starts)."""
        if self.sbuf:
            self.sbuf.set(self.case.send_image(self.me, epoch))
        if self.rbuf:
            self.rbuf.set(self.case.prefill(self.me, epoch))
            self.rbuf.expect(self.case.expected(self.me, oracle, epoch))

    def reset(self):
        """The receive buffer back to its prefill (the same call again)."""
        if self.rbuf:
            want = self.rbuf.want
            self.rbuf.set(self.case.prefill(self.me))
            self.rbuf.expect(want)

    def moves(self):
        """Does this rank walk a datatype in this call?"""
        c, me = self.case, self.me
        return (c.st[me] is not None and any(c.sc[me])) or (c.rt[me] is not None and any(c.rc[me]))

    def args(self):
        s = coll.IN_PLACE if self.case.inplace else (self.sbuf.ptr if self.sbuf else None)
        return self.case.args(self.me, s, self.rbuf.ptr if self.rbuf else None)

    def init(self):
        return getattr(self.comm, self.case.kind + "_typed_init")(*self.args())

    def run(self, form="blocking"):
        if form == "blocking":
            getattr(self.comm, self.case.kind + "_typed")(*self.args(), blocking=True)
        else:
            r = getattr(self.comm, "i" + self.case.kind + "_typed")(*self.args())
            r.wait()
            r.free()
        return self.check()

    def check(self):
        if self.comm.error():
            return False, f"device error {self.comm.error()}: {self.case.what()}"
        for name, b in (("rbuf", self.rbuf), ("sbuf", self.sbuf)):   # a source comes back unchanged
            if b is not None:
                ok, msg = b.check(f"{self.case.what()} {name}")
                if not ok:
                    return ok, msg
        return True, ""


def typed_paths(comm):
    return tuple(comm.get_param(k) for k in ("typed_fused", "typed_staged", "typed_landing"))


def took(comm, before, which):
    d = [a - b for a, b in zip(typed_paths(comm), before)]
    want = [0, 0, 0]
    if which is not None:
        want[which] = 1
    return d == want, f"typed path counters moved by {d}, expected {want}"


def roots(n):
    return list(range(n)) if n == 3 else sorted({0, n - 1})


def case_shapes(comm, rank, n, T):
    """Every datatype on both sides of an alltoall, 0 / 1 / 7 elements (and
    2200 of v12: three workgroup slices on the fused path at N = 2), on each
    path; the granule of each; v48 again 4 B off a 16-B boundary."""
    try:
        for path in range(3):
            force(comm, path)
            for name in ("v12", "v24", "v48", "struct", "idx", "resized", "contig"):
                t, G = T[name]
                for cnt in (0, 1, 7) + ((2200,) if name == "v12" else ()):
                    for off in (0, 4) if name == "v48" and cnt == 7 else (0,):
                        x = Call(comm, "alltoall", t, t, n0=cnt, seed=path * 100 + cnt, soff=off, roff=off)
                        before = typed_paths(comm)
                        ok, msg = x.run()
                        if ok:
                            ok, msg = took(comm, before, path if cnt else None)
                        g = comm.get_param("typed_granule")
                        print(f"# {name} cnt {cnt} off {off} path {path}: typed_granule {g}", flush=True)
                        if ok and cnt and g != (4 if off else G):
                            ok, msg = False, f"typed_granule {g}, expected {4 if off else G}"
                        if not ok:
                            return False, f"path {path} {name} x{cnt} off {off}: {msg}"
        # the landing path in three passes of 256 B whose boundaries split an
        # element (struct: 256 = 21 * 12 + 4) and a run (512 = 42 * 12 + 8, inside the double)
        force(comm, 2)
        comm.set_param("alltoall_chunk", 256)
        for name, cnt in (("struct", 58), ("idx", 78), ("v12", 175)):
            t = T[name][0]
            x = Call(comm, "alltoall", t, t, n0=cnt, seed=900 + cnt)
            p0, before = comm.get_param("alltoall_passes"), typed_paths(comm)
            ok, msg = x.run()
            if ok:
                ok, msg = took(comm, before, 2)
            grew = comm.get_param("alltoall_passes") - p0
            if ok and grew != 3:
                ok, msg = False, f"alltoall_passes grew by {grew}, expected 3"
            if not ok:
                return False, f"passes {name}: {msg}"
    finally:
        comm.set_param("alltoall_chunk", 0)
        force(comm, None)
    return True, ""


def ragged(n, seed):
    row = [(r * 5 + seed) % 11 + 1 for r in range(n)]
    row[1 % n] = 0
    return row


def case_mixed(comm, rank, n, T):
    """Send type != receive type with one signature (the transpose: a vector
    in, contiguous out, and the reverse), typed on one side only, and both
    sides typed with the own block through its slot: every collective, every
    path, every root at N = 3."""
    v12, c4, st = T["v12"][0], T["c4"][0], T["struct"][0]
    pairs = ((v12, c4), (c4, v12), (v12, BYTES), (BYTES, v12), (st, st))
    try:
        for path in range(3):
            force(comm, path)
            for kind in KINDS:
                for a, b in pairs:
                    for root in roots(n) if kind not in ("alltoall", "alltoallv", "allgatherv") else [0]:
                        x = Call(comm, kind, a, b, n0=7, row=ragged(n, path), root=root, seed=path * 31 + root)
                        before = typed_paths(comm)
                        ok, msg = x.run()
                        if ok:
                            ok, msg = took(comm, before, path)
                        if not ok:
                            return False, f"path {path} root {root}: {msg}"
    finally:
        force(comm, None)
    return True, ""


def case_inplace(comm, rank, n, T):
    """MPI_IN_PLACE alltoall and allgatherv: the typed bytes a rank reads are
    the ones it writes; gap bytes of the one buffer survive."""
    try:
        for path in range(3):
            force(comm, path)
            for name in ("v12", "struct", "idx"):
                t = T[name][0]
                for kind in ("alltoall", "allgatherv"):
                    for form in ("blocking", "post"):
                        x = Call(comm, kind, t, t, n0=9, row=[(3 * r + 2) % 7 + 1 for r in range(n)],
                                 seed=40 + path, inplace=True)
                        before = typed_paths(comm)
                        ok, msg = x.run(form)
                        if ok:
                            ok, msg = took(comm, before, path)
                        if not ok:
                            return False, f"path {path} {name} {form}: {msg}"
    finally:
        force(comm, None)
    return True, ""


def case_forms(comm, rank, n, T):
    """i* and *_init of all seven on each path: plan.kind == 4, started twice
    with the source changed in between."""
    v12, st = T["v12"][0], T["struct"][0]
    try:
        for path in range(3):
            force(comm, path)
            for k, kind in enumerate(KINDS):
                a, b = ((v12, v12), (st, st), (v12, BYTES))[(k + path) % 3]
                x = Call(comm, kind, a, b, n0=11, row=ragged(n, k), root=(k + path) % n, seed=300 + k)
                ok, msg = x.run("post")
                if not ok:
                    return False, f"i{kind} path {path}: {msg}"
                plan = x.init()
                if plan.kind != 4:
                    plan.free()
                    return False, f"plan kind {plan.kind}"
                for start in range(2):
                    x.refill(310 + 2 * k + start)
                    torch.cuda.synchronize()
                    before = typed_paths(comm)
                    plan.start()
                    plan.wait()
                    ok, msg = x.check()
                    if ok:
                        ok, msg = took(comm, before, path)
                    if not ok:
                        plan.free()
                        return False, f"{kind} plan path {path} start {start}: {msg}"
                plan.free()
    finally:
        force(comm, None)
    return True, ""


def case_force64(comm, rank, n, T):
    """typed_force64: the 64-bit walk at a small size, once per collective."""
    st = T["struct"][0]
    comm.set_param("typed_force64", 1)
    try:
        for k, kind in enumerate(KINDS):
            x = Call(comm, kind, st, st, n0=13, row=ragged(n, 3), root=k % n, seed=500 + k)
            w0 = comm.get_param("typed_walk64")
            ok, msg = x.run()
            grew = comm.get_param("typed_walk64") - w0
            moves = (x.sends and sum(x.sc) > 0) or (x.recvs and sum(x.rc) > 0)  # a zero row walks nothing
            if ok and moves and grew < 1:
                ok, msg = False, "typed_walk64 did not move"
            if not ok:
                return False, f"{kind}: {msg}"
    finally:
        comm.set_param("typed_force64", 0)
    w0 = comm.get_param("typed_walk64")
    ok, msg = Call(comm, "alltoall", st, st, n0=13, seed=520).run()
    if ok and comm.get_param("typed_walk64") != w0:
        ok, msg = False, "the 32-bit walk counted as 64-bit"
    return ok, msg


def case_interleave(comm, rank, n, T):
    """A byte alltoall between two typed calls on one communicator with no
    host sync: the scratch halves and the epochs still pair."""
    v12 = T["v12"][0]
    try:
        for path in range(3):
            force(comm, path)
            B = 1000
            x = Call(comm, "alltoall", v12, v12, n0=50, seed=600 + path)
            y = Call(comm, "gatherv", v12, BYTES, row=ragged(n, 4), root=n - 1, seed=610 + path)
            src = np.concatenate([image(rank, 620 + q, B) for q in range(n)])
            want = np.concatenate([image(p, 620 + rank, B) for p in range(n)])
            s = torch.from_numpy(src).cuda()
            r = torch.zeros(B * n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            x.blocking(sync=False)
            comm.alltoall(s, r, B)
            y.blocking(sync=False)
            torch.cuda.synchronize()
            if comm.error():
                return False, f"device error {comm.error()}"
            for c in (x, y):
                ok, msg = c.check()
                if not ok:
                    return False, f"path {path}: {msg}"
            if not np.array_equal(r.cpu().numpy(), want):
                return False, f"path {path}: the byte alltoall between the typed calls differs"
    finally:
        force(comm, None)
    return True, ""


EXTRA = {}   # case name -> further fields of its JSON line


def case_layouts(comm, rank, n, T):
    """Generated calls (typed_random.worker_case) on each forced path: every
    rank with datatypes of its own, all seven kinds, every root at N = 3,
    ragged rows with a zero, in place, more than 16 KiB per pair, passes of
    256 B, two full trips of byte granules per fused workgroup, the 64-bit
    walk.  N = 8 runs the shorter list typed_random.WORKER_SEEDS_N8 (the kinds
    of seeds 0-4 and the four directed seeds).  Reports the granules this
    rank's launches took."""
    gs = set()
    try:
        for path in range(3):
            force(comm, path)
            for s in tr.WORKER_SEEDS_N8 if n == 8 else range(tr.WORKER_SEEDS):
                case, meta = tr.worker_case(s, n, path)
                chunked = meta["chunk"] and path == 2
                comm.set_param("alltoall_chunk", meta["chunk"] if chunked else 0)
                comm.set_param("typed_force64", meta["force64"])
                x = GenCall(comm, case)
                before, w0 = typed_paths(comm), comm.get_param("typed_walk64")
                p0 = comm.get_param("alltoall_passes") + comm.get_param("gather_passes")
                ok, msg = x.run("post" if s % 4 == 3 else "blocking")
                if ok:
                    ok, msg = took(comm, before, path)
                g = comm.get_param("typed_granule")
                print(f"# layouts path {path} seed {s}: typed_granule {g} {case.what()}", flush=True)
                if x.moves():
                    gs.add(g)
                    if ok and meta["G"] and g != meta["G"]:
                        ok, msg = False, f"typed_granule {g}, expected {meta['G']}"
                    if ok and meta["force64"] and comm.get_param("typed_walk64") == w0:
                        ok, msg = False, "typed_walk64 did not move"
                passes = comm.get_param("alltoall_passes") + comm.get_param("gather_passes") - p0
                most = max(max(row) for row in case.B)
                if ok and chunked and passes != -(-most // 256):
                    ok, msg = False, f"{passes} passes, expected {-(-most // 256)}"
                if not ok:
                    return False, f"path {path} seed {s}: {msg}"
    finally:
        comm.set_param("alltoall_chunk", 0)
        comm.set_param("typed_force64", 0)
        force(comm, None)
        EXTRA["layouts"] = {"granules": sorted(gs)}
    return True, ""


CASES = [("shapes", case_shapes), ("mixed", case_mixed), ("inplace", case_inplace), ("forms", case_forms),
         ("force64", case_force64), ("interleave", case_interleave), ("layouts", case_layouts)]


def report(rank, n, obj):
    line = json.dumps(obj)
    print(line, flush=True)
    d = os.environ.get("COLL_LOG_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"typed_n{n}_rank{rank}.jsonl"), "a") as f:
            f.write(line + "\n")


def main():
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = int(os.environ.get("OMPI_AMD_DEVICE", "0"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lost signal is an error line, not a kill
    force(comm, None)
    T = make_types()
    only = set(filter(None, os.environ.get("TYPED_CASES", "").split(",")))
    ok_all = True
    for name, fn in CASES:
        if only and name not in only:
            continue
        t0 = time.time()
        try:
            ok, msg = fn(comm, rank, n, T)
        except Exception as e:  # noqa: BLE001 — a library error is the case's failure
            ok, msg = False, f"{type(e).__name__}: {e}"
        report(rank, n, {"rank": rank, "case": name, "ok": bool(ok), "msg": msg,
                         "s": round(time.time() - t0, 3), **EXTRA.pop(name, {})})
        ok_all = ok_all and ok
        if comm.error():  # the communicator is unusable after a device error
            break
    if not comm.error():
        comm.free()
    dist.destroy_process_group()
    sys.exit(0 if ok_all else 1)


if __name__ == "__main__":
    main()
