"""One rank of tests/test_alltoallw_gpu.py.  Every pair has its own datatypes and
byte count; a rank gathers its blocks from the senders' seeded images through
their run lists, scatters them through its own and compares whole buffers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from gather_worker import Buf, PREFILL, force  # noqa: E402
from ompi_amd import coll, datatype as dt  # noqa: E402

LDS_ELEMS = 256  # coll_kernels.h kA2awLdsElems: the element programs one table may stage


def pool(big):
    """What a pair draws from; None is bytes.  big: the indexed type alone passes the LDS budget."""
    lens = [1, 2] * 120 + [1, 3] * 30 if big else [1, 3, 2, 5, 1, 3, 2, 4, 1, 2]
    runs = [(sum(lens[:i]) + i, ln) for i, ln in enumerate(lens)]  # neighbours differ and never touch
    idx = dt.from_runs("idx", runs, sum(lens) + len(lens) + 3)     # 1-B granule, size 24 (480), odd extent
    assert idx.nelems == len(lens) and (idx.nelems > LDS_ELEMS if big else idx.nelems > 8)
    vec = dt.type_vector(3, 1, 2, dt.predefined("MPI_INT"))  # 4-B granule: size 12, extent 20
    st = dt.from_runs("struct", [(0, 16), (32, 32)], 80)     # 16-B granule, two elements: size 48
    return [idx, vec, st, None]


def offs(t, count):
    """Byte offsets, in packed order, of `count` elements of t."""
    runs, extent = (t.runs, t.extent) if t else ([(0, 1)], 1)
    one = np.concatenate([np.arange(d, d + ln) for d, ln in runs])
    return (np.arange(count)[:, None] * extent + one).ravel()


def image(rank, seed, nbytes):
    return np.random.default_rng([seed, rank, 0xA2]).integers(0, 256, nbytes, dtype=np.uint8)


class Call:
    """One alltoallw as every rank can compute it."""

    def __init__(self, comm, seed, big=False, inplace=False):
        self.n, self.me, self.inplace, self.P = comm.size, comm.rank, inplace, pool(big)
        self.unit, self.step = int(np.lcm.reduce([t.size for t in self.P if t])), 1 if big else 17
        st, sc, sd, sbytes = self.side(self.me, False)
        self.rt, self.rc, self.rd, rbytes = self.side(self.me, True)
        self.sbuf = None if inplace else Buf(np.zeros(sbytes, np.uint8), 0)
        self.rbuf = Buf(np.zeros(rbytes, np.uint8), 0)
        send = (coll.IN_PLACE, None, None, None) if inplace else (self.sbuf.ptr, sc, sd, st)
        self.args = send + (self.rbuf.ptr, self.rc, self.rd, self.rt)
        act = {id(t): t.nelems for t, c in zip(st + self.rt, sc + self.rc) if t and c}
        self.staged = 0 < sum(act.values()) <= LDS_ELEMS  # the programs that move data fit the LDS budget
        self.seed = seed

    def pair(self, p, q):
        """Packed bytes of p -> q: up to 4944 (two fused workgroups), one pair 0."""
        if self.inplace:  # both directions of a pair through one description
            p, q = min(p, q), max(p, q)
        elif self.n > 1 and (p, q) == (0, self.n - 1):
            return 0
        return self.unit * (1 + self.step * ((5 * p + 3 * q + 6) % 7))

    def side(self, r, recv):
        """Rank r's datatypes, counts, byte displacements and buffer bytes (in place: the receive side's)."""
        recv = recv or self.inplace
        ts = [self.P[(2 * r + 3 * p + 1 if recv else r + p) % 4] for p in range(self.n)]
        cs = [(self.pair(p, r) if recv else self.pair(r, p)) // (t.size if t else 1) for p, t in enumerate(ts)]
        ds, at = [], 16  # 16 is a multiple of no extent of the pool; peer 1 sits one byte further
        for p, (t, c) in enumerate(zip(ts, cs)):
            ds.append(at + (p == 1))
            at += -(-(c * t.extent + max(t.true_span, t.extent) if t else c) // 16) * 16 + 16
        return ts, cs, ds, at + 16

    def fill(self, seed):
        """The input of `seed` into the buffers, and what rbuf must hold after the call."""
        self.seed = seed
        if self.sbuf:
            self.sbuf.set(image(self.me, seed, self.sbuf.n))
        want = image(self.me, seed, self.rbuf.n) if self.inplace else np.full(self.rbuf.n, PREFILL, np.uint8)
        self.rbuf.set(want)
        for p in range(self.n):
            if not (self.inplace and p == self.me):
                ts, cs, ds, nbytes = self.side(p, False)
                src = image(p, seed, nbytes)[ds[self.me] + offs(ts[self.me], cs[self.me])]
                want[self.rd[p] + offs(self.rt[p], self.rc[p])] = src
        self.rbuf.expect(want)


def run(comm, path, x, form, passes):
    """x in one form (a plan: started twice).  Each launch moves its path's counter and alltoallw_calls
    by one, makes `passes` passes where given, and counts LDS launches exactly when the programs fit."""
    want = {**{k: int(path == i) for i, k in enumerate(("typed_fused", "typed_staged", "typed_landing"))},
            "alltoallw_calls": 1, **({"alltoall_passes": passes} if passes else {})}
    plan = comm.alltoallw_init(*x.args) if form == "plan" else None
    try:
        assert not plan or plan.kind == 4, f"plan kind {plan.kind}"
        for _ in range(2 if plan else 1):
            x.fill(x.seed + 50)
            torch.cuda.synchronize()
            before = {k: comm.get_param(k) for k in (*want, "alltoallw_lds_programs")}
            if plan:
                plan.start()
                plan.wait()
            elif form == "post":
                r = comm.ialltoallw(*x.args)
                r.wait()
                r.free()
            else:
                comm.alltoallw(*x.args, blocking=True)
            assert not comm.error(), f"device error {comm.error()}"
            for name in ("rbuf", "sbuf"):  # the source must come back unchanged
                ok, msg = getattr(x, name).check(name) if getattr(x, name) else (True, "")
                assert ok, msg
            d = {k: comm.get_param(k) - b for k, b in before.items()}
            lds = d.pop("alltoallw_lds_programs")
            # (LDS launches are not judged in place, where the own pair's datatype moves nothing)
            assert d == want and (x.inplace or (lds > 0) == x.staged), \
                f"counters moved by {d}, expected {want}; {lds} LDS launches, programs fit: {x.staged}"
    finally:
        if plan:
            plan.free()


def main():
    rank, n, device = (int(os.environ[k]) for k in ("RANK", "WORLD_SIZE", "OMPI_AMD_DEVICE"))
    path = int(os.environ["A2AW_PATH"]) if n > 1 else None  # one rank: the local route only
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lost signal is an error line, not a kill
    force(comm, path)
    # big: the 300-element indexed type, so the ranks it reaches walk global memory
    cases = [("blocking", {}, 0), ("post", {}, 0), ("plan", {}, 0), ("blocking", dict(inplace=True), 0),
             ("blocking", dict(big=True), 0)]
    if path == 2:  # the 4944-B largest pair in 5 passes of 1024 B, and
        # 1024 = 42 * 24 + 16 cuts what 1 sends inside the receivers' indexed 2-B run [15, 17)
        cases.append(("blocking", {}, 5))
    for seed, (form, kw, passes) in enumerate(cases):  # a failed assertion ends the rank: exit status 1
        print(f"rank {rank}: case {seed} ({form} {kw})", flush=True)
        comm.set_param("alltoall_chunk", 1024 if passes else 0)
        run(comm, path, Call(comm, seed, **kw), form, passes)
    comm.free()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
