"""One rank of the alltoall / alltoallv test (tests/test_alltoall_gpu.py).

Launched N times like tests/coll_worker.py.  Rank r fills block r -> q with
bytes f(r, q, i, seed); every rank computes the rbuf it must end up with from
that formula alone (nothing is exchanged, no oracle) and compares byte for
byte, the 64 sentinel bytes on each side of rbuf and the prefill of every gap
included.  The thresholds are shrunk so that small shapes reach every path:
fused_bytes 4096, small_bytes 65536, and alltoall_chunk 32768 where a case
needs passes.  Prints one JSON line per case; exits 0 only if all passed.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from ompi_amd import coll  # noqa: E402
from ompi_amd import op as mop  # noqa: E402

FUSED, SMALL, CHUNK = 4096, 65536, 32768
PREFILL, SENTINEL = 0x5A, 0xA5


def block(r, q, nbytes, seed):
    """Bytes of block r -> q."""
    i = np.arange(nbytes, dtype=np.int64)
    return ((r * 131 + q * 31 + i * 7 + (i >> 8) * 13 + seed * 17 + 3) & 0xFF).astype(np.uint8)


class Buf:
    """`nbytes` of device memory starting `off` bytes past a 256-B boundary,
    with 64 sentinel bytes on each side."""

    def __init__(self, host: np.ndarray, off: int):
        n = host.size
        self.t = torch.empty(n + 1024, dtype=torch.uint8, device="cuda")
        self.lo = (-self.t.data_ptr()) % 256 + 256 + off
        img = np.full(n + 128, SENTINEL, dtype=np.uint8)
        img[64:64 + n] = host
        self.n = n
        self.t[self.lo - 64:self.lo + n + 64].copy_(torch.from_numpy(img))
        self.ptr = self.t.data_ptr() + self.lo

    def set(self, host: np.ndarray):
        self.t[self.lo:self.lo + self.n].copy_(torch.from_numpy(host))

    def image(self) -> np.ndarray:
        return self.t[self.lo - 64:self.lo + self.n + 64].cpu().numpy()


class Xfer:
    """One exchange with count matrix S (S[p][q] bytes p -> q): its buffers,
    displacements and the rbuf image this rank expects."""

    def __init__(self, rank, n, S, seed, soff=0, roff=0, inplace=False, desc=False, gap=0):
        S = np.asarray(S, dtype=np.int64)
        self.rank, self.n, self.seed, self.inplace = rank, n, seed, inplace
        self.sc = [int(v) for v in S[rank, :]]
        self.rc = [int(v) for v in S[:, rank]]
        if inplace:
            assert self.sc == self.rc, "in place needs a symmetric matrix"
        self.sd, self.rd = self.layout(self.sc, desc, 0), self.layout(self.rc, desc, gap)
        stot = max([d + c for d, c in zip(self.sd, self.sc)] + [0])
        rtot = max([d + c for d, c in zip(self.rd, self.rc)] + [0]) + gap
        self.rbuf = Buf(self.rimage(seed, initial=True, total=rtot), roff)
        self.sbuf = None if inplace else Buf(self.simage(seed, stot), soff)
        self.rtot = rtot
        self.expect(seed)

    @staticmethod
    def layout(counts, desc, gap):
        order = range(len(counts) - 1, -1, -1) if desc else range(len(counts))
        d, at = [0] * len(counts), gap
        for p in order:
            d[p] = at
            at += counts[p] + gap
        return d

    def simage(self, seed, total=None):
        img = np.zeros(self.sbuf.n if total is None else total, dtype=np.uint8)
        for q in range(self.n):
            img[self.sd[q]:self.sd[q] + self.sc[q]] = block(self.rank, q, self.sc[q], seed)
        return img

    def rimage(self, seed, initial, total=None):
        img = np.full(self.rtot if total is None else total, PREFILL, dtype=np.uint8)
        for p in range(self.n):
            if initial and not self.inplace:
                break
            src = (self.rank, p) if initial else (p, self.rank)
            img[self.rd[p]:self.rd[p] + self.rc[p]] = block(src[0], src[1], self.rc[p], seed)
        return img

    def expect(self, seed):
        self.want = np.full(self.rtot + 128, SENTINEL, dtype=np.uint8)
        self.want[64:64 + self.rtot] = self.rimage(seed, initial=False)

    def refill(self, seed):
        """New input (and expectation) in the same buffers: persistent starts."""
        self.seed = seed
        if self.inplace:
            self.rbuf.set(self.rimage(seed, initial=True))
        else:
            self.sbuf.set(self.simage(seed))
            self.rbuf.set(np.full(self.rtot, PREFILL, dtype=np.uint8))
        self.expect(seed)

    @property
    def s(self):
        return coll.IN_PLACE if self.inplace else self.sbuf.ptr

    def v_args(self):
        if self.inplace:
            return (coll.IN_PLACE, None, None, self.rbuf.ptr, self.rc, self.rd)
        return (self.sbuf.ptr, self.sc, self.sd, self.rbuf.ptr, self.rc, self.rd)

    def check(self):
        got = self.rbuf.image()
        if np.array_equal(got, self.want):
            return True, ""
        bad = np.flatnonzero(got != self.want)
        return False, (f"{bad.size}/{got.size} bytes differ, first at {int(bad[0]) - 64} "
                       f"(got {int(got[bad[0]])} want {int(self.want[bad[0]])}), last at "
                       f"{int(bad[-1]) - 64}; rc {self.rc} rd {self.rd}")


def uniform(n, B):
    return np.full((n, n), B, dtype=np.int64)


def run(comm, x, api, B=None):
    """One blocking-style run of exchange x through `api`."""
    if api == "alltoall":
        comm.alltoall(x.s, x.rbuf.ptr, B, blocking=True)
    elif api == "alltoallv":
        comm.alltoallv(*x.v_args(), blocking=True)
    elif api == "ialltoall":
        r = comm.ialltoall(x.s, x.rbuf.ptr, B)
        r.wait()
        r.free()
    elif api == "ialltoallv":
        r = comm.ialltoallv(*x.v_args())
        r.wait()
        r.free()
    else:
        raise ValueError(api)
    return x.check()


def paths(comm):
    return tuple(comm.get_param(k) for k in ("alltoall_fused", "alltoall_staged", "alltoall_landing"))


def took(comm, before, which):
    """The one call since `before` ran on path `which` (0 fused, 1 staged, 2 landing)."""
    d = [a - b for a, b in zip(paths(comm), before)]
    want = [0, 0, 0]
    want[which] = 1
    return (d == want), f"path counters moved by {d}, expected {want}"


def case_sizes(comm, rank, n):
    """alltoall at every size where the path changes, and the edge sizes."""
    below, above = FUSED // n, FUSED // n + 1
    plan = [(0, None), (1, 0), (12, 0), (below, 0), (above, 1), (SMALL, 1), (SMALL + 16, 2)]
    for k, (B, path) in enumerate(plan):
        x = Xfer(rank, n, uniform(n, B), seed=k)
        before = paths(comm)
        ok, msg = run(comm, x, "alltoall", B)
        if ok and path is not None:
            ok, msg = took(comm, before, path)
        if ok and path is None and paths(comm) != before:
            ok, msg = False, "a zero-byte alltoall took a path"
        if not ok:
            return False, f"B={B}: {msg}"
    # passes: 100000 B per pair in chunks of 32768 -> 4 passes, the last ragged
    comm.set_param("alltoall_chunk", CHUNK)
    try:
        for api in ("alltoall", "alltoallv"):
            p0 = comm.get_param("alltoall_passes")
            x = Xfer(rank, n, uniform(n, 100000), seed=40)
            ok, msg = run(comm, x, api, 100000)
            grew = comm.get_param("alltoall_passes") - p0
            if ok and grew != 4:
                ok, msg = False, f"alltoall_passes grew by {grew}, expected 4"
            if not ok:
                return False, f"{api} in passes: {msg}"
    finally:
        comm.set_param("alltoall_chunk", 0)
    return True, ""


def path_sizes(n):
    """A per-pair size on each path: fused, staged, landing (none a multiple of 16)."""
    return (FUSED // n - 3, 5003, SMALL + 4001)


def case_misaligned(comm, rank, n):
    """Each path with sbuf / rbuf at (0,0), (4,4), (1,3) past a 256-B
    boundary: vector body with head and tail, and no common alignment."""
    for path, B in enumerate(path_sizes(n)):
        for soff, roff in ((0, 0), (4, 4), (1, 3)):
            for api in ("alltoall", "alltoallv"):
                x = Xfer(rank, n, uniform(n, B), seed=soff + roff + path, soff=soff, roff=roff)
                before = paths(comm)
                ok, msg = run(comm, x, api, B)
                if ok:
                    ok, msg = took(comm, before, path)
                if not ok:
                    return False, f"{api} B={B} offsets ({soff},{roff}): {msg}"
    return True, ""


def sym_matrix(n, hi, seed, zeros=True):
    rng = np.random.default_rng(seed)  # the same on every rank
    S = rng.integers(0, hi + 1, (n, n))
    S = np.triu(S) + np.triu(S, 1).T
    if zeros:
        S[0, n - 1] = S[n - 1, 0] = 0
    S[0, 0] = hi  # the call's largest pair: fixes the path
    return S


def case_inplace(comm, rank, n):
    """MPI_IN_PLACE on each path, both calls (alltoallv: rcounts / rdispls
    describe both sides)."""
    for path, B in enumerate(path_sizes(n)):
        for api in ("alltoall", "ialltoall"):
            x = Xfer(rank, n, uniform(n, B), seed=60 + path, inplace=True, roff=4 * path)
            before = paths(comm)
            ok, msg = run(comm, x, api, B)
            if ok:
                ok, msg = took(comm, before, path)
            if not ok:
                return False, f"{api} in place B={B}: {msg}"
        for api in ("alltoallv", "ialltoallv"):
            x = Xfer(rank, n, sym_matrix(n, B, 70 + path), seed=70 + path, inplace=True, gap=5)
            before = paths(comm)
            ok, msg = run(comm, x, api)
            if ok:
                ok, msg = took(comm, before, path)
            if not ok:
                return False, f"{api} in place M={B}: {msg}"
    return True, ""


def case_v_variants(comm, rank, n):
    fused_hi = FUSED // n - 1
    rng = np.random.default_rng(20261020)  # shared by every rank
    variants = []
    S = rng.integers(0, fused_hi + 1, (n, n))
    S[rng.random((n, n)) < 0.3] = 0
    variants.append(("random with zero pairs", S, {}, None))
    S = rng.integers(1, fused_hi + 1, (n, n))
    S[n - 1, :] = 0
    variants.append(("one rank sends nothing", S, {}, None))
    S = rng.integers(1, fused_hi + 1, (n, n))
    S[:, 0] = 0
    variants.append(("one rank receives nothing", S, {}, None))
    variants.append(("descending displacements", rng.integers(1, fused_hi + 1, (n, n)), {"desc": True}, None))
    variants.append(("gaps keep their prefill", rng.integers(0, 3000, (n, n)), {"gap": 7}, None))
    variants.append(("all zero", np.zeros((n, n), dtype=np.int64), {}, None))
    for path, M in enumerate(path_sizes(n)):  # M puts the call on each path
        S = rng.integers(0, M // 2, (n, n))
        S[n - 1, 0] = M
        variants.append((f"M={M} on path {path}", S, {"gap": 3, "soff": 1, "roff": 3}, path))
    # a path chosen from local counts would differ between the ranks here:
    # only pair 1 -> 0 is above small_bytes, every other rank sees 8-B pairs
    S = np.full((n, n), 8, dtype=np.int64)
    S[1, 0] = SMALL + 777
    variants.append(("one large pair elsewhere", S, {}, 2))
    comm.set_param("alltoall_chunk", CHUNK)
    try:
        S = rng.integers(0, 3 * CHUNK, (n, n))
        S[0, n - 1] = 3 * CHUNK + 1234
        for api in ("alltoallv", "ialltoallv"):
            p0 = comm.get_param("alltoall_passes")
            x = Xfer(rank, n, S, seed=99, gap=1)
            ok, msg = run(comm, x, api)
            grew = comm.get_param("alltoall_passes") - p0
            if ok and grew != 4:
                ok, msg = False, f"alltoall_passes grew by {grew}, expected 4"
            if not ok:
                return False, f"{api} ragged passes: {msg}"
    finally:
        comm.set_param("alltoall_chunk", 0)
    for k, (name, S, kw, path) in enumerate(variants):
        for api in ("alltoallv", "ialltoallv"):
            x = Xfer(rank, n, S, seed=100 + k, **kw)
            before = paths(comm)
            ok, msg = run(comm, x, api)
            if ok and path is not None:
                ok, msg = took(comm, before, path)
            if not ok:
                return False, f"{api}, {name}: {msg}"
    return True, ""


def case_reuse(comm, rank, n):
    """64 calls back to back on one stream with no host sync: fused alltoall,
    fused allreduce, staged allgather, fused alltoallv in turn — the scratch
    halves and the flag rows they share.  Everything is checked at the end.
    The allreduce's inputs are the exact values k * 2^-8 (coll_worker.py's
    dataset "E": every summation order gives the same bits, so numpy's sum is
    the reference).  That every call took the intended path is asserted: the
    alltoalls by their path counters, all 64 by the communicator's epoch —
    a fused kernel and a staged allgather take one epoch each, while a staged
    two-shot allreduce or a zero-copy allgather would take two."""
    F = mop.MPI_FLOAT
    count, ag = 256, 8192
    B = FUSED // n - 5
    checks = []
    staged = comm.get_param("alltoall_staged") + comm.get_param("alltoall_landing")
    fused0, epoch0 = comm.get_param("alltoall_fused"), comm.get_param("epoch")
    for it in range(64):
        kind = it % 4
        if kind == 0:
            x = Xfer(rank, n, uniform(n, B), seed=200 + it, roff=it % 3)
            checks.append(x)
        elif kind == 3:
            x = Xfer(rank, n, sym_matrix(n, B, 300 + it), seed=300 + it, gap=2)
            checks.append(x)
        elif kind == 1:  # exact values k * 2^-8: the sum does not depend on the order
            xs = [(np.random.default_rng(1000 * it + r).integers(-1024, 1025, count) * 2.0 ** -8)
                  .astype(np.float32) for r in range(n)]
            s = torch.from_numpy(xs[rank]).cuda()
            out = torch.zeros_like(s)
            checks.append((out, np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)))
            x = (s, out)
        else:
            blocks = [np.random.default_rng(5000 * it + r).integers(0, 256, ag).astype(np.uint8)
                      for r in range(n)]
            s = torch.from_numpy(blocks[rank]).cuda()
            out = torch.zeros(ag * n, dtype=torch.uint8, device="cuda")
            checks.append((out, np.concatenate(blocks)))
            x = (s, out)
        checks[-1] = (kind, x, checks[-1])
    torch.cuda.synchronize()  # every input is in place; from here on no host sync
    for kind, x, _ in checks:
        if kind == 0:
            comm.alltoall(x.s, x.rbuf.ptr, B)
        elif kind == 3:
            comm.alltoallv(*x.v_args())
        elif kind == 1:
            comm.allreduce(x[0], x[1], count, F, mop.MPI_SUM)
        else:
            comm.allgather(x[0], x[1], ag)
    torch.cuda.synchronize()
    if comm.error():
        return False, f"device error {comm.error()}"
    if comm.get_param("alltoall_staged") + comm.get_param("alltoall_landing") != staged:
        return False, "an alltoall of the sequence did not take the fused kernel"
    if comm.get_param("alltoall_fused") - fused0 != 32:
        return False, f"{comm.get_param('alltoall_fused') - fused0} fused alltoalls, expected 32"
    if comm.get_param("epoch") - epoch0 != 64:
        return False, (f"the 64 calls took {comm.get_param('epoch') - epoch0} epochs: the allreduce "
                       "was not fused or the allgather not staged")
    for it, (kind, x, chk) in enumerate(checks):
        if kind in (0, 3):
            ok, msg = chk.check()
        else:
            got = chk[0].cpu().numpy()
            ok, msg = np.array_equal(got.view(np.uint8), chk[1].view(np.uint8)), "result differs"
        if not ok:
            return False, f"call {it} (kind {kind}): {msg}"
    return True, ""


def case_nonblocking(comm, rank, n):
    """ialltoall / ialltoallv four deep, waited in reverse order."""
    sizes = path_sizes(n)
    xs, reqs = [], []
    for k in range(4):
        B = sizes[k % 3]
        a = Xfer(rank, n, uniform(n, B), seed=400 + k, roff=k)
        xs.append(a)
        reqs.append(comm.ialltoall(a.s, a.rbuf.ptr, B))
        b = Xfer(rank, n, sym_matrix(n, sizes[(k + 1) % 3], 410 + k), seed=410 + k, gap=k)
        xs.append(b)
        reqs.append(comm.ialltoallv(*b.v_args()))
    for r in reversed(reqs):
        r.wait()
    for r in reqs:
        r.free()
    for k, x in enumerate(xs):
        ok, msg = x.check()
        if not ok:
            return False, f"request {k}: {msg}"
    return True, ""


def case_no_rendezvous(comm, rank, n):
    """ialltoall and a plan start at a landing size make no host rendezvous
    once the landing buffer is there (get_param boot_calls)."""
    B = path_sizes(n)[2]
    x = Xfer(rank, n, uniform(n, B), seed=500)
    ok, msg = run(comm, x, "ialltoall", B)  # grows the landing buffer if nobody has
    if not ok:
        return False, "warm-up: " + msg
    y = Xfer(rank, n, uniform(n, B), seed=501)
    before, pb = comm.get_param("boot_calls"), paths(comm)
    ok, msg = run(comm, y, "ialltoall", B)
    if ok:
        ok, msg = took(comm, pb, 2)
    if ok and comm.get_param("boot_calls") != before:
        ok, msg = False, f"ialltoall made {comm.get_param('boot_calls') - before} host rendezvous"
    if not ok:
        return False, "ialltoall: " + msg
    for v in (False, True):
        z = Xfer(rank, n, sym_matrix(n, B, 510) if v else uniform(n, B), seed=510)
        plan = comm.alltoallv_init(*z.v_args()) if v else comm.alltoall_init(z.s, z.rbuf.ptr, B)
        before, pb = comm.get_param("boot_calls"), paths(comm)
        plan.start()
        plan.wait()
        after = comm.get_param("boot_calls")
        ok, msg = z.check()
        if ok:
            ok, msg = took(comm, pb, 2)
        plan.free()
        if ok and after != before:
            ok, msg = False, f"the start made {after - before} host rendezvous"
        if not ok:
            return False, f"plan start ({'alltoallv' if v else 'alltoall'}): {msg}"
    return True, ""


def case_persistent(comm, rank, n):
    """alltoall_init / alltoallv_init started three times, the input changed
    between the starts; on each path."""
    for path, B in enumerate(path_sizes(n)):
        for v in (False, True):
            x = Xfer(rank, n, sym_matrix(n, B, 600 + path) if v else uniform(n, B), seed=600,
                     gap=3 if v else 0)
            plan = comm.alltoallv_init(*x.v_args()) if v else comm.alltoall_init(x.s, x.rbuf.ptr, B)
            if plan.kind != 4:
                return False, f"plan kind {plan.kind}"
            for start in range(3):
                x.refill(610 + 10 * path + start)
                torch.cuda.synchronize()
                plan.start()
                plan.wait()
                ok, msg = x.check()
                if not ok:
                    plan.free()
                    return False, f"{'alltoallv' if v else 'alltoall'} plan, path {path}, start {start}: {msg}"
            plan.free()
    return True, ""


def case_wait(comm, rank, n):
    """alltoall_wait: the fused kernel's own completion mark, then a staged size."""
    for k, B in enumerate((8, FUSED // n, 5003, 16)):
        x = Xfer(rank, n, uniform(n, B), seed=700 + k)
        torch.cuda.synchronize()
        comm.alltoall_wait(x.s, x.rbuf.ptr, B)
        ok, msg = x.check()  # no stream sync before it: the wait is the completion
        if not ok:
            return False, f"B={B}: {msg}"
    return True, ""


CASES = [("sizes", case_sizes), ("misaligned", case_misaligned), ("inplace", case_inplace),
         ("alltoallv_variants", case_v_variants), ("reuse", case_reuse),
         ("nonblocking", case_nonblocking), ("no_rendezvous", case_no_rendezvous),
         ("persistent", case_persistent), ("wait", case_wait)]


def report(rank, n, obj):
    line = json.dumps(obj)
    print(line, flush=True)
    d = os.environ.get("COLL_LOG_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"alltoall_n{n}_rank{rank}.jsonl"), "a") as f:
            f.write(line + "\n")


def main():
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = int(os.environ.get("OMPI_AMD_DEVICE", "0"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lost signal is an error line, not a kill
    comm.set_param("fused_bytes", FUSED)
    comm.set_param("small_bytes", SMALL)
    ok_all = True
    for name, fn in CASES:
        t0 = time.time()
        try:
            ok, msg = fn(comm, rank, n)
        except Exception as e:  # noqa: BLE001 — a library error is the case's failure
            ok, msg = False, f"{type(e).__name__}: {e}"
        report(rank, n, {"rank": rank, "case": name, "ok": bool(ok), "msg": msg,
                         "s": round(time.time() - t0, 3)})
        ok_all = ok_all and ok
        if comm.error():  # the communicator is unusable after a device error
            break
    if not comm.error():
        comm.free()
    dist.destroy_process_group()
    sys.exit(0 if ok_all else 1)


if __name__ == "__main__":
    main()
