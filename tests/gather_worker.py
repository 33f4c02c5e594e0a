"""One rank of the allgatherv / gather(v) / scatter(v) test (tests/test_gather_gpu.py).

Launched N times like tests/alltoall_worker.py.  A source is filled with a
pattern that is a function of (rank, byte index); every rank computes the
rbuf it must end up with from that formula alone (nothing is exchanged, no
oracle) and compares the whole buffer byte for byte: the 64 sentinel bytes on
each side and the prefill of every byte no block covers included.  A rank
that receives nothing (the non-roots of a gather) passes a buffer all the
same and must find it untouched.  The three paths are reached with small data
by setting fused_bytes / small_bytes (and alltoall_chunk for passes).  Prints
one JSON line per case; exits 0 only if all passed.
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

FUSED, SMALL = 4096, 65536     # the thresholds outside a forced path
BIG = 1 << 22
PREFILL, SENTINEL = 0x5A, 0xA5
KINDS = ("allgatherv", "gather", "gatherv", "scatter", "scatterv")
GATHERISH = ("allgatherv", "gather", "gatherv")
SIZES = (0, 1, 15, 16, 17, 255, 4095, 4097, 70001)


def pat(r, seed, nbytes):
    """Bytes [0, nbytes) of rank r's source."""
    i = np.arange(nbytes, dtype=np.int64)
    return ((r * 131 + i * 7 + (i >> 8) * 13 + seed * 17 + 3) & 0xFF).astype(np.uint8)


class Buf:
    """`nbytes` of device memory starting `off` bytes past a 256-B boundary,
    with 64 sentinel bytes on each side."""

    def __init__(self, host: np.ndarray, off: int):
        n = host.size
        self.t = torch.empty(n + 1024, dtype=torch.uint8, device="cuda")
        self.lo = (-self.t.data_ptr()) % 256 + 256 + off
        self.n = n
        self.ptr = self.t.data_ptr() + self.lo
        self.set(host)

    def set(self, host: np.ndarray):
        img = np.full(self.n + 128, SENTINEL, dtype=np.uint8)
        img[64:64 + self.n] = host
        self.want = img
        self.t[self.lo - 64:self.lo + self.n + 64].copy_(torch.from_numpy(img))

    def expect(self, host: np.ndarray):
        self.want = np.full(self.n + 128, SENTINEL, dtype=np.uint8)
        self.want[64:64 + self.n] = host

    def check(self, what):
        got = self.t[self.lo - 64:self.lo + self.n + 64].cpu().numpy()
        if np.array_equal(got, self.want):
            return True, ""
        bad = np.flatnonzero(got != self.want)
        return False, (f"{what}: {bad.size}/{got.size} bytes differ, first at {int(bad[0]) - 64} "
                       f"(got {int(got[bad[0]])} want {int(self.want[bad[0]])}), last at "
                       f"{int(bad[-1]) - 64}")


def contiguous(counts):
    d, at = [], 0
    for c in counts:
        d.append(at)
        at += c
    return d


class Call:
    """One of the five collectives: buffers, arguments and expectation.

    counts / displs describe the gathered layout (allgatherv, gather(v): the
    receive side; scatter(v): the root's send side).  inplace: MPI_IN_PLACE
    where the collective takes it; alias: allgatherv's sbuf == rbuf +
    rdispls[rank] spelling."""

    def __init__(self, comm, kind, counts, displs=None, root=0, seed=0, inplace=False, alias=False,
                 soff=0, roff=0, tail=16):
        self.comm, self.kind, self.root, self.seed = comm, kind, root, seed
        self.rank, self.n = comm.rank, comm.size
        self.c = [int(v) for v in counts]
        self.d = contiguous(self.c) if displs is None else [int(v) for v in displs]
        self.total = max([d + c for d, c in zip(self.d, self.c)] + [0]) + tail
        self.gatherish = kind in GATHERISH
        self.at_root = kind == "allgatherv" or self.rank == root
        self.inplace = (inplace or alias) and self.at_root
        self.alias = alias
        me = self.rank
        if self.gatherish:
            self.rbuf = Buf(self.gathered(initial=True), roff)
            self.sbuf = None if self.inplace else Buf(pat(me, seed, self.c[me]), soff)
            self.rbuf.expect(self.gathered(initial=False))
        else:
            self.sbuf = Buf(pat(root, seed, self.total), soff) if self.at_root else None
            self.rbuf = None if self.inplace else Buf(np.full(self.c[me] + tail, PREFILL, np.uint8), roff)
            if self.rbuf:
                self.rbuf.expect(self.scattered())

    def gathered(self, initial):
        img = np.full(self.total, PREFILL, dtype=np.uint8)
        for p in range(self.n):
            if (initial and not (self.inplace and p == self.rank)) or (not initial and not self.at_root):
                continue
            img[self.d[p]:self.d[p] + self.c[p]] = pat(p, self.seed, self.c[p])
        return img

    def scattered(self):
        me = self.rank
        img = np.full(self.rbuf.n, PREFILL, dtype=np.uint8)
        img[:self.c[me]] = pat(self.root, self.seed, self.total)[self.d[me]:self.d[me] + self.c[me]]
        return img

    def refill(self, seed):
        """New input (and expectation) in the same buffers: persistent starts."""
        self.seed = seed
        if self.gatherish:
            self.rbuf.set(self.gathered(initial=True))
            if self.sbuf:
                self.sbuf.set(pat(self.rank, seed, self.c[self.rank]))
            self.rbuf.expect(self.gathered(initial=False))
        else:
            if self.sbuf:
                self.sbuf.set(pat(self.root, seed, self.total))
            if self.rbuf:
                self.rbuf.set(np.full(self.rbuf.n, PREFILL, np.uint8))
                self.rbuf.expect(self.scattered())

    def args(self):
        me, root, k = self.rank, self.root, self.kind
        sig = self.c if self.at_root else None   # "significant only at root"
        sigd = self.d if self.at_root else None
        if self.gatherish:
            s = self.sbuf.ptr if self.sbuf else coll.IN_PLACE
            if self.alias and k == "allgatherv":
                s = self.rbuf.ptr + self.d[me]
            if k == "allgatherv":
                return (s, self.c[me], self.rbuf.ptr, self.c, self.d)
            if k == "gather":
                return (s, self.rbuf.ptr, self.c[me], root)
            return (s, self.c[me], self.rbuf.ptr, sig, sigd, root)
        s = self.sbuf.ptr if self.sbuf else None
        r = self.rbuf.ptr if self.rbuf else coll.IN_PLACE
        if k == "scatter":
            return (s, r, self.c[me], root)
        return (s, sig, sigd, r, self.c[me], root)

    def blocking(self, stream_sync=True):
        getattr(self.comm, self.kind)(*self.args(), blocking=stream_sync)

    def post(self):
        return getattr(self.comm, "i" + self.kind)(*self.args())

    def init(self):
        return getattr(self.comm, self.kind + "_init")(*self.args())

    def run(self, form="blocking"):
        if form == "blocking":
            self.blocking()
        else:
            r = self.post()
            r.wait()
            r.free()
        return self.check()

    def check(self):
        what = f"{self.kind} root {self.root} counts {self.c[:4]}.."
        for name, b in (("rbuf", self.rbuf), ("sbuf", self.sbuf)):
            if b is not None:
                ok, msg = b.check(f"{what} {name}")  # a source must come back unchanged
                if not ok:
                    return ok, msg
        return True, ""


def roots(kind, n):
    return [0] if kind == "allgatherv" else list(range(n))


def force(comm, path):
    """Every size from here on takes `path` (0 fused, 1 staged, 2 landing);
    None: the worker's usual thresholds."""
    comm.set_param("fused_bytes", {None: FUSED, 0: BIG}.get(path, 0))
    comm.set_param("small_bytes", {None: SMALL, 2: 0}.get(path, BIG))


def paths(comm):
    return tuple(comm.get_param(k) for k in ("gather_fused", "gather_staged", "gather_landing"))


def a2a_paths(comm):
    return tuple(comm.get_param(k) for k in ("alltoall_fused", "alltoall_staged", "alltoall_landing"))


def took(comm, before, which):
    """The one call since `before` ran on path `which`; None: on none (zero bytes)."""
    d = [a - b for a, b in zip(paths(comm), before)]
    want = [0, 0, 0]
    if which is not None:
        want[which] = 1
    return (d == want), f"gather path counters moved by {d}, expected {want}"


def path_sizes(n):
    """A size on each path under the usual thresholds (none a multiple of 16)."""
    return (FUSED // n - 3, 5003, SMALL + 4001)


def case_sizes(comm, rank, n):
    a2a0 = a2a_paths(comm)
    try:
        for path in range(3):
            force(comm, path)
            for B in SIZES:
                for kind in KINDS:
                    for root in roots(kind, n):
                        x = Call(comm, kind, [B] * n, root=root, seed=B + root + path)
                        before = paths(comm)
                        ok, msg = x.run()
                        if ok:
                            ok, msg = took(comm, before, path if B else None)
                        if not ok:
                            return False, f"path {path} B={B}: {msg}"
        # the landing path in passes: 70001 B in chunks of 1024 -> 69 passes
        comm.set_param("alltoall_chunk", 1024)
        for kind in KINDS:
            x = Call(comm, kind, [70001] * n, root=n - 1, seed=77)
            p0 = comm.get_param("gather_passes")
            ok, msg = x.run()
            grew = comm.get_param("gather_passes") - p0
            if ok and grew != -(-70001 // 1024):
                ok, msg = False, f"gather_passes grew by {grew}, expected {-(-70001 // 1024)}"
            if not ok:
                return False, f"{kind} in passes: {msg}"
    finally:
        comm.set_param("alltoall_chunk", 0)
        force(comm, None)
    if a2a_paths(comm) != a2a0:
        return False, "the alltoall's counters moved"
    return True, ""


def ragged_layout(counts, odd):
    """Displacements out of rank order (descending) with gaps: every offset a
    multiple of 16, or every offset odd."""
    d, at = [0] * len(counts), 16
    for p in range(len(counts) - 1, -1, -1):
        at = (at + 15) & ~15
        d[p] = at + 1 if odd else at
        at = d[p] + counts[p] + 7
    return d


def case_ragged(comm, rank, n):
    counts = [(r * 37 + 5) % 211 for r in range(n)]
    counts[1 % n] = 0
    if n >= 4:
        counts[n - 1] = 0
    try:
        for path in range(3):
            force(comm, path)
            for odd, offs in ((False, ((0, 0),)), (True, ((1, 1), (8, 13), (13, 8)))):
                d = ragged_layout(counts, odd)
                for soff, roff in offs:
                    for kind in ("allgatherv", "gatherv", "scatterv"):
                        for root in sorted({0, n - 1}) if kind != "allgatherv" else [0]:
                            for form in ("blocking", "post"):
                                x = Call(comm, kind, counts, d, root=root, seed=path + soff, soff=soff,
                                         roff=roff)
                                before = paths(comm)
                                ok, msg = x.run(form)
                                if ok:
                                    ok, msg = took(comm, before, path)
                                if not ok:
                                    return False, f"path {path} odd={odd} offsets ({soff},{roff}) {form}: {msg}"
    finally:
        force(comm, None)
    return True, ""


def case_inplace(comm, rank, n):
    B = 1003
    counts = [B + 16 * p for p in range(n)]
    try:
        for path in range(3):
            force(comm, path)
            for kind in KINDS:
                for root in sorted({path % n, n - 1}) if kind != "allgatherv" else [0]:
                    for alias in ((False, True) if kind == "allgatherv" else (False,)):
                        for form in ("blocking", "post"):
                            cs = [B] * n if kind in ("gather", "scatter") else counts
                            x = Call(comm, kind, cs, root=root, seed=30 + path, inplace=True, alias=alias,
                                     roff=4 * path)
                            before = paths(comm)
                            ok, msg = x.run(form)
                            if ok:
                                ok, msg = took(comm, before, path)
                            if not ok:
                                return False, f"path {path} alias={alias} {form}: {msg}"
    finally:
        force(comm, None)
    return True, ""


def case_reuse(comm, rank, n):
    """64 fused calls back to back on one stream with no host sync: the five
    collectives with changing roots, a fused allreduce and a fused alltoall in
    turn — the scratch halves and the flag rows they share.  Everything is
    checked at the end.  The allreduce's inputs are the exact values k * 2^-8
    (every summation order gives the same bits).  That every call was fused
    is asserted: by the path counters, and by the communicator's epoch — a
    fused kernel takes one epoch, every other path more."""
    F = mop.MPI_FLOAT
    count = 256
    B = FUSED // n - 5
    fused0, a2a0, epoch0 = paths(comm), a2a_paths(comm), comm.get_param("epoch")
    calls, ngather = [], 0
    for it in range(64):
        kind = it % 7
        if kind < 5:
            cs = [B - 3 * ((p + it) % 5) for p in range(n)]
            if KINDS[kind] in ("gather", "scatter"):
                cs = [B] * n
            calls.append(("x", Call(comm, KINDS[kind], cs, root=it % n, seed=200 + it, roff=it % 3), None))
            ngather += 1
        elif kind == 5:
            xs = [(np.random.default_rng(1000 * it + r).integers(-1024, 1025, count) * 2.0 ** -8)
                  .astype(np.float32) for r in range(n)]
            s = torch.from_numpy(xs[rank]).cuda()
            calls.append(("ar", (s, torch.zeros_like(s)),
                          np.sum(np.stack(xs).astype(np.float64), axis=0).astype(np.float32)))
        else:
            src = np.concatenate([pat(rank, it + q, B) for q in range(n)])
            want = np.concatenate([pat(p, it + rank, B) for p in range(n)])
            calls.append(("a2a", (torch.from_numpy(src).cuda(),
                                  torch.zeros(B * n, dtype=torch.uint8, device="cuda")), want))
    torch.cuda.synchronize()  # every input is in place; from here on no host sync
    for what, x, _ in calls:
        if what == "x":
            x.blocking(stream_sync=False)
        elif what == "ar":
            comm.allreduce(x[0], x[1], count, F, mop.MPI_SUM)
        else:
            comm.alltoall(x[0], x[1], B)
    torch.cuda.synchronize()
    if comm.error():
        return False, f"device error {comm.error()}"
    moved = [a - b for a, b in zip(paths(comm), fused0)]
    if moved != [ngather, 0, 0]:
        return False, f"gather path counters moved by {moved}, expected {[ngather, 0, 0]}"
    moved = [a - b for a, b in zip(a2a_paths(comm), a2a0)]
    if moved != [64 // 7, 0, 0]:
        return False, f"alltoall path counters moved by {moved}"
    if comm.get_param("epoch") - epoch0 != 64:
        return False, f"the 64 calls took {comm.get_param('epoch') - epoch0} epochs: one was not fused"
    for it, (what, x, want) in enumerate(calls):
        if what == "x":
            ok, msg = x.check()
        else:
            ok, msg = np.array_equal(x[1].cpu().numpy().view(np.uint8), want.view(np.uint8)), "result differs"
        if not ok:
            return False, f"call {it} ({what}): {msg}"
    return True, ""


def case_nonblocking(comm, rank, n):
    """Four requests outstanding, mixed over the five collectives and the
    three paths, waited in reverse order; then igatherv / iscatterv completed
    by polling test()."""
    sizes = path_sizes(n)
    for rnd, kinds in enumerate((("allgatherv", "gather", "scatter", "gatherv"),
                                 ("scatterv", "gatherv", "allgatherv", "scatter"))):
        xs = []
        for k, kind in enumerate(kinds):
            B = sizes[(k + rnd) % 3]
            cs = [B] * n if kind in ("gather", "scatter") else [max(0, B - 11 * p) for p in range(n)]
            xs.append(Call(comm, kind, cs, root=(k + rnd) % n, seed=400 + 10 * rnd + k, roff=k))
        reqs = [x.post() for x in xs]
        for r in reversed(reqs):
            r.wait()
        for r in reqs:
            r.free()
        for k, x in enumerate(xs):
            ok, msg = x.check()
            if not ok:
                return False, f"round {rnd} request {k}: {msg}"
    for path, B in enumerate(sizes):
        xs = [Call(comm, kind, [max(0, B - 5 * p) for p in range(n)], root=(path + 1) % n, seed=450 + path)
              for kind in ("gatherv", "scatterv")]
        reqs = [x.post() for x in xs]
        deadline = time.time() + 60
        for r in reqs:
            while not r.test():
                if time.time() > deadline:
                    return False, f"path {path}: test() never completed"
        for r in reqs:
            r.free()
        for x in xs:
            ok, msg = x.check()
            if not ok:
                return False, f"polled, path {path}: {msg}"
    return True, ""


def case_no_rendezvous(comm, rank, n):
    """allgatherv, gather and scatter know the call's largest pair locally:
    boot_calls stands still across their blocking fused / staged calls, their
    i* forms on every path (once the landing buffer has grown) and every plan
    start of all five.  gatherv / scatterv agree on it: boot_calls rises
    across the blocking call and once at their init."""
    sizes = path_sizes(n)
    boot = lambda: comm.get_param("boot_calls")  # noqa: E731
    # the landing buffer, grown by a blocking call of the largest size used here
    ok, msg = Call(comm, "allgatherv", [sizes[2]] * n, seed=500).run()
    if not ok:
        return False, "warm-up: " + msg
    for kind in ("allgatherv", "gather", "scatter"):
        for path, B in enumerate(sizes):
            for form in ("blocking", "post"):
                if form == "blocking" and path == 2:
                    continue
                x = Call(comm, kind, [B] * n, root=path % n, seed=510 + path)
                b0, p0 = boot(), paths(comm)
                ok, msg = x.run(form)
                if ok:
                    ok, msg = took(comm, p0, path)
                if ok and boot() != b0:
                    ok, msg = False, f"{boot() - b0} host rendezvous"
                if not ok:
                    return False, f"{kind} {form} path {path}: {msg}"
    for kind in KINDS:
        agrees = kind in ("gatherv", "scatterv")
        for path, B in enumerate(sizes):
            x = Call(comm, kind, [B] * n, root=(path + 1) % n, seed=520 + path)
            b0 = boot()
            plan = x.init()
            rose = boot() - b0
            if rose != (1 if agrees else 0):
                plan.free()
                return False, f"{kind}_init made {rose} host rendezvous"
            for start in range(2):
                x.refill(530 + start)
                torch.cuda.synchronize()
                b0, p0 = boot(), paths(comm)
                plan.start()
                plan.wait()
                after = boot()
                ok, msg = x.check()
                if ok:
                    ok, msg = took(comm, p0, path)
                if ok and after != b0:
                    ok, msg = False, f"the start made {after - b0} host rendezvous"
                if not ok:
                    plan.free()
                    return False, f"{kind} plan path {path} start {start}: {msg}"
            plan.free()
        if agrees:
            x = Call(comm, kind, [sizes[0]] * n, root=0, seed=540)
            b0 = boot()
            ok, msg = x.run()
            if ok and boot() <= b0:
                ok, msg = False, "the blocking call made no host rendezvous"
            if not ok:
                return False, f"{kind} blocking: {msg}"
    return True, ""


def case_persistent(comm, rank, n):
    """Each _init started three times, the source changed between the starts;
    on each path; the plan kind is 4."""
    for path, B in enumerate(path_sizes(n)):
        for kind in KINDS:
            cs = [B] * n if kind in ("gather", "scatter") else [max(0, B - 9 * p) for p in range(n)]
            x = Call(comm, kind, cs, root=(path + 2) % n, seed=600, inplace=(kind == "gather" and path == 1))
            plan = x.init()
            if plan.kind != 4:
                plan.free()
                return False, f"plan kind {plan.kind}"
            for start in range(3):
                x.refill(610 + 10 * path + start)
                torch.cuda.synchronize()
                plan.start()
                plan.wait()
                ok, msg = x.check()
                if not ok:
                    plan.free()
                    return False, f"{kind} plan, path {path}, start {start}: {msg}"
            plan.free()
    return True, ""


def case_args(comm, rank, n):
    """Arguments significant only at the root may be NULL elsewhere (every
    non-root passes None here), and zero-byte calls take NULL buffers.  The
    BAD_PARAM list runs at N = 1 (tests/test_gather_gpu.py)."""
    root = n - 1
    B = 777
    x = Call(comm, "gather", [B] * n, root=root, seed=700)
    y = Call(comm, "gatherv", [B + p for p in range(n)], root=root, seed=701)
    z = Call(comm, "scatter", [B] * n, root=root, seed=702)
    w = Call(comm, "scatterv", [B + p for p in range(n)], root=root, seed=703)
    at_root = rank == root
    for form in (0, 1, 2):
        def go(name, *a):
            fn = getattr(comm, ("", "i", "")[form] + name + ("", "", "_init")[form])
            h = fn(*a) if form else fn(*a, blocking=True)
            if form == 2:
                h.start()
            if form:
                h.wait()
                h.free()
        for c in (x, y, z, w):
            c.refill(710 + form)
        torch.cuda.synchronize()
        go("gather", x.sbuf.ptr, x.rbuf.ptr if at_root else None, B, root)
        go("gatherv", y.sbuf.ptr, y.c[rank], y.rbuf.ptr if at_root else None, y.c if at_root else None,
           y.d if at_root else None, root)
        go("scatter", z.sbuf.ptr if at_root else None, z.rbuf.ptr, B, root)
        go("scatterv", w.sbuf.ptr if at_root else None, w.c if at_root else None,
           w.d if at_root else None, w.rbuf.ptr, w.c[rank], root)
        for c in (x, y, z, w):
            ok, msg = c.check()
            if not ok:
                return False, f"form {form}: {msg}"
        zero = [0] * n
        before = paths(comm)
        go("allgatherv", None, 0, None, zero, zero)
        go("gather", None, None, 0, root)
        go("scatter", None, None, 0, root)
        go("gatherv", None, 0, None, zero if at_root else None, zero if at_root else None, root)
        go("scatterv", None, zero if at_root else None, zero if at_root else None, None, 0, root)
        if paths(comm) != before:
            return False, "a zero-byte call took a path"
    return True, ""


CASES = [("sizes", case_sizes), ("ragged", case_ragged), ("inplace", case_inplace), ("reuse", case_reuse),
         ("nonblocking", case_nonblocking), ("no_rendezvous", case_no_rendezvous),
         ("persistent", case_persistent), ("args", case_args)]


def report(rank, n, obj):
    line = json.dumps(obj)
    print(line, flush=True)
    d = os.environ.get("COLL_LOG_DIR")
    if d:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, f"gather_n{n}_rank{rank}.jsonl"), "a") as f:
            f.write(line + "\n")


def main():
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    device = int(os.environ.get("OMPI_AMD_DEVICE", "0"))
    torch.cuda.set_device(device)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=device)
    comm.set_param("timeout_ms", 10000)  # a lost signal is an error line, not a kill
    force(comm, None)
    only = set(filter(None, os.environ.get("GATHER_CASES", "").split(",")))
    ok_all = True
    for name, fn in CASES:
        if only and name not in only:
            continue
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
