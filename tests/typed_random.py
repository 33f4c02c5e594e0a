"""Generated calls of the typed exchange collectives (numpy only, no GPU).

A Case is one full N-rank call of ompi_amd_<kind>_typed: every rank's send
and receive datatype, the packed bytes of every pair, the element
displacements, the buffer origins and offsets, the seeded images and the
receive image each rank must end up with (oracle.pack through the SENDER's
type, oracle.unpack through the receiver's).  Everything follows from the
seed, so every rank of a multi-rank test rebuilds the same Case.

Datatypes come from ddt_random.rand_layout / rand_type and from a small
directed pool (directed_pool) that holds what those two do not draw: every
granule 1..16 as the datatype's own, a 2-B granule, more than eight elements
(device find_elem's binary search), a zero extent and an extent smaller than a
run (send only), one run cut by every 16-B slice boundary.

tests/test_typed_fuzz_cpu.py proves the generator's properties,
tests/test_typed_fuzz_gpu.py runs single_case() at N = 1 and
tests/typed_worker.py runs worker_case() at N = 2, 3, 4, 8.
"""
import math

import numpy as np

from ddt_random import LAYOUT_CLASSES, rand_layout, rand_type, run_bounds, typed_bounds
from ompi_amd import datatype as dd

KINDS = ("alltoall", "alltoallv", "allgatherv", "gather", "gatherv", "scatter", "scatterv")
UNIFORM = ("alltoall", "gather", "scatter")   # the API fixes displacement p * count * extent
ROOTED = ("gather", "gatherv", "scatter", "scatterv")
GUARD = 64
MAX_LCM = 64 << 10       # packed bytes of the unit of a pair (or of a group of pairs)
MAX_SIZE = 16 << 10      # packed bytes of one element of a drawn type
GS = (1, 2, 4, 8, 16)
OFFSETS = {1: (1, 3, 7), 2: (2, 6, 10), 4: (4, 12), 8: (8,), 16: (0,)}   # address mod 16 -> that G


# ---- a side without a datatype is bytes --------------------------------------
def size_of(t):
    return 1 if t is None else t.size


def ext_of(t):
    return 1 if t is None else t.extent


def runs_of(t):
    return [(0, 1)] if t is None else t.runs


def bounds_of(t, count):
    """[lo, hi) of the typed bytes of `count` elements, relative to the block's base."""
    if count == 0:
        return 0, 0
    return (0, count) if t is None else typed_bounds(t, count)


def pow2(v):
    g = 16
    while g > 1 and v % g:
        g >>= 1
    return g


def gran_of(t):
    """ddt_view.gran: the power of two (<= 16) dividing the extent and every
    run length, displacement and stride of the element table."""
    if t is None:
        return 16
    v = abs(t.extent)
    for c, bl, st, d in t.elems:
        v |= bl | abs(d) | (abs(st) if c > 1 else bl)
    return pow2(v)


# ---- the engine's integer rules, restated (coll_typed.h, coll_kernels.h) ------
def typed_granule(gran, typed_addr, contig_addr):
    return pow2(gran | typed_addr | contig_addr)


def a2a_slice(b, g, G):
    per = ((b + G - 1) // G + 15) & ~15
    return min(per * g, b), min(per * (g + 1), b)


def copy_blocks(most, max_blocks=1024, jobs=1):
    """launch_typed_copy's grid.x: 16 KiB per workgroup."""
    return max(1, min((most // 16 + 1023) // 1024, max(1, max_blocks // jobs)))


TRIP = 256 * 8           # granules per trip of typed_walk: kXferThreads * kDdtUnroll


# ---- the directed pool ---------------------------------------------------------
def _blk(w):
    return dd.Datatype(f"b{w}", [(1, w, w, 0)], 0, w, min(w, 8))


_POOL = None


def directed_pool():
    """name -> (class, datatype).  For every granule g: `unit` (one g-byte run,
    size g), `tri` (runs g and 2g, size 3g), `run` (one 3g-byte run: a 16-B cut
    falls inside it), `neg` (negative stride, below the origin), `many` (eleven
    elements)."""
    global _POOL
    if _POOL is not None:
        return _POOL
    f = dd.from_runs
    i32, f64, i16 = (dd.predefined(k) for k in ("MPI_INT", "MPI_DOUBLE", "MPI_SHORT"))
    P = {}
    for g in GS:
        P[f"unit{g}"] = ("unit", f(f"unit{g}", [(0, g)], 3 * g))
        P[f"tri{g}"] = ("tri", f(f"tri{g}", [(0, g), (2 * g, 2 * g)], 5 * g))
        P[f"run{g}"] = ("run", f(f"run{g}", [(0, 3 * g)], 5 * g))
        neg = dd.type_vector(4, 1, -3, _blk(g))
        neg.name = f"neg{g}"
        P[neg.name] = ("negstride", neg)
        runs, at = [], 0
        for k in range(11):   # neighbours differ in length and do not touch: nothing folds
            n = g * (k % 3 + 1)
            runs.append((at, n))
            at += n + g
        P[f"many{g}"] = ("many", f(f"many{g}", runs, at))
    P["g2"] = ("g2", f("g2", [(0, 2), (6, 4)], 12))
    sv = dd.type_vector(5, 3, 7, i16)
    sv.name = "short_vec"
    P["short_vec"] = ("g2", sv)
    P["zero_extent"] = ("stacked", dd.type_create_resized(dd.type_vector(3, 2, 5, i32), 0, 0))
    P["sub_run_extent"] = ("stacked", dd.type_create_resized(f("r8", [(0, 8)], 8), 0, 4))
    P["wide"] = ("padded", dd.type_create_resized(dd.type_struct([1, 1], [0, 8], [i32, f64]), 0, 5000))
    for cls, t in P.values():
        t.max_count = None
    _POOL = P
    return P


class Stats:
    """Draws of datatypes and how many were thrown away (the lcm limit, a
    class the side may not use, a size past MAX_SIZE)."""

    def __init__(self):
        self.draws = self.rejected = 0


def legal(cls, t, side, uniform, max_span=None):
    """May `side` (0 send, 1 receive) of a call use t?  max_span: the most
    bytes one element may span or advance (many blocks of many ranks: the
    buffers stay small)."""
    if t.size == 0 or t.size > MAX_SIZE or t.extent < 0:   # `backward`: refused by the entry points
        return False
    if max_span and (t.extent > max_span or run_bounds(t)[1] - run_bounds(t)[0] > max_span):
        return False
    if side == 0:
        return True
    if cls == "stacked" or t.extent == 0:                  # overlapping instances: send only
        return False
    lo, hi = run_bounds(t)
    if t.max_count is None and hi - lo > t.extent:         # instances would overlap
        return False
    if uniform and hi - lo > t.extent:                     # count instances must fit count * extent
        return False
    return True


def draw_type(rng, side, stats, uniform=False, gran=None, cls_in=None, ok=None, source=None, pool=0.45,
              max_span=None):
    """(class, datatype) for `side`.  gran: from the directed pool, with that
    granule; cls_in: only those pool classes; source: a LAYOUT_CLASSES name or
    "nested" (rand_type), where the side may use it.  ok(t): a further condition of
    the caller (the lcm limit); a draw that fails one is counted and redrawn,
    from the pool (whose sizes pair with most others) more often than before.
    pool: the share of draws from the directed pool."""
    P = directed_pool()
    names = sorted(P)
    if gran is not None:
        names = [k for k in names if gran_of(P[k][1]) == gran and (cls_in is None or P[k][0] in cls_in)
                 and legal(P[k][0], P[k][1], side, uniform, max_span)]
    else:
        names = [k for k in names if legal(P[k][0], P[k][1], side, uniform, max_span)]
    if source in ("backward",) or (side == 1 and source == "stacked") or \
            (uniform and source == "interleaved") or \
            (source in P and not legal(P[source][0], P[source][1], side, uniform, max_span)):
        source = None
    for tries in range(400):
        if tries == 3:    # the class asked for does not pair with the other side's sizes
            source = None
        if tries:
            pool = max(pool, 0.9)
        stats.draws += 1
        r = rng.random()
        if source in P:
            cls, t = P[source]
        elif gran is not None or (source is None and r < pool):
            cls, t = P[names[int(rng.integers(len(names)))]]
        elif source in LAYOUT_CLASSES or (source is None and r < pool + 0.6 * (1 - pool)):
            cls, t = rand_layout(rng, source)
        else:
            cls, t = "nested", rand_type(rng, int(rng.integers(1, 3)))
            t.max_count = None
        if legal(cls, t, side, uniform, max_span) and (ok is None or ok(t)):
            return cls, t
        stats.rejected += 1
    raise RuntimeError("no legal datatype in 400 draws")


def place(t, counts, rng):
    """Element displacements of consecutive blocks of `counts` elements of t:
    typed ranges disjoint, one to two elements' worth of untouched bytes
    between them where the extent allows (a zero extent puts all at 0)."""
    ext, out, end, at = ext_of(t), [], None, 0
    for c in counts:
        if c and ext > 0:
            lo, hi = bounds_of(t, c)
            if end is None:   # a byte side starts on a 16-B boundary: the test's offsets pick G
                at = int(rng.integers(0, 3)) * (16 if t is None else 1)
            else:
                at = max(0, -((lo - end - 1) // ext)) + int(rng.integers(0, 2))
            end = at * ext + hi
        out.append(at if ext > 0 else 0)
    return out


def _groups(kind, n, root):
    """The sets of (side, rank) whose datatypes share one unit of packed bytes."""
    S, R = [(0, p) for p in range(n)], [(1, q) for q in range(n)]
    if kind == "alltoall":
        return [S + R]
    if kind == "allgatherv":
        return [[s] + R for s in S]
    if kind == "gather":
        return [S + [(1, root)]]
    if kind == "scatter":
        return [[(0, root)] + R]
    if kind == "alltoallv":
        return [[s, r] for s in S for r in R]
    if kind == "gatherv":
        return [[s, (1, root)] for s in S]
    return [[(0, root), r] for r in R]


class Case:
    """One generated call.  types: {(side, rank): (class, datatype or None)}
    fixes some or all datatypes; the rest are drawn per rank and side from
    default_rng([seed, rank, side]).  target: packed bytes aimed at per pair;
    rows: per-rank multipliers of the v kinds (a zero: that row moves
    nothing).  soff / roff: the buffer origin's address mod 256 per rank.
    source(side, rank): where that draw comes from (draw_type's `source`)."""

    def __init__(self, seed, n, kind, root=0, inplace=False, target=600, rows=None, types=None,
                 soff=None, roff=None, exact=None, max_lcm=MAX_LCM, stats=None, source=None,
                 max_span=None):
        assert kind in KINDS and (not inplace or kind in ("alltoall", "allgatherv"))
        self.seed, self.n, self.kind, self.root, self.inplace = seed, n, kind, root, inplace
        self._src = (None, None)
        self.stats = stats = stats or Stats()
        types = dict(types or {})
        rc = np.random.default_rng([seed, 0xC0])
        uniform = kind in UNIFORM
        groups = _groups(kind, n, root)
        T = {}

        def fits(key, t):
            T[key] = ("?", t)
            try:
                for g in groups:
                    if key in g:
                        sizes = [size_of(T[k][1]) for k in g if k in T]
                        L = math.lcm(*sizes)
                        if L > max_lcm:
                            return False
                        for k in g:   # an interleaved receive type holds at most max_count instances
                            tk = T.get(k, (0, None))[1]
                            if k[0] == 1 and tk is not None and getattr(tk, "max_count", None) \
                                    and L // tk.size > tk.max_count:
                                return False
                return True
            finally:
                del T[key]

        order = [(1, q) for q in range(n)] if inplace else \
            [(0, p) for p in range(n)] + [(1, q) for q in range(n)]
        for key in order:
            side, rank = key
            if key in types:
                T[key] = types[key]
                continue
            rng = np.random.default_rng([seed, rank, side])
            T[key] = draw_type(rng, 1 if inplace else side, stats, uniform=uniform and side == 1,
                               ok=lambda t, key=key: fits(key, t),
                               source=source(side, rank) if source else None,
                               max_span=max_span,
                               pool=0.45 if n <= 3 else 0.8)   # many ranks: one unit must suit them all
        if inplace:   # one buffer, one datatype per rank: it sends through what it receives through
            for q in range(n):
                T[(0, q)] = T[(1, q)]
        self.cls = {k: v[0] for k, v in T.items()}
        self.st = [T[(0, p)][1] for p in range(n)]
        self.rt = [T[(1, q)][1] for q in range(n)]

        # packed bytes per pair
        rows = list(rows) if rows is not None else [1] * n
        unit = {}
        for g in groups:
            L = math.lcm(*[size_of(T[k][1]) for k in g])
            cap = min([t.max_count * t.size // L for s, r in g if s == 1
                       for t in [T[(s, r)][1]] if t is not None and t.max_count] + [1 << 40])
            for s in g:
                for r in g:
                    if s[0] == 0 and r[0] == 1:
                        unit[(s[1], r[1])] = (L, cap)
        self.B = [[0] * n for _ in range(n)]
        for p in range(n):
            for q in range(n):
                if (p, q) not in unit:
                    continue
                L, cap = unit[(p, q)]
                row = 1 if uniform else rows[{"alltoallv": (p + q) % n, "scatterv": q}.get(kind, p)]
                k = exact if exact is not None else max(1, int(round(target / L)))
                self.B[p][q] = L * min(k * row, max(cap, 1 if row else 0))
        for p in range(n):
            for q in range(n):
                assert self.B[p][q] % size_of(self.st[p]) == 0 and self.B[p][q] % size_of(self.rt[q]) == 0
        self.sc = [[self.B[p][q] // size_of(self.st[p]) for q in range(n)] for p in range(n)]
        self.rc = [[self.B[p][q] // size_of(self.rt[q]) for p in range(n)] for q in range(n)]

        # element displacements
        self.sd, self.rd = [], []
        for p in range(n):
            if kind in ("alltoall", "scatter"):
                self.sd.append([q * max(self.sc[p]) for q in range(n)])
            elif kind in ("alltoallv", "scatterv"):
                self.sd.append(place(self.st[p], self.sc[p], rc))
            else:
                self.sd.append([0] * n)
        for q in range(n):
            if kind in ("alltoall", "gather"):
                self.rd.append([p * max(self.rc[q]) for p in range(n)])
            elif kind in ("alltoallv", "allgatherv", "gatherv"):
                self.rd.append(place(self.rt[q], self.rc[q], rc))
            else:
                self.rd.append([0] * n)
        if inplace:   # the block for q sits where q's block will land (allgatherv: the own block)
            self.sd = [[self.rd[p][p] if kind == "allgatherv" else self.rd[p][q] for q in range(n)]
                       for p in range(n)]
            if kind == "alltoall":   # rank p reads rc[p][q] elements for q: the same packed bytes
                assert all(self.rc[p][q] * size_of(self.rt[p]) == self.B[p][q] for p in range(n) for q in range(n))
        self.soff = [int(rc.choice([0, 0, 16, 1, 2, 4, 6, 8, 10])) for _ in range(n)] if soff is None else list(soff)
        self.roff = [int(rc.choice([0, 0, 16, 1, 2, 4, 6, 8, 10])) for _ in range(n)] if roff is None else list(roff)

    # -- who moves what --
    def sends(self, p):
        return self.kind not in ("scatter", "scatterv") or p == self.root

    def recvs(self, q):
        return self.kind not in ("gather", "gatherv") or q == self.root

    def blocks(self, side, r):
        """[(byte offset of the typed base, elements)] of rank r's buffer of `side`."""
        t = (self.st, self.rt)[side][r]
        d, c = ((self.sd, self.sc), (self.rd, self.rc))[side]
        return [(d[r][k] * ext_of(t), c[r][k]) for k in range(self.n) if c[r][k]]

    def ranges(self, side, r):
        """Typed byte ranges [lo, hi) of every block of that buffer, relative to its origin."""
        t = (self.st, self.rt)[side][r]
        return [(b + lo, b + hi) for b, c in self.blocks(side, r) for lo, hi in [bounds_of(t, c)]]

    def geometry(self, side, r):
        """(low, high): the buffer holds typed bytes [low, high) around the
        origin (low <= 0 < high) between two guards; the origin sits at
        index GUARD - low of the image."""
        rg = self.ranges(side, r)
        return min([lo for lo, _ in rg] + [0]), max([hi for _, hi in rg] + [1])

    def image_size(self, side, r):
        low, high = self.geometry(side, r)
        return high - low + 2 * GUARD

    def origin(self, side, r):
        return GUARD - self.geometry(side, r)[0]

    def _image(self, r, tag, epoch, size):
        """Seeded random bytes; past 65521 of them (a prime: no period a
        layout shares) the block repeats, which keeps large buffers cheap."""
        block = np.random.default_rng([self.seed, r, tag, epoch]).integers(0, 256, min(size, 65521), dtype=np.uint8)
        return np.resize(block, size)

    def send_image(self, p, epoch=0):
        """Rank p's whole source buffer (guards included), every byte random.
        In place it is p's receive buffer before the call."""
        if self.inplace:
            return self.prefill(p, epoch)
        return self._image(p, 0xD7, epoch, self.image_size(0, p))

    def prefill(self, q, epoch=0):
        return self._image(q, 0xF1, epoch, self.image_size(1, q))

    def packed(self, p, q, oracle, epoch=0):
        """The packed stream of pair p -> q."""
        side = 1 if self.inplace else 0
        if self._src[0] != (p, epoch):   # one sender's blocks come one after the other
            self._src = ((p, epoch), self.send_image(p, epoch))
        img, at = self._src[1], self.origin(side, p) + self.sd[p][q] * ext_of(self.st[p])
        out = oracle.pack(runs_of(self.st[p]), ext_of(self.st[p]), self.B[p][q] // size_of(self.st[p]),
                          img[at:], 0, self.B[p][q])
        assert out.size == self.B[p][q]
        return out

    def expected(self, q, oracle, epoch=0, recv_type_of=None):
        """Rank q's whole receive buffer after the call.  recv_type_of(p, q):
        a wrong receive datatype, for the CPU test of the inputs."""
        want = self.prefill(q, epoch)
        o, pad = self.origin(1, q), 0
        if recv_type_of is not None:   # a wrong layout may leave the buffer: room on both sides
            pad = 64 + sum(abs(x) for p in range(self.n) for t in [recv_type_of(p, q)]
                           for x in bounds_of(t, self.B[p][q] // size_of(t)))
            want = np.concatenate([np.zeros(pad, np.uint8), want, np.zeros(pad, np.uint8)])
        for p in range(self.n):
            if not self.B[p][q] or (self.inplace and p == q):
                continue
            t = self.rt[q] if recv_type_of is None else recv_type_of(p, q)
            oracle.unpack(runs_of(t), ext_of(t), self.B[p][q] // size_of(t), self.packed(p, q, oracle, epoch),
                          want[pad + o + self.rd[q][p] * ext_of(self.rt[q]):], 0)
        return want[pad:want.size - pad]

    def args(self, me, s, r):
        """The operands of comm.<kind>_typed on rank `me` (s, r: buffer origins)."""
        k, root = self.kind, self.root
        at_root = me == root
        ts = (self.st[me], self.rt[me])
        sc, sd, rc, rd = self.sc[me], self.sd[me], self.rc[me], self.rd[me]
        if k == "alltoall":
            return (s, r, sc[0], rc[0]) + ts
        if k == "alltoallv":
            return (s, sc, sd, r, rc, rd) + ts
        if k == "allgatherv":
            return (s, sc[0], r, rc, rd) + ts
        if k == "gather":
            return (s, r, sc[root], rc[root] if at_root else 0, root) + ts
        if k == "gatherv":
            return (s, sc[root], r, rc if at_root else None, rd if at_root else None, root) + ts
        if k == "scatter":
            return (s, r, sc[0] if at_root else 0, rc[root], root) + ts
        return (s, sc if at_root else None, sd if at_root else None, r, rc[root], root) + ts

    def side_granules(self, side, r, off=None):
        """The G of every block of that buffer when the contiguous end is 16-B
        aligned: the datatype's granule and the typed base's address."""
        t = (self.st, self.rt)[side][r]
        if t is None:
            return set()
        off = (self.soff, self.roff)[side][r] if off is None else off
        return {typed_granule(gran_of(t), (off + b) % 256 + 256, 0) for b, _ in self.blocks(side, r)}

    def what(self):
        names = lambda ts: ",".join("bytes" if t is None else t.name for t in ts)  # noqa: E731
        return (f"seed {self.seed} {self.kind} n {self.n} root {self.root}"
                f"{' in place' if self.inplace else ''} send [{names(self.st)}] recv [{names(self.rt)}] "
                f"B {self.B} soff {self.soff} roff {self.roff}")


# ---- N = 1: the seeds of tests/test_typed_fuzz_gpu.py -------------------------
SHAPES = ("send", "recv", "both")
SIZE_CLASSES = ("zero", "one", "elem", "g2047", "g2048", "g2049", "two_wg", "three_wg", "one_wg_40k")
SINGLE_SEEDS = 15 * len(SIZE_CLASSES)
EDGE = {"g2047": 2047, "g2048": 2048, "g2049": 2049}
AT_LEAST = {"two_wg": 16400, "three_wg": 32784, "one_wg_40k": 40960}   # copy_blocks: 2, 3, (param blocks = 1)


SOURCES = ("negstride", "descending", "negdisp", "interleaved", "padded", "stacked", "nested", None,
           "zero_extent", "sub_run_extent", "g2", "wide")


def single_case(s, stats=None):
    """(Case, meta) of N = 1 seed s.  s runs through every (granule aimed at,
    shape, size class); the way G is reached — the datatype's own granule, the
    buffer address under a 16-B-granule type, or whatever a freely drawn type
    gives — rotates with the shape, and the 64-bit walk with both."""
    assert 0 <= s < SINGLE_SEEDS
    gi, ti, ci = s % 5, (s // 5) % 3, s // 15
    gt, shape, size = GS[gi], SHAPES[ti], SIZE_CLASSES[ci]
    mode = ("type", "addr", "free")[(ti + ci) % 3]
    if size in EDGE or size == "one":
        mode = "type"     # only a type of size G (3 G, 4 G) gives that many granules
    stats = stats or Stats()
    rng = np.random.default_rng([s, 0x51])
    kind = KINDS[s % 7]
    types, soff, roff = {}, [0], [0]

    def units(n):   # pool classes whose size divides n granules
        return ("unit",) + (("tri", "run") if n % 3 == 0 else ()) + (("negstride",) if n % 4 == 0 else ())

    for side in (0, 1):
        if shape == ("recv", "send")[side]:   # "recv": the send side is bytes; "send": the receive side
            types[(side, 0)] = ("bytes", None)
        elif mode == "type":
            cls_in = units(EDGE.get(size, 1)) if size in EDGE or size == "one" else None
            types[(side, 0)] = draw_type(rng, side, stats, gran=gt, cls_in=cls_in)
        elif mode == "addr":
            types[(side, 0)] = draw_type(rng, side, stats, gran=16)
    off = [16 * int(rng.integers(0, 3)), 16 * int(rng.integers(0, 3))]
    if mode == "addr":    # the address picks G: the typed side's, or (one side typed) the contiguous side's
        which = [0, 1] if shape == "both" else [int(rng.integers(0, 2))]
        for side in which:
            off[side] += int(rng.choice(OFFSETS[gt]))
    elif mode == "free":
        off = [int(rng.choice([0, 1, 2, 4, 6, 8, 10, 16])) for _ in range(2)]
    fixed = {"zero": 0, "one": 1, "elem": 1}.get(size)
    source = lambda side, rank: SOURCES[(s // 5 + gi + 3 * side) % len(SOURCES)]  # noqa: E731
    case = Case(1000 + s, 1, kind, source=source, types=types, soff=[off[0]], roff=[off[1]], exact=1 if fixed is None else fixed,
                max_lcm=MAX_LCM if fixed is not None else 16384, stats=stats)
    if fixed is None:     # the same datatypes again, as many units as the size class asks for
        L = math.lcm(size_of(case.st[0]), size_of(case.rt[0]))
        exact = EDGE[size] * gt // L if size in EDGE else -(-AT_LEAST[size] // L)
        assert size not in EDGE or L * exact == EDGE[size] * gt
        case = Case(1000 + s, 1, kind, types={k: (case.cls[k], t) for k, t in (((0, 0), case.st[0]), ((1, 0), case.rt[0]))},
                    soff=[off[0]], roff=[off[1]], exact=exact, stats=Stats())
    meta = {"seed": s, "aim": gt, "shape": shape, "size": size, "mode": mode,
            "force64": (s // 5 + gi) % 2, "blocks": 1 if size == "one_wg_40k" else None,
            "forms": s % 4 == 0}
    return case, meta


def single_plan(case, meta, saddr=None, raddr=None, scratch=0, max_blocks=1024):
    """What the N = 1 call launches, from the layout alone: one entry per
    typed_copy_kernel launch of the first pass, {unpack, G, blocks, trips,
    cut_elem, cut_run, nelems}.  saddr / raddr: the buffer origins' addresses
    (default: the offsets the case asks for, past a 256-B boundary)."""
    B = case.B[0][0]
    if not B:
        return []
    st, rt = case.st[0], case.rt[0]
    sa = (256 + case.soff[0] if saddr is None else saddr) + case.sd[0][0] * ext_of(st)
    ra = (256 + case.roff[0] if raddr is None else raddr) + case.rd[0][0] * ext_of(rt)
    if meta["blocks"]:
        max_blocks = meta["blocks"]
    out = []
    for unpack, t, typed, contig in ((0, st, sa, ra if rt is None else scratch),
                                     (1, rt, ra, sa if st is None else scratch)):
        if t is None:
            continue
        G = typed_granule(gran_of(t), typed, contig)
        nb = copy_blocks(B, max_blocks)
        cuts = [a2a_slice(B, g, nb)[0] for g in range(1, nb)]
        cuts = [c for c in cuts if c < B]
        ends = set(np.cumsum([0] + [n for _, n in t.runs]).tolist())
        most = max(hi - lo for lo, hi in (a2a_slice(B, g, nb) for g in range(nb)))
        out.append({"unpack": unpack, "G": G, "blocks": nb, "trips": -(-(most // G) // TRIP),
                    "cut_elem": any(c % t.size for c in cuts),
                    "cut_run": any(c % t.size not in ends for c in cuts),
                    "nelems": len(t.elems), "w64": bool(meta["force64"])})
    return out


# ---- N > 1: the seeds of typed_worker.py's `layouts` case -----------------------
WORKER_SEEDS = 13
WORKER_SEEDS_N8 = (0, 1, 2, 3, 4, 9, 10, 11, 12)   # N = 8 runs a shorter list (see typed_worker.case_layouts)


def worker_rows(n, s):
    row = [(r * 3 + s) % 4 + 1 for r in range(n)]
    row[(s + 1) % n] = 0
    return row


def worker_case(s, n, path, stats=None):
    """(Case, meta) of seed s of the `layouts` case at N = n on forced path
    `path` (0 fused, 1 staged, 2 landing).  Seeds 0-6: the seven kinds, the
    root moving with seed and path, ragged rows with a zero, and seeds 0-4
    with every datatype from the pool at granule 1, 2, 4, 8, 16; 7, 8: in
    place; 9: more than 16 KiB per pair; 10: alltoall_chunk = 256 (landing
    path) and element sizes that do not divide 256; 11: G = 1 and full 4096-B
    fused slices (two trips); 12: the 64-bit walk."""
    assert 0 <= s < WORKER_SEEDS
    stats = stats or Stats()
    seed = 5000 + 100 * path + s
    meta = {"seed": s, "chunk": 0, "force64": 0, "G": None}
    kw = {"root": (s + path) % n, "rows": worker_rows(n, s + path), "stats": stats, "max_span": 2048,
          "source": lambda side, rank: SOURCES[(s + path + rank + 3 * side) % len(SOURCES)] if rank < 3 else None}
    P = directed_pool()

    def pooled(g, classes):
        names = sorted(k for k in P if gran_of(P[k][1]) == g and P[k][0] in classes)
        t = {}
        for side in (0, 1):
            for r in range(n):
                rng = np.random.default_rng([seed, r, side, 0x77])
                t[(side, r)] = P[names[int(rng.integers(len(names)))]]
        return t

    if s < 7:
        kind = KINDS[s]
        if s < 5:     # the granule is the datatypes' own: every rank draws from the pool's types of it
            meta["G"] = GS[s]
            kw.update(types=pooled(GS[s], ("unit", "tri", "run", "negstride", "g2", "many")),
                      soff=[16 * (r % 2) for r in range(n)], roff=[16 * ((r + 1) % 2) for r in range(n)])
        return Case(seed, n, kind, **kw), meta
    if s in (7, 8):
        return Case(seed, n, ("alltoall", "allgatherv")[s - 7], inplace=True, **kw), meta
    if s == 9:        # two workgroups per job (staged, landing), five fused groups
        kw.update(types=pooled(4, ("unit", "tri", "run", "negstride")), target=16400 + 12 * 4)
        return Case(seed, n, "alltoall", **kw), meta
    if s == 10:       # passes of 256 B cut elements of 3, 12, 48 B ... anywhere
        meta["chunk"] = 256
        kw.update(types=pooled((1, 4, 16)[path], ("tri", "run")), target=700)
        return Case(seed, n, "alltoallv", **kw), meta
    if s == 11:       # byte granules, 4096 of them per fused workgroup: two full trips
        meta["G"] = 1
        kw.update(types=pooled(1, ("unit", "tri", "run", "negstride", "many")), target=3 * 4096)
        return Case(seed, n, "alltoall", **kw), meta
    meta["force64"] = 1
    return Case(seed, n, "alltoallv", **kw), meta
