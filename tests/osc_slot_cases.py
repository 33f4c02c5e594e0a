"""Case table and numpy expectations for the one-sided accumulate kernels
(ompi_amd/csrc/osc_ipc.hip), one entry per (op, type) slot the oracle
defines.  Pure numpy + the CPU oracle: importable and checkable without a
GPU (tests/test_osc_slots_cpu.py); tests/test_osc_slots_gpu.py runs it.

Every case is `target_after = op_2buff(op, type, in=origin, inout=target)`
and `fetched = target_before` on inputs from test_op_gpu.gen, on one of the
paths of the library:

    a  acc_kernel's 16-B vector body and its tail (operands 16-B aligned)
    b  acc_kernel's one-element-per-lane loop (one operand displaced)
    c  rma_small_kernel (one launch) and the boundary to lock/kernel/unlock
    d  ddt_acc_kernel (derived target), and a packed derived origin
    p  ddt_pair_kernel (pair type with a derived side)
    w  the second trip of the grid-stride loops (more than the grid cap)
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from ompi_amd import datatype as dd
from ompi_amd import op as mop
from test_op_gpu import SLOTS, gen, same_bits  # noqa: F401  (same_bits re-exported)

# ---- shape constants; test_osc_slots_cpu.py checks each against the source
K_RMA_SMALL_BYTES = 16 << 10  # osc_ipc.hip kRmaSmallBytes: last byte count of the one-launch path
K_OSC_THREADS = 256           # osc_ipc.hip kOscThreads: lanes per workgroup of every kernel here
K_OSC_UNROLL = 4              # osc_ipc.hip kOscUnroll: 16-B vectors per lane per pass of acc_kernel
K_ACC_UNROLL = 4              # osc_ipc.hip kAccUnroll: elements per lane per pass of ddt_acc_kernel
K_OSC_MAX_BLOCKS = 256        # osc_ipc.hip kOscMaxBlocks: osc_grid_cap() without the environment
K_DDT_LDS_ELEMS = 256         # ddt_device.h kDdtLdsElems: longest element table staged in LDS

# one full chunk of acc_kernel's vector body (kOscThreads * kOscUnroll) + 5:
# two workgroups, the second with five live vectors
N_VECS = K_OSC_THREADS * K_OSC_UNROLL + 5
# one full pass of ddt_acc_kernel (kOscThreads * kAccUnroll) + 5 elements
N_DDT = K_OSC_THREADS * K_ACC_UNROLL + 5
# one workgroup of ddt_pair_kernel (kOscThreads, one pair per lane) + 5 pairs
N_PAIR = K_OSC_THREADS + 5
# past the grid cap: kOscMaxBlocks full chunks, then the shapes above again
N_WRAP_VECS = K_OSC_MAX_BLOCKS * K_OSC_THREADS * K_OSC_UNROLL + N_VECS  # acc_kernel, 16-B vectors
N_WRAP_ELEMS = K_OSC_MAX_BLOCKS * K_OSC_THREADS + N_PAIR                # per-element loop, pair kernel
N_WRAP_DDT = K_OSC_MAX_BLOCKS * K_OSC_THREADS * K_ACC_UNROLL + N_DDT    # ddt_acc_kernel

GUARD = 64   # bytes after every operated region that must stay as they were
DISP = 48    # 16-B aligned window displacement of a contiguous target (bytes before it: untouched)
N_SINGLE = 64  # the n = 1 cases draw their element from gen(dt, N_SINGLE, seed)

assert N_VECS == 1029 and N_DDT == 1029 and N_PAIR == 261


def n_vec(e: int) -> int:
    """1029 vectors of E = 16 / e elements and E - 1 tail elements."""
    E = 16 // e
    return N_VECS * E + (E - 1)


def n_small(e: int) -> int:
    """The last count rma_small_kernel takes (exactly kRmaSmallBytes)."""
    return K_RMA_SMALL_BYTES // e


PAIR_CODES = {mop.MPI_FLOAT_INT.code, mop.MPI_DOUBLE_INT.code, mop.MPI_LONG_INT.code,
              mop.MPI_2INT.code, mop.MPI_SHORT_INT.code}
FP_CODES = {mop.MPIX_C_FLOAT16.code, mop.MPI_FLOAT.code, mop.MPI_DOUBLE.code}
FP_PAIR_CODES = {mop.MPI_FLOAT_INT.code, mop.MPI_DOUBLE_INT.code}
WRAP_SLOTS = {(mop.MPI_SUM.index, mop.MPI_FLOAT.code), (mop.MPI_BXOR.index, mop.MPI_UINT8_T.code),
              (mop.MPI_PROD.index, mop.MPI_C_DOUBLE_COMPLEX.code),
              (mop.MPI_MAXLOC.index, mop.MPI_DOUBLE_INT.code)}


def is_pair(dt) -> bool:
    return dt.code in PAIR_CODES


def order_sensitive(op, dt) -> bool:
    """Slots where f(target, origin) and f(origin, target) differ on gen's
    data: MAX / MIN of fp (a NaN against a number and +0 against -0 resolve
    to the second operand) and MAXLOC / MINLOC of the fp pairs (gen plants
    its NaN values at the same indices of both operands, an unordered
    compare keeps the target's pair, and the indices differ).

    The three integer pair types are NOT here although they carry the same
    rule: over a total order LOC_FUNC is commutative in (v, k) — the larger
    value wins whichever side holds it, a tie takes min(k) — so no input
    tells the operand order apart.  test_osc_slots_cpu.py asserts that, so
    the claim is checked, not assumed."""
    if op in (mop.MPI_MAX, mop.MPI_MIN):
        return dt.code in FP_CODES
    if op in (mop.MPI_MAXLOC, mop.MPI_MINLOC):
        return dt.code in FP_PAIR_CODES
    return False


def slots(orc):
    """The (op, type) slots of test_op_gpu.SLOTS the oracle defines."""
    return [(op, dt) for op, dt in SLOTS if orc.defined(op.index, dt.code)]


def slot_id(op, dt) -> str:
    return f"{op.name}-{dt.name}"


def first_of_size(orc, op, dt) -> bool:
    """True for the first slot of each element extent: it also runs the
    cases that depend on the element size only (the granule-typed REPLACE /
    NO_OP kernels)."""
    for o, d in slots(orc):
        if d.extent == dt.extent:
            return o is op and d is dt
    return False


# ---- inputs ---------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _gen_cached(code: int, n: int, seed: int) -> np.ndarray:
    a = gen(mop.BY_CODE[code], n, seed)
    a.setflags(write=False)
    return a


def inputs(dt, n: int, seed: int):
    """(origin, target_before) of `n` elements, read-only."""
    return _gen_cached(dt.code, n, 2 * seed + 1), _gen_cached(dt.code, n, 2 * seed + 2)


def edge_elements(dt, n: int):
    """Where a loop over n elements starts and ends: the first element, the
    first element after the last whole 16-B vector (acc_kernel's tail; the
    per-element loop's first element when nothing is vectorised is 0), the
    last element."""
    E = max(1, 16 // dt.extent)
    return sorted({0, min(n - 1, (n // E) * E), n - 1})


@functools.lru_cache(maxsize=None)
def _edge_seed(orc, op_index: int, code: int, n: int, seed: int) -> int:
    op = next(o for o in mop.OPS if o.index == op_index)
    dt = mop.BY_CODE[code]
    for j in range(400):
        o, t = inputs(dt, n, seed + 1000 * j)
        e = np.array(edge_elements(dt, n))
        oe, te = np.ascontiguousarray(o[e]), np.ascontiguousarray(t[e])
        r = apply_op(orc, op, dt, oe, te)
        if all(not same_bits(r[i:i + 1], te[i:i + 1], dt) for i in range(len(e))):
            return seed + 1000 * j
    raise AssertionError(f"no seed moves the edge elements of {op.name} {dt.name} n={n}")


def case_inputs(orc, case, dt):
    """(origin, target_before) of a case.  Where the call carries the
    slot's op, the first seed of case.seed, case.seed + 1000, ... at which
    the oracle's result differs from the target at every edge element: a
    loop that starts one element late or ends one early then shows in every
    slot, also under a selecting rule that keeps about half the elements."""
    n, seed = case.n, case.seed
    if case.path == "c1":
        return inputs(dt, N_SINGLE, seed)
    if case.op not in (mop.MPI_REPLACE, mop.MPI_NO_OP):
        seed = _edge_seed(orc, case.op.index, dt.code, n, seed)
    return inputs(dt, n, seed)


def apply_op(orc, op, dt, origin: np.ndarray, target: np.ndarray) -> np.ndarray:
    """target_after for the op of a call (REPLACE / NO_OP included)."""
    if op is mop.MPI_NO_OP:
        return target.copy()
    if op is mop.MPI_REPLACE:
        return origin.copy()
    out = target.copy()
    orc.op_2buff(op.index, dt.code, np.ascontiguousarray(origin), out, len(out))
    return out


def discriminates(orc, op, dt, origin, target):
    """(differs from the untouched target, from a plain replace, from the
    swapped operands) for the oracle's result on these inputs."""
    res = apply_op(orc, op, dt, origin, target)
    swp = apply_op(orc, op, dt, target, origin)
    return (not same_bits(res, target, dt), not same_bits(res, origin, dt),
            not same_bits(res, swp, dt))


@functools.lru_cache(maxsize=None)
def _single_picks(orc, op_index: int, code: int, seed: int):
    op = next(o for o in mop.OPS if o.index == op_index)
    dt = mop.BY_CODE[code]
    o, t = inputs(dt, N_SINGLE, seed)
    want = [True, True, order_sensitive(op, dt)]
    flags = [discriminates(orc, op, dt, o[i:i + 1], t[i:i + 1]) for i in range(N_SINGLE)]
    for i, f in enumerate(flags):  # one element that shows everything
        if all(f[k] or not want[k] for k in range(3)):
            return (i,)
    picks = []
    for k in range(3):  # else the first element for each property
        if want[k] and not any(flags[i][k] for i in picks):
            picks.append(next(i for i in range(N_SINGLE) if flags[i][k]))
    return tuple(sorted(set(picks)))


def single_picks(orc, op, dt, seed: int):
    """Indices into inputs(dt, N_SINGLE, seed) the n = 1 case (fetch_and_op)
    runs on, one call each.

    gen(dt, 1, seed) cannot serve for any seed: at n = 1 a pair's value is
    always -0.0 on both sides (index 0 takes both planted specials), and a
    selecting rule (MAX, MIN, MAXLOC, MINLOC, LAND / LOR of bool) returns
    one of its two operands, so ONE element can never differ from both the
    untouched target and a plain replace.  So the element comes from a
    N_SINGLE-element draw, and where no single element shows every property
    the shortest set that shows them jointly runs: a result other than the
    target, a result other than the origin and, for the order-sensitive
    slots, a result other than f(origin, target)."""
    return _single_picks(orc, op.index, dt.code, seed)


# ---- datatypes --------------------------------------------------------------
def member_runs(dt):
    """(offset, length) of the bytes MPI owns in one element."""
    nd = dt.np_dtype
    if is_pair(dt):
        return [(nd.fields["v"][1], nd.fields["v"][0].itemsize), (nd.fields["k"][1], 4)]
    return [(0, dt.extent)]


@functools.lru_cache(maxsize=None)
def prim_type(code: int):
    dt = mop.BY_CODE[code]
    return dd.from_runs(f"prim_{dt.name}", member_runs(dt), dt.extent)


@dataclass(frozen=True)
class Lay:
    """A derived side of a call: the library's datatype and count, and the
    same typemap as the oracle's pack / unpack take it (`reps` repetitions,
    `extent` apart, of `runs`), stated on its own."""
    ddt: object
    count: int
    runs: tuple
    extent: int
    reps: int

    @property
    def span(self) -> int:
        return (self.count - 1) * self.ddt.extent + self.ddt.true_span


def _lay(ddt, count):
    return Lay(ddt, count, tuple(ddt.runs), ddt.extent, count)


def _vector_lay(code: int, n: int, stride: int):
    """n single elements, `stride` elements apart."""
    dt = mop.BY_CODE[code]
    return Lay(dd.type_vector(n, 1, stride, prim_type(code)), 1, tuple(member_runs(dt)),
               stride * dt.extent, n)


@functools.lru_cache(maxsize=None)
def layout(kind: str, code: int) -> Lay:
    """N_DDT elements (N_PAIR pairs) of the type in a derived layout.

    vector   a gap after every element: ONE table entry (kept in registers)
    indexed  three runs of different lengths (table in LDS)
    packed   the element at displacement e / 2 of an extent of 2 e, as in a
             packed struct: runs that are no multiple of e, so the 64-bit
             offset path on elements that are not e-aligned
    long     294 runs of 3 and 4 elements, more than kDdtLdsElems (table
             in global memory)
    origin   a vector with blocks of 3 (packed into scratch first)
    result   a vector with a gap of two elements
    split    pairs only: value and index in separate runs"""
    dt = mop.BY_CODE[code]
    e, p = dt.extent, prim_type(code)
    n = N_PAIR if is_pair(dt) else N_DDT
    if kind == "vector":
        return _vector_lay(code, n, 2)
    if kind == "indexed":
        return _lay(dd.type_indexed([300, 400, n - 700], [2, 310, 720], p), 1)
    if kind == "packed":
        return _lay(dd.from_runs(f"packed_{dt.name}", [(e // 2, e)], 2 * e), n)
    if kind == "long":
        runs, pos = [], 0
        for i in range(2 * (n // 7)):
            ln = 3 if i % 2 == 0 else 4
            runs.append((pos * e, ln * e))
            pos += ln + 1
        assert sum(r[1] for r in runs) == n * e and len(runs) > K_DDT_LDS_ELEMS
        return _lay(dd.from_runs(f"long_{dt.name}", runs, pos * e), 1)
    if kind == "origin":
        return _lay(dd.type_vector(n // 3, 3, 5, p), 1)
    if kind == "result":
        return _vector_lay(code, n, 3)
    if kind == "split":
        (v0, vl), _ = member_runs(dt)
        return _lay(dd.from_runs(f"split_{dt.name}", [(v0, vl), (16, 4)], 24), n)
    raise KeyError(kind)


def to_stream(dt, a: np.ndarray) -> np.ndarray:
    """Packed stream bytes of memory elements (a pair: value then index)."""
    if not is_pair(dt):
        return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), dt.extent)
    return np.concatenate([raw[:, o:o + ln] for o, ln in member_runs(dt)], axis=1).reshape(-1).copy()


def from_stream(dt, s: np.ndarray) -> np.ndarray:
    """Memory elements of a packed stream (a pair's gap bytes zero)."""
    if not is_pair(dt):
        return s.copy().view(dt.np_dtype)
    n = s.nbytes // dt.size
    raw = np.zeros((n, dt.extent), np.uint8)
    src, pos = s.reshape(n, dt.size), 0
    for o, ln in member_runs(dt):
        raw[:, o:o + ln] = src[:, pos:pos + ln]
        pos += ln
    return raw.reshape(-1).view(dt.np_dtype)


# ---- cases ------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    path: str            # a, b, c, c1 (n = 1), d, p, w
    call: str            # acc, gacc, fop (contiguous calls); acc_ddt, gacc_ddt
    op: object           # the op of the call (the slot's, MPI_REPLACE or MPI_NO_OP)
    n: int
    seed: int
    disp: int = DISP     # window byte displacement of the target
    ooff: int = 0        # byte offset of the origin in its 16-B aligned buffer
    roff: int = 0        # ... of a contiguous result
    tkind: str = ""      # layout() kinds; "" = contiguous
    okind: str = ""
    rkind: str = ""
    exact: bool = False  # the whole window compared byte-exactly (ddt_pair_kernel)
    picks: tuple = ()    # c1: the elements fetch_and_op runs on

    @property
    def fetch(self) -> bool:
        return self.call in ("gacc", "fop", "gacc_ddt")


def cases_for(orc, op, dt):
    """Every case of the slot (op, dt), in path order."""
    e, pair = dt.extent, is_pair(dt)
    step = e if e < 16 else 8  # one element; a 16-B type by its C alignment of 8
    first = first_of_size(orc, op, dt)
    R, N = mop.MPI_REPLACE, mop.MPI_NO_OP
    nv, ns = n_vec(e), n_small(e)
    out = [
        Case("a/accumulate", "a", "acc", op, nv, 11),
        Case("a/get_accumulate", "a", "gacc", op, nv, 12),
        Case("b/target displaced", "b", "acc", op, nv, 13, disp=DISP + step),
        Case("b/origin displaced", "b", "gacc", op, nv, 14, ooff=step),
        Case("c/fetch_and_op", "c1", "fop", op, 1, 15, picks=single_picks(orc, op, dt, 15)),
        Case("c/last small", "c", "gacc", op, ns, 16),
        Case("c/first large", "c", "gacc", op, ns + 1, 17),
    ]
    for n in (ns, ns + 1):
        out.append(Case(f"c/REPLACE n={n}", "c", "gacc", R, n, 18))
        out.append(Case(f"c/NO_OP n={n}", "c", "gacc", N, n, 19))
        if first:  # the granule below 16: an operand displaced by one element
            out.append(Case(f"c/REPLACE origin displaced n={n}", "c", "gacc", R, n, 20, ooff=step))
            out.append(Case(f"c/NO_OP result displaced n={n}", "c", "gacc", N, n, 21, roff=step))
    if not pair:
        kinds = ["vector", "indexed"] + (["packed"] if e >= 2 else [])
        for i, k in enumerate(kinds):
            out.append(Case(f"d/{k} accumulate", "d", "acc_ddt", op, N_DDT, 30 + i, tkind=k))
            out.append(Case(f"d/{k} get_accumulate", "d", "gacc_ddt", op, N_DDT, 40 + i, tkind=k))
        if first:
            out.append(Case("d/long REPLACE", "d", "gacc_ddt", R, N_DDT, 50, tkind="long"))
            out.append(Case("d/long NO_OP", "d", "gacc_ddt", N, N_DDT, 51, tkind="long"))
        out.append(Case("d/derived origin", "d", "acc_ddt", op, N_DDT, 52, okind="origin"))
    else:
        sd = 60
        for tk, ok in (("vector", ""), ("split", ""), ("", "vector")):
            what = f"{tk or 'contiguous'} target" + (", derived origin" if ok else "")
            for o in (op, R, N):
                if o is not N:
                    out.append(Case(f"p/{what} {o.name} accumulate", "p", "acc_ddt", o, N_PAIR, sd,
                                    tkind=tk, okind=ok, exact=True))
                out.append(Case(f"p/{what} {o.name} get_accumulate", "p", "gacc_ddt", o, N_PAIR, sd + 1,
                                tkind=tk, okind=ok, rkind="result", exact=True))
                sd += 2
    if (op.index, dt.code) in WRAP_SLOTS:
        E = 16 // e
        out.append(Case("w/vector body", "w", "acc", op, N_WRAP_VECS * E, 80))
        out.append(Case("w/per-element loop", "w", "acc", op, N_WRAP_ELEMS, 81, disp=DISP + step))
        if pair:
            out.append(Case("w/pair kernel", "w", "acc_ddt", op, N_WRAP_ELEMS, 82, tkind="wrap",
                            exact=True))
        else:
            out.append(Case("w/derived target", "w", "acc_ddt", op, N_WRAP_DDT, 83, tkind="wrap"))
    return out


def case_layouts(case: Case, dt):
    """(target, origin, result) layouts of a case: a Lay, or None (contiguous)."""
    def one(kind):
        if not kind:
            return None
        if kind == "wrap":
            return _wrap_layout(dt.code, case.n)
        return layout(kind, dt.code)
    return one(case.tkind), one(case.okind), one(case.rkind)


@functools.lru_cache(maxsize=4)
def _wrap_layout(code: int, n: int) -> Lay:
    return _vector_lay(code, n, 2)  # the vector layout at a wrap count


# ---- expectations -------------------------------------------------------------
@dataclass
class Built:
    win0: np.ndarray      # window bytes before the call (GUARD bytes after the target's span)
    origin: np.ndarray    # origin buffer bytes (ooff junk bytes first), or None (NO_OP)
    result0: np.ndarray   # result buffer bytes before the call, or None
    win_exp: np.ndarray   # window bytes after the call
    touched: np.ndarray   # bool per window byte: a member byte of a target element
    wfree: np.ndarray     # bool per window byte: unspecified after the call (see _place)
    result_exp: np.ndarray  # result buffer bytes after the call, or None
    rtouched: np.ndarray    # bool per result byte: a member byte fetched into
    rfree: np.ndarray


def _junk(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(9000 + seed).integers(0, 256, n, dtype=np.uint8)


def _place(orc, lay, dt, elems: np.ndarray, buf: np.ndarray, at: int):
    """Write memory elements into `buf` at byte `at` through a layout (None:
    contiguous, whole elements with their gap bytes).  Returns (members,
    gaps): the mask of the member bytes written, and of a pair's gap bytes
    between them in a contiguous region — store_elem leaves those
    unspecified, so no test compares them."""
    mask = np.zeros(buf.nbytes, bool)
    gaps = np.zeros(buf.nbytes, bool)
    if lay is None:
        raw = np.ascontiguousarray(elems).view(np.uint8).reshape(-1)
        buf[at:at + raw.nbytes] = raw
        m = mask[at:at + raw.nbytes].reshape(len(elems), dt.extent)
        for o, ln in member_runs(dt):
            m[:, o:o + ln] = True
        gaps[at:at + raw.nbytes] = ~mask[at:at + raw.nbytes]
        return mask, gaps
    stream = to_stream(dt, elems)
    view = buf[at:].copy()
    assert orc.unpack(list(lay.runs), lay.extent, lay.reps, stream, view, 0) == stream.nbytes
    buf[at:] = view
    mview = np.zeros(buf.nbytes - at, np.uint8)
    orc.unpack(list(lay.runs), lay.extent, lay.reps, np.full(stream.nbytes, 1, np.uint8), mview, 0)
    mask[at:] = mview.astype(bool)
    return mask, gaps


def extract(orc, lay, dt, buf: np.ndarray, at: int, n: int) -> np.ndarray:
    """The n memory elements a layout describes in `buf` at byte `at`."""
    if lay is None:
        return buf[at:at + n * dt.extent].copy().view(dt.np_dtype)
    s = orc.pack(list(lay.runs), lay.extent, lay.reps, buf[at:].copy(), 0, n * dt.size)
    assert s.nbytes == n * dt.size
    return from_stream(dt, s)


def build(orc, case: Case, dt) -> Built:
    """Buffers and expectations of one case, on numpy only."""
    tl, ol, rl = case_layouts(case, dt)
    n, e = case.n, dt.extent
    if case.path == "c1":
        n = N_SINGLE
    origin, target = case_inputs(orc, case, dt)
    tspan = tl.span if tl else n * e
    win0 = _junk(case.seed, case.disp + tspan + GUARD)
    touched, wfree = _place(orc, tl, dt, target, win0, case.disp)
    if case.exact:
        wfree[:] = False
    # target_after: the whole call's (c1: only the picked elements change)
    after = apply_op(orc, case.op, dt, origin, target)
    if case.path == "c1":
        keep = np.ones(n, bool)
        keep[list(case.picks)] = False
        after[keep] = target[keep]
    win_exp = win0.copy()
    if tl is None and not is_pair(dt):
        _place(orc, None, dt, after, win_exp, case.disp)
    elif tl is None:
        # members only: a pair's gap bytes keep the window's (ddt_pair_kernel
        # promises it; on the other paths they are not compared)
        raw = np.ascontiguousarray(after).view(np.uint8).reshape(n, e)
        dst = win_exp[case.disp:case.disp + n * e].reshape(n, e)
        for o, ln in member_runs(dt):
            dst[:, o:o + ln] = raw[:, o:o + ln]
    else:
        _place(orc, tl, dt, after, win_exp, case.disp)
    obuf = None
    if case.op is not mop.MPI_NO_OP:
        ospan = ol.span if ol else n * e
        obuf = _junk(case.seed + 100, case.ooff + ospan + GUARD)
        _place(orc, ol, dt, origin, obuf, case.ooff)
    result0 = result_exp = rtouched = rfree = None
    if case.fetch:
        rspan = rl.span if rl else n * e
        result0 = _junk(case.seed + 200, case.roff + rspan + GUARD)
        result_exp = result0.copy()
        if case.path == "c1":  # one element per call, fetched to the same index
            rtouched = np.zeros(result0.nbytes, bool)
            rfree = np.zeros(result0.nbytes, bool)
            for i in case.picks:
                m, g = _place(orc, None, dt, target[i:i + 1], result_exp, case.roff + i * e)
                rtouched |= m
                rfree |= g
        else:
            rtouched, rfree = _place(orc, rl, dt, target, result_exp, case.roff)
    return Built(win0, obuf, result0, win_exp, touched, wfree, result_exp, rtouched, rfree)


def window_bytes(orc) -> int:
    """The largest window any case of any slot needs."""
    need = 0
    for op, dt in slots(orc):
        for c in cases_for(orc, op, dt):
            tl, _, _ = case_layouts(c, dt)
            n = N_SINGLE if c.path == "c1" else c.n
            need = max(need, c.disp + (tl.span if tl else n * dt.extent) + GUARD)
    return need
