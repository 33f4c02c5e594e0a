"""The collective fold on one GPU at every rank count from 2 to 16.

reduce_kernel needs no peer: it folds a set of source pointers.  Through
ompi_amd_coll_fold_local, n buffers of this one process are the n ranks'
inputs, and the library's own planners (allreduce_fold, fold_jobs,
tuned_reduce_order, tuned_reduce_scatter_order, the reduce_scatter and scan
jobs) and its own launch produce what a rank of an n-rank communicator would
hold — including reduce_kernel<.., 16>, which the multi-process tests
(N <= 8) never launch, and every rem / remain / extra >= 2.

Expected values come only from the oracle's message-flow simulations
(fold_local_cases.exp_*); the comparison is bit-exact, NaN equal only to NaN
at the same element.  tests/test_fold_local_cpu.py shows on these very inputs
that the algorithms told apart here differ in enough elements to fail a wrong
order.  Every destination sits between guard bytes that must stay unchanged.
"""
import functools

import numpy as np
import pytest

from ompi_amd import coll
from ompi_amd import op as mop

import fold_local_cases as fc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from coll_worker import inputs as worker_inputs  # noqa: E402
from test_op_gpu import _cplx, same_bits  # noqa: E402

DEV = "cuda:0"
GUARD = 64          # bytes before and after every destination range (keeps 16-B phase)
FILL = 0xA5


class Slot:
    def __init__(self, name, op, dt, make):
        self.name, self.op, self.dt, self.make = name, op, dt, make

    @functools.lru_cache(maxsize=None)
    def inputs(self, n):
        xs = self.make(self.dt, n)
        assert all(len(x) == fc.GEN for x in xs)
        return tuple(xs)

    @functools.lru_cache(maxsize=None)
    def on_device(self, n, disps=None):
        """(tensors, pointers) of the n inputs, input r displaced by
        disps[r] bytes from a 256-B aligned allocation."""
        disps = disps or (0,) * n
        ts, ps = [], []
        for x, d in zip(self.inputs(n), disps):
            raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
            t = torch.zeros(raw.nbytes + d + 16, dtype=torch.uint8, device=DEV)
            t[d:d + raw.nbytes].copy_(torch.from_numpy(raw.copy()))
            ts.append(t)
            ps.append(t.data_ptr() + d)
        return ts, ps


def _worker(salt):
    return lambda dt, n: [worker_inputs(dt, fc.GEN, r, salt + n) for r in range(n)]


def _complex(dt, n):
    f = mop.MPI_FLOAT
    return [_cplx(worker_inputs(f, fc.GEN, r, 700 + n), worker_inputs(f, fc.GEN, r, 800 + n),
                  dt.np_dtype) for r in range(n)]


MAXS = Slot("MAX-f32-specials", mop.MPI_MAX, mop.MPI_FLOAT, lambda dt, n: fc.f32_inputs(n, True))
SUMF = Slot("SUM-f32", mop.MPI_SUM, mop.MPI_FLOAT, lambda dt, n: fc.f32_inputs(n, False))
FULL = [MAXS, SUMF]
MORE = [
    Slot("SUM-f16", mop.MPI_SUM, mop.MPIX_C_FLOAT16, _worker(10)),       # E = 8, rounds every step
    Slot("SUM-f64", mop.MPI_SUM, mop.MPI_DOUBLE, _worker(20)),
    Slot("SUM-i8", mop.MPI_SUM, mop.MPI_INT8_T, _worker(30)),            # E = 16
    Slot("PROD-c64", mop.MPI_PROD, mop.MPI_C_FLOAT_COMPLEX, _complex),
    Slot("MAXLOC-double_int", mop.MPI_MAXLOC, mop.MPI_DOUBLE_INT, _worker(40)),  # 16-B extent, E = 1
    Slot("MINLOC-2int", mop.MPI_MINLOC, mop.MPI_2INT, _worker(50)),
    Slot("BXOR-u16", mop.MPI_BXOR, mop.MPI_UINT16_T, _worker(60)),
]
MORE_NS = [3, 5, 7, 8, 9, 12, 13, 16]
SI8 = MORE[2]

ids = lambda s: s.name if isinstance(s, Slot) else None  # noqa: E731


def new_dst(nbytes, disp=0):
    return torch.full((GUARD + disp + nbytes + GUARD,), FILL, dtype=torch.uint8, device=DEV)


def dst_ptr(t, disp=0):
    return t.data_ptr() + GUARD + disp


def read_dst(t, nbytes, dt, disp=0, what=()):
    """The destination range; the bytes around it must be untouched."""
    raw = t.cpu().numpy()
    lo = GUARD + disp
    assert (raw[:lo] == FILL).all(), ("guard bytes before the result", what)
    assert (raw[lo + nbytes:] == FILL).all(), ("guard bytes after the result", what)
    return raw[lo:lo + nbytes].view(dt.np_dtype)


def fold(slot, n, kind, counts, out_elems, *, srcs=None, ndst=1, dst_disps=None, what=(), **kw):
    """One fold_local call into fresh guarded destinations; returns every
    destination's result."""
    ps = srcs or slot.on_device(n)[1]
    nbytes = out_elems * slot.dt.extent
    dd = dst_disps or (0,) * ndst
    ds = [new_dst(nbytes, d) for d in dd]
    coll.fold_local(kind, ps, [dst_ptr(t, d) for t, d in zip(ds, dd)], counts, slot.dt, slot.op, **kw)
    return [read_dst(t, nbytes, slot.dt, d, what) for t, d in zip(ds, dd)]


def check(slot, got, exp, what):
    exp = np.ascontiguousarray(exp).view(slot.dt.np_dtype)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    if not same_bits(got, exp, slot.dt):
        g = np.ascontiguousarray(got).view(np.uint8).reshape(len(got), -1)
        e = np.ascontiguousarray(exp).view(np.uint8).reshape(len(exp), -1)
        bad = np.flatnonzero((g != e).any(axis=1))
        raise AssertionError(f"{slot.name} {what}: {bad.size}/{len(got)} elements differ "
                             f"(NaN pairs included), first {bad[:4].tolist()} last {int(bad[-1])}")


def allreduce_case(slot, n, count, alg, what, inplace=False, red_alg=0, **kw):
    exp = fc.exp_allreduce(slot.inputs(n), count, slot.op.index, slot.dt.code, alg, inplace, red_alg)
    for got in fold(slot, n, coll.FOLD_ALLREDUCE, count, count, alg=alg, red_alg=red_alg,
                    inplace=inplace, which=-1, what=what, **kw):
        check(slot, got, exp, what)


def reduce_scatter_cases(slot, n, algs, what):
    for rc in fc.rs_counts(n):
        for alg in algs:
            exp = fc.exp_reduce_scatter(slot.inputs(n), rc, slot.op.index, slot.dt.code, alg)
            for b in range(n):  # an empty block stores nothing: only the guards are checked
                w = (what, "reduce_scatter", "alg", alg, "rcounts", rc[:3], "block", b)
                got, = fold(slot, n, coll.FOLD_REDUCE_SCATTER, rc, rc[b], alg=alg, which=b, what=w)
                check(slot, got, exp[b], w)


# ------------------------------------------------------------------ the full grid
@pytest.mark.parametrize("n", fc.NS)
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_allreduce_every_algorithm(slot, n):
    """Fixed decision and forced algorithms 1..6 at the fallback counts
    (pof2 - 1: Rabenseifner -> linear; n - 1: ring -> recursive doubling), n,
    16 n + 5 and 4099; non-overlapping also under each forced reduce
    algorithm, rank 0 in place or not."""
    for count in fc.allreduce_counts(n):
        for alg in fc.AR_ALGS:
            allreduce_case(slot, n, count, alg, ("allreduce", n, "count", count, "alg", alg))
        for red in (1, 3, 4, 5):
            for inplace in (False, True):
                allreduce_case(slot, n, count, fc.AR_NONOVERLAPPING,
                               ("allreduce nonoverlapping", n, count, "red_alg", red, inplace),
                               inplace=inplace, red_alg=red)


@pytest.mark.parametrize("n", fc.NS)
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_allreduce_block_by_block(slot, n):
    """The owners' jobs: each ring block folded by its own call (Rabenseifner
    pieces cut at the ring blocks) into one destination gives the vector."""
    for count in (16 * n + 5, fc.COUNT):
        for alg in (fc.AR_RECURSIVE_DOUBLING, fc.AR_RING, fc.AR_RABENSEIFNER):
            exp = fc.exp_allreduce(slot.inputs(n), count, slot.op.index, slot.dt.code, alg)
            nbytes = count * slot.dt.extent
            t = new_dst(nbytes)
            for b in range(n):
                coll.fold_local(coll.FOLD_ALLREDUCE, slot.on_device(n)[1], [dst_ptr(t)], count,
                                slot.dt, slot.op, alg=alg, which=b)
            what = ("allreduce by block", n, count, alg)
            check(slot, read_dst(t, nbytes, slot.dt, 0, what), exp, what)


@pytest.mark.parametrize("n", fc.NS)
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_reduce_every_root(slot, n):
    """Fixed decision and forced 1, 3, 4, 5: every root, in place or not, at
    257 elements; roots 0, n // 2, n - 1 at 4099."""
    for count, roots in ((257, range(n)), (fc.COUNT, sorted({0, n // 2, n - 1}))):
        for red in fc.RED_ALGS:
            for root in roots:
                for inplace in (False, True):
                    what = ("reduce", n, "count", count, "alg", red, "root", root, inplace)
                    exp = fc.exp_reduce(slot.inputs(n), count, slot.op.index, slot.dt.code, root,
                                        inplace, red)
                    got, = fold(slot, n, coll.FOLD_REDUCE, count, count, red_alg=red, which=root,
                                inplace=inplace, what=what)
                    check(slot, got, exp, what)


@pytest.mark.parametrize("n", fc.NS)
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_reduce_scatter_every_block(slot, n):
    """Halving, ring, non-overlapping and the fixed decision: every block of
    equal and of ragged counts (one block empty); non-overlapping also with
    every rank in place under the binomial reduce; reduce_scatter_block at
    rcount 1, 5, 257."""
    reduce_scatter_cases(slot, n, (fc.RS_HALVING, fc.RS_RING, fc.RS_NONOVERLAPPING, 0), n)
    xs, op, code = slot.inputs(n), slot.op.index, slot.dt.code
    rc = fc.rs_counts(n)[1]
    exp = fc.exp_reduce_scatter(xs, rc, op, code, fc.RS_NONOVERLAPPING, fc.RED_BINOMIAL, True)
    for b in range(n):
        w = ("reduce_scatter nonoverlapping in place", n, b)
        got, = fold(slot, n, coll.FOLD_REDUCE_SCATTER, rc, rc[b], alg=fc.RS_NONOVERLAPPING,
                    red_alg=fc.RED_BINOMIAL, inplace=True, which=b, what=w)
        check(slot, got, exp[b], w)
    for rcount in (1, 5, 257):
        for red in (0, fc.RED_BINARY):
            exp = fc.exp_rsb(xs, rcount, op, code, red, slot.dt.np_dtype)
            for b in range(n):
                w = ("reduce_scatter_block", n, rcount, "red_alg", red, "block", b)
                got, = fold(slot, n, coll.FOLD_REDUCE_SCATTER_BLOCK, rcount, rcount, red_alg=red,
                            which=b, what=w)
                check(slot, got, exp[b], w)


@pytest.mark.parametrize("n", fc.NS)
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_scan_exscan_every_rank(slot, n):
    count = 257
    for exclusive in (False, True):
        exp = fc.exp_scan(slot.inputs(n), count, slot.op.index, slot.dt.code, exclusive)
        kind = coll.FOLD_EXSCAN if exclusive else coll.FOLD_SCAN
        for r in range(n):
            w = ("exscan" if exclusive else "scan", n, "rank", r)
            t = new_dst(count * 4)
            coll.fold_local(kind, slot.on_device(n)[1], [dst_ptr(t)], count, slot.dt, slot.op, which=r)
            if exclusive and r == 0:  # rank 0's rbuf is untouched
                assert (t.cpu().numpy() == FILL).all(), w
                continue
            check(slot, read_dst(t, count * 4, slot.dt, 0, w), exp[r], w)


def test_one_rank_is_a_copy():
    for kind, counts, which, off, cnt in (
            (coll.FOLD_ALLREDUCE, 1000, -1, 0, 1000), (coll.FOLD_REDUCE, 1000, 0, 0, 1000),
            (coll.FOLD_REDUCE_SCATTER, [777], 0, 0, 777), (coll.FOLD_SCAN, 33, 0, 0, 33)):
        x = fc.f32_inputs(2, True)[0]
        t = torch.from_numpy(x.copy()).to(DEV)
        d = new_dst(cnt * 4)
        coll.fold_local(kind, [t], [dst_ptr(d)], counts, mop.MPI_FLOAT, mop.MPI_MAX, which=which)
        got = read_dst(d, cnt * 4, mop.MPI_FLOAT)
        assert np.array_equal(got.view(np.uint32), x[off:off + cnt].view(np.uint32)), kind


# ------------------------------------------------------------------ further types and ops
@pytest.mark.parametrize("n", MORE_NS)
@pytest.mark.parametrize("slot", MORE, ids=ids)
def test_more_slots(slot, n):
    """Recursive doubling, ring and Rabenseifner allreduce and the halving
    reduce_scatter on types of other vector widths (E = 16, 8, 2, 1) and on
    the pair and complex handlers."""
    for count in fc.allreduce_counts(n):
        for alg in (fc.AR_RECURSIVE_DOUBLING, fc.AR_RING, fc.AR_RABENSEIFNER):
            allreduce_case(slot, n, count, alg, ("allreduce", n, "count", count, "alg", alg))
    reduce_scatter_cases(slot, n, (fc.RS_HALVING,), n)


# ------------------------------------------------------------------ alignment
@pytest.mark.parametrize("n", [5, 8, 13])
@pytest.mark.parametrize("slot", [MAXS, SI8], ids=ids)
def test_alignment(slot, n):
    """All buffers displaced alike inside 16 B (the head is peeled, vectors
    after it); one source displaced differently (no common phase: every
    element through the scalar loop); the destination displaced differently."""
    ext = slot.dt.extent
    k = ext * (1 if ext == 4 else 3)
    odd = n // 2
    layouts = [
        ("same", (k,) * n, k),
        ("one source off", tuple(k if r != odd else (k + ext) % 16 for r in range(n)), k),
        ("destination off", (k,) * n, (k + ext) % 16),
    ]
    xs, op, code = slot.inputs(n), slot.op.index, slot.dt.code
    for name, sd, dd in layouts:
        srcs = slot.on_device(n, sd)[1]
        for alg in (fc.AR_RECURSIVE_DOUBLING, fc.AR_RING, fc.AR_RABENSEIFNER):
            w = ("alignment", name, n, "allreduce", alg)
            exp = fc.exp_allreduce(xs, fc.COUNT, op, code, alg)
            got, = fold(slot, n, coll.FOLD_ALLREDUCE, fc.COUNT, fc.COUNT, srcs=srcs, dst_disps=(dd,),
                        alg=alg, which=-1, what=w)
            check(slot, got, exp, w)
        rc = fc.rs_counts(n)[1]
        exp = fc.exp_reduce_scatter(xs, rc, op, code, fc.RS_HALVING)
        for b in (0, n - 1):
            w = ("alignment", name, n, "reduce_scatter block", b)
            got, = fold(slot, n, coll.FOLD_REDUCE_SCATTER, rc, rc[b], srcs=srcs, dst_disps=(dd,),
                        alg=fc.RS_HALVING, which=b, what=w)
            check(slot, got, exp[b], w)


# ------------------------------------------------------------------ the multi-destination store
@pytest.mark.parametrize("n", [3, 8, 13, 16])
@pytest.mark.parametrize("slot", FULL, ids=ids)
def test_every_destination_gets_the_result(slot, n):
    """ndst = 1, 2, n (the fused push stores the owner's block into every
    rank's rbuf), non-temporal stores on and off; and with one destination at
    another phase, where the element loop stores to all of them."""
    for nd in (1, 2, n):
        for nt in (False, True):
            for alg in (fc.AR_RING, fc.AR_RABENSEIFNER):
                allreduce_case(slot, n, fc.COUNT, alg, ("ndst", nd, "nt", nt, n, alg), ndst=nd,
                               nt_store=nt)
    allreduce_case(slot, n, fc.COUNT, fc.AR_RING, ("ndst 2, second displaced", n), ndst=2,
                   dst_disps=(0, slot.dt.extent))


# ------------------------------------------------------------------ grid-stride trips
@pytest.mark.parametrize("n", [2, 3, 8, 16])
@pytest.mark.parametrize("slot", [MAXS, SUMF, SI8], ids=ids)
def test_block_cap_forces_grid_stride_trips(slot, n):
    """A cap of 1 or 2 workgroups makes each one walk the vector body and the
    scalar ends in several trips; the result is the default grid's."""
    for alg in (fc.AR_RECURSIVE_DOUBLING, fc.AR_RING, fc.AR_RABENSEIFNER):
        ref, = fold(slot, n, coll.FOLD_ALLREDUCE, fc.COUNT, fc.COUNT, alg=alg, which=-1)
        check(slot, ref, fc.exp_allreduce(slot.inputs(n), fc.COUNT, slot.op.index, slot.dt.code, alg),
              ("default cap", n, alg))
        for cap in (1, 2):
            for nt in (False, True):
                got, = fold(slot, n, coll.FOLD_ALLREDUCE, fc.COUNT, fc.COUNT, alg=alg, which=-1,
                            max_blocks=cap, nt_store=nt)
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint8),
                                      np.ascontiguousarray(ref).view(np.uint8)), (n, alg, cap, nt)
