"""CPU side of the single-process fold tests (tests/test_fold_local_gpu.py).

1. ompi_amd_coll_fold_local's argument checks, all of which return before
   any device call.
2. The GPU test can fail: on the very inputs it uses, the oracle's results
   of the algorithms it tells apart differ in enough elements that a device
   fold in the wrong operand order, association or in-place swap cannot pass.
   The thresholds are conditions on the inputs (fold_local_cases.f32_inputs):
   if a pair falls under one, the input has to change, not the threshold.
   Measured with these inputs: MAX/specials allreduce pairs >= 3.7 % for
   every n >= 3, the tightest in-place swap (binomial, n = 16) 0.5 %; SUM
   ring against recursive doubling 21 % (n = 3) to 68 % (n = 16).
"""
import ctypes

import numpy as np
import pytest

from ompi_amd import _lib

import fold_local_cases as fc

SUCCESS, UNSUPPORTED, BAD_PARAM = 0, -1, -2
ALLREDUCE, REDUCE, REDUCE_SCATTER, RSB, SCAN, EXSCAN = range(6)
SUM_F32 = (15, 3)


def _call(kind, size, srcs, dsts, ndst, counts, type_op=SUM_F32, alg=0, red_alg=0, which=0,
          inplace=0, max_blocks=0, nt=0):
    lib = _lib.load()
    sp = None if srcs is None else (ctypes.c_void_p * len(srcs))(*srcs)
    dp = None if dsts is None else (ctypes.c_void_p * len(dsts))(*dsts)
    cv = None if counts is None else (ctypes.c_size_t * len(counts))(*counts)
    return lib.ompi_amd_coll_fold_local(kind, size, sp, dp, ndst, cv, type_op[0], type_op[1], alg,
                                        red_alg, which, inplace, max_blocks, nt, None)


def test_fold_local_argument_checks():
    """Every return below happens before a HIP call (this runs without a GPU):
    the pointers are never dereferenced as device memory."""
    p4 = [0x1000] * 4
    # size, ndst, kind, counts
    for size in (0, -1, 17):
        assert _call(ALLREDUCE, size, p4, p4, 1, [8], which=-1) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 0, [8], which=-1) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 5, [8], which=-1) == BAD_PARAM
    assert _call(-1, 4, p4, p4, 1, [8]) == BAD_PARAM
    assert _call(6, 4, p4, p4, 1, [8]) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 1, None, which=-1) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], which=-1, max_blocks=-1) == BAD_PARAM
    # root / block / rank
    for kind in (REDUCE, REDUCE_SCATTER, RSB, SCAN, EXSCAN):
        counts = [2, 2, 2, 2] if kind == REDUCE_SCATTER else [8]
        assert _call(kind, 4, p4, p4, 1, counts, which=4) == BAD_PARAM
        assert _call(kind, 4, p4, p4, 1, counts, which=-1) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], which=4) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], which=-2) == BAD_PARAM
    # algorithm numbers
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], which=-1, alg=7) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], which=-1, alg=-1) == BAD_PARAM
    assert _call(REDUCE, 4, p4, p4, 1, [8], red_alg=2) == UNSUPPORTED   # chain with fan-out
    assert _call(REDUCE, 4, p4, p4, 1, [8], red_alg=7) == UNSUPPORTED
    assert _call(REDUCE_SCATTER, 4, p4, p4, 1, [2, 2, 2, 2], alg=4) == UNSUPPORTED
    # undefined (op, type): SUM DOUBLE_INT, MAXLOC float, an op that does not exist
    assert _call(REDUCE, 4, p4, p4, 1, [8], type_op=(35, 3)) == UNSUPPORTED
    assert _call(SCAN, 4, p4, p4, 1, [8], type_op=(15, 11)) == UNSUPPORTED
    assert _call(ALLREDUCE, 4, p4, p4, 1, [8], type_op=(15, 99), which=-1) == UNSUPPORTED
    # null pointers with a non-zero count
    assert _call(ALLREDUCE, 4, None, p4, 1, [8], which=-1) == BAD_PARAM
    assert _call(ALLREDUCE, 4, p4, None, 1, [8], which=-1) == BAD_PARAM
    assert _call(REDUCE, 4, [0x1000, 0, 0x1000, 0x1000], p4, 1, [8]) == BAD_PARAM
    assert _call(REDUCE, 4, p4, [0x1000, 0], 2, [8]) == BAD_PARAM
    # a scan reads only the ranks it folds: rank 1 never touches srcs[2], srcs[3]
    assert _call(SCAN, 4, [0x1000, 0, 0, 0], p4, 1, [8], which=1) == BAD_PARAM
    # zero counts: success, even on null pointers
    for kind in (ALLREDUCE, REDUCE, RSB, SCAN, EXSCAN):
        assert _call(kind, 4, None, None, 1, [0], which=-1 if kind == ALLREDUCE else 0) == SUCCESS
    assert _call(REDUCE_SCATTER, 4, None, None, 1, [0, 0, 0, 0]) == SUCCESS
    assert _call(REDUCE_SCATTER, 4, None, None, 1, [3, 0, 3, 3], which=1) == SUCCESS  # my block is empty
    assert _call(EXSCAN, 4, None, None, 1, [8], which=0) == SUCCESS  # rank 0 receives nothing
    # and a zero count does not excuse a bad size or root
    assert _call(REDUCE, 17, None, None, 1, [0]) == BAD_PARAM
    assert _call(REDUCE, 4, None, None, 1, [0], which=9) == BAD_PARAM


MAX_MIN = 16              # 0.4 % of COUNT


@pytest.mark.parametrize("n", [n for n in fc.NS if n >= 3])
def test_max_specials_separate_orders_and_swaps(n):
    xs = fc.f32_inputs(n, True)
    ar = {a: fc.exp_allreduce(xs, fc.COUNT, fc.MAX, fc.F32, a)
          for a in (fc.AR_LINEAR, fc.AR_RECURSIVE_DOUBLING, fc.AR_RING, fc.AR_RABENSEIFNER)}
    pairs = [(fc.AR_RECURSIVE_DOUBLING, fc.AR_RABENSEIFNER), (fc.AR_RECURSIVE_DOUBLING, fc.AR_RING),
             (fc.AR_LINEAR, fc.AR_RECURSIVE_DOUBLING)]
    for a, b in pairs:
        d = fc.differ(ar[a], ar[b])
        print(f"n={n} MAX allreduce alg {a} vs {b}: {d} / {fc.COUNT}")
        assert d >= MAX_MIN, (n, a, b, d)
    root = n // 2
    for red in (fc.RED_PIPELINE, fc.RED_BINARY, fc.RED_BINOMIAL):
        d = fc.differ(fc.exp_reduce(xs, fc.COUNT, fc.MAX, fc.F32, root, False, red),
                      fc.exp_reduce(xs, fc.COUNT, fc.MAX, fc.F32, root, True, red))
        print(f"n={n} MAX reduce alg {red} root {root} in place vs not: {d} / {fc.COUNT}")
        assert d >= MAX_MIN, (n, red, d)


@pytest.mark.parametrize("n", [n for n in fc.NS if n >= 3])
def test_sum_separates_associations(n):
    xs = fc.f32_inputs(n, False)
    ring = fc.exp_allreduce(xs, fc.COUNT, fc.SUM, fc.F32, fc.AR_RING)
    tree = fc.exp_allreduce(xs, fc.COUNT, fc.SUM, fc.F32, fc.AR_RECURSIVE_DOUBLING)
    d = fc.differ(ring, tree)
    print(f"n={n} SUM ring vs recursive doubling: {d} / {fc.COUNT}")
    assert 5 * d >= fc.COUNT, (n, d)   # 20 %
    rc = fc.rs_counts(n)[0]
    halv = np.concatenate(fc.exp_reduce_scatter(xs, rc, fc.SUM, fc.F32, fc.RS_HALVING))
    rng_ = np.concatenate(fc.exp_reduce_scatter(xs, rc, fc.SUM, fc.F32, fc.RS_RING))
    d = fc.differ(halv, rng_)
    print(f"n={n} SUM reduce_scatter halving vs ring: {d} / {halv.size}")
    assert 5 * d >= halv.size, (n, d)


@pytest.mark.parametrize("n", fc.NS)
def test_sum_cannot_tell_rabenseifner_from_recursive_doubling(n):
    """fp32 SUM has the same association in both and commuted operands, so
    their results are equal: only the MAX/specials leg pins Rabenseifner's
    operand order (the `right` half, the owner's masks).  Keep that leg."""
    xs = fc.f32_inputs(n, False)
    a = fc.exp_allreduce(xs, fc.COUNT, fc.SUM, fc.F32, fc.AR_RECURSIVE_DOUBLING)
    b = fc.exp_allreduce(xs, fc.COUNT, fc.SUM, fc.F32, fc.AR_RABENSEIFNER)
    assert fc.differ(a, b) == 0
