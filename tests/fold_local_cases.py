"""Inputs and oracle expectations shared by tests/test_fold_local_gpu.py and
tests/test_fold_local_cpu.py (numpy + the CPU oracle only, no GPU).

Every expected value is one of the oracle's message-flow simulations of the
reference's algorithms (orc.allreduce / allreduce_forced / reduce /
reduce_scatter / reduce_scatter_block / scan) — never a restatement of the
device's fold().  The inputs of a rank count n are drawn once at GEN
elements with seed 100 + n; a case of fewer elements takes their prefix.
"""
import functools

import numpy as np

from oracle import oracle as orc

COUNT = 4099  # fp32 over 16 ring blocks: every block has a head, a vector body and a tail
GEN = 257 * 16  # elements drawn per rank: reduce_scatter_block at rcount 257 on 16 ranks
NS = list(range(2, 17))
MAX, SUM = 1, 3
F32 = 15

# coll_tuned_allreduce_algorithm (0 = the fixed decision)
AR_ALGS = [0, 1, 2, 3, 4, 5, 6]
AR_LINEAR, AR_NONOVERLAPPING, AR_RECURSIVE_DOUBLING, AR_RING, AR_RABENSEIFNER = 1, 2, 3, 4, 6
# coll_tuned_reduce_algorithm the device path runs (0 = the fixed decision)
RED_ALGS = [0, 1, 3, 4, 5]
RED_LINEAR, RED_PIPELINE, RED_BINARY, RED_BINOMIAL = 1, 3, 4, 5
# coll_tuned_reduce_scatter_algorithm -> the oracle's numbering
RS_NONOVERLAPPING, RS_HALVING, RS_RING = 1, 2, 3
RS_TO_ORACLE = {0: orc.RS_TUNED, RS_NONOVERLAPPING: orc.RS_NONOVERLAPPING, RS_HALVING: orc.RS_HALVING,
                RS_RING: orc.RS_RING}


def pof2_floor(n: int) -> int:
    a = 1
    while a * 2 <= n:
        a *= 2
    return a


def allreduce_counts(n: int) -> list[int]:
    """Rabenseifner's and the ring's fallbacks, one element per rank, a few
    vectors per rank, and COUNT."""
    return sorted({pof2_floor(n) - 1, n - 1, n, 16 * n + 5, COUNT} - {0})


@functools.lru_cache(maxsize=None)
def f32_inputs(n: int, specials: bool) -> tuple:
    """uniform(-1, 1) fp32; specials: {NaN, 0.0, -0.0, 1.0} over half the
    positions (MAX then depends on the operand order: NaN and the sign of a
    zero are taken from one side)."""
    rng = np.random.default_rng(100 + n)
    xs = [rng.uniform(-1, 1, GEN).astype(np.float32) for _ in range(n)]
    if specials:
        sp = np.array([np.nan, 0.0, -0.0, 1.0], dtype=np.float32)
        for x in xs:
            idx = rng.integers(0, GEN, GEN // 2)
            x[idx] = rng.choice(sp, idx.size)
    for x in xs:
        x.setflags(write=False)
    return tuple(xs)


def prefix(xs, count: int) -> list:
    return [np.ascontiguousarray(x[:count]).copy() for x in xs]


def differ(a: np.ndarray, b: np.ndarray) -> int:
    """Elements whose bits differ, not counting those NaN in both."""
    if a.dtype.kind == "f":
        both = np.isnan(a) & np.isnan(b)
        w = np.dtype(f"u{a.dtype.itemsize}")
        return int(np.count_nonzero((a.view(w) != b.view(w)) & ~both))
    return int(np.count_nonzero(a != b))


def exp_allreduce(xs, count, op, code, alg, root0_inplace=False, red_alg=0) -> np.ndarray:
    """Rank 0's result (every rank holds the same bits; the GPU test needs
    one).  Non-overlapping with a forced reduce algorithm is coll/tuned's
    reduce to rank 0 with that algorithm + bcast."""
    s = prefix(xs, count)
    if alg == 0:
        return orc.allreduce(s, count, op, code)[0][0]
    if alg == AR_NONOVERLAPPING and red_alg != 0:
        return orc.reduce(s, count, op, code, 0, root0_inplace, red_alg)[0]
    return orc.allreduce_forced(s, count, op, code, alg, root0_inplace=root0_inplace)[0][0]


def exp_reduce(xs, count, op, code, root, inplace, red_alg) -> np.ndarray:
    return orc.reduce(prefix(xs, count), count, op, code, root, inplace, red_alg)[0]


def exp_reduce_scatter(xs, rcounts, op, code, alg, red_alg=0, inplace=False) -> list:
    s = prefix(xs, sum(rcounts))
    return orc.reduce_scatter(s, list(rcounts), op, code, RS_TO_ORACLE[alg], red_alg, inplace)[0]


def exp_rsb(xs, rcount, op, code, red_alg, np_dtype) -> list:
    s = prefix(xs, rcount * len(xs))
    return [r.view(np_dtype) for r in orc.reduce_scatter_block(s, rcount, op, code, red_alg)]


def exp_scan(xs, count, op, code, exclusive) -> list:
    return orc.scan(prefix(xs, count), count, op, code, exclusive)


def rs_counts(n: int) -> list[list[int]]:
    """Equal blocks, and ragged ones with an empty block (total <= COUNT)."""
    equal = [COUNT // n] * n
    ragged = [(37 * (b + 1)) % 53 + (200 if b % 5 == 1 else 0) for b in range(n)]
    ragged[n // 2] = 0
    assert sum(ragged) <= COUNT and sum(equal) <= COUNT
    return [equal, ragged]
