"""Properties of the second typemap generator (tests/ddt_random.py
rand_layout) over the seeds tests/test_ddt_layouts_gpu.py runs: every class
is drawn, instances overlap only in the `stacked` class, the oracle itself
handles these layouts (signed displacements, strides and extents), and the
inputs would expose a convertor that ignored typemap order or the sign of a
stride.  No GPU."""
import collections

import numpy as np
import pytest

from ddt_random import (LAYOUT_CLASSES, LAYOUT_SEEDS, all_runs, layout_case, typed_bounds)
from ompi_amd import datatype as dd


@pytest.fixture(scope="module")
def cases():
    return [layout_case(seed) for seed in range(LAYOUT_SEEDS)]


def ownership(dt, count, lo, hi):
    """How many runs own each typed byte of [lo, hi)."""
    starts, lens = all_runs(dt, count)
    diff = np.zeros(hi - lo + 1, dtype=np.int64)
    np.add.at(diff, starts - lo, 1)
    np.add.at(diff, starts + lens - lo, -1)
    return np.cumsum(diff)[:-1]


def gather(buf, origin, starts, lens):
    """The packed stream of runs (starts, lens) read from buf, in the order given."""
    idx = np.concatenate([np.arange(s, s + n) for s, n in zip(starts + origin, lens)]) \
        if len(starts) < 4096 else (np.repeat(starts + origin - np.concatenate(
            [[0], np.cumsum(lens)[:-1]]), lens) + np.arange(int(lens.sum())))
    return buf[idx]


def test_every_class_is_drawn(cases):
    seen = collections.Counter(c[1] for c in cases)
    assert set(seen) == set(LAYOUT_CLASSES), seen
    assert all(seen[k] >= 8 for k in LAYOUT_CLASSES), seen
    # the only seeds whose unpack is skipped (overlapping instances: send only)
    assert 8 * seen["stacked"] <= LAYOUT_SEEDS, seen


def test_resized_keeps_the_typemap():
    v = dd.type_vector(3, 2, 5, dd.predefined("MPI_INT"))
    r = dd.type_create_resized(v, -4, 8)
    assert r.elems == v.elems and r.size == v.size
    assert (r.lb, r.ub, r.extent) == (-4, 4, 8)
    assert dd.type_create_resized(v, 0, -48).extent == -48
    assert typed_bounds(dd.type_create_resized(v, 0, -48), 3) == (-96, 48)


def test_only_stacked_overlaps(cases):
    for seed, (_, cls, dt, count, lo, hi) in enumerate(cases):
        own = ownership(dt, count, lo, hi)
        assert own.min() >= 0 and own.max() >= 1
        if cls == "stacked":
            assert own.max() > 1, (seed, dt.name, count)
        else:
            assert own.max() == 1, (seed, cls, dt.name, count)
        if cls in ("negstride", "negdisp", "backward"):
            assert lo < 0, (seed, cls, dt.name)
        if cls == "interleaved":  # instances interleave: an instance spans more than the extent
            assert count > 1 and 0 < dt.extent < dt.true_span, (seed, dt.name, count)


def test_oracle_handles_the_layouts(orc, cases):
    """Pack by the oracle equals a numpy gather over the signed run
    addresses; the oracle's unpack of it into a pre-filled buffer reproduces
    the owned bytes and leaves every other byte (guards included) alone."""
    for seed, (_, cls, dt, count, lo, hi) in enumerate(cases):
        rng = np.random.default_rng(seed)
        guard, low = 64, min(lo, 0)   # the buffer holds [low, hi) between two guards
        origin = guard - low
        buf = rng.integers(0, 256, hi - low + 2 * guard, dtype=np.uint8)
        total = dt.size * count
        packed = orc.pack(dt.runs, dt.extent, count, buf[origin:], 0, total)
        assert packed.nbytes == total
        starts, lens = all_runs(dt, count)
        assert np.array_equal(packed, gather(buf, origin, starts, lens)), (seed, cls, dt.name)
        if cls == "stacked":
            continue
        dst = rng.integers(0, 256, buf.size, dtype=np.uint8)
        before = dst.copy()
        assert orc.unpack(dt.runs, dt.extent, count, packed, dst[origin:], 0) == total
        own = np.zeros(buf.size, dtype=bool)
        own[origin + lo:origin + hi] = ownership(dt, count, lo, hi) > 0
        assert np.array_equal(dst[own], buf[own]), (seed, cls, dt.name)
        assert np.array_equal(dst[~own], before[~own]), (seed, cls, dt.name)


def test_inputs_catch_order_and_sign_mistakes(orc, cases):
    """A pack that walked the runs in address order, and for negative strides
    one that took abs(stride), gives other bytes than the right pack: in
    every negstride seed for the sign, and in several seeds of every class
    for the order."""
    differs = collections.Counter()
    for seed, (_, cls, dt, count, lo, hi) in enumerate(cases):
        rng = np.random.default_rng(1000 + seed)
        low = min(lo, 0)
        origin = -low
        buf = rng.integers(0, 256, hi - low, dtype=np.uint8)
        total = dt.size * count
        right = orc.pack(dt.runs, dt.extent, count, buf[origin:], 0, total)
        starts, lens = all_runs(dt, count)
        order = np.argsort(starts, kind="stable")
        if not np.array_equal(gather(buf, origin, starts[order], lens[order]), right):
            differs[cls] += 1
        if cls == "negstride":
            (c, bl, st, d), = dt.elems
            assert st < 0
            k = np.arange(c, dtype=np.int64) * -st + d
            inst = np.arange(count, dtype=np.int64) * dt.extent
            s2 = (inst[:, None] + k[None, :]).ravel()
            hi2 = int(s2.max()) + bl
            buf2 = rng.integers(0, 256, max(hi2, hi) - low, dtype=np.uint8)
            right2 = orc.pack(dt.runs, dt.extent, count, buf2[origin:], 0, total)
            wrong = gather(buf2, origin, s2, np.full(s2.size, bl, dtype=np.int64))
            assert not np.array_equal(wrong, right2), (seed, dt.name)
    assert all(differs[k] >= 4 for k in LAYOUT_CLASSES), differs
