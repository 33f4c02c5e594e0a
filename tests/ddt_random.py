"""Random nested MPI datatypes for the fuzz tests (contiguous / vector /
indexed / struct, non-overlapping typemaps, non-negative displacements)."""
import numpy as np

from ompi_amd import datatype as dd

BASES = ["MPI_CHAR", "MPI_SHORT", "MPI_INT", "MPI_DOUBLE", "MPI_DOUBLE"]


def rand_type(rng, depth, bases=BASES):
    """A random datatype over the predefined `bases`, up to `depth` levels."""
    if depth == 0 or rng.random() < 0.2:
        return dd.predefined(bases[rng.integers(len(bases))])
    old = rand_type(rng, depth - 1, bases)
    k = int(rng.integers(4))
    if k == 0:
        return dd.type_contiguous(int(rng.integers(1, 6)), old)
    if k == 1:
        bl = int(rng.integers(1, 9))
        stride = bl + int(rng.choice([0, 1, 3, bl, 40]))
        return dd.type_vector(int(rng.integers(1, 60)), bl, stride, old)
    if k == 2:
        nb = int(rng.integers(1, 9))
        bls, disps, pos = [], [], int(rng.integers(0, 5))
        for _ in range(nb):
            b = int(rng.integers(0, 7))
            bls.append(b)
            disps.append(pos)
            pos += b + int(rng.integers(0, 7))
        return dd.type_indexed(bls, disps, old)
    m = int(rng.integers(2, 4))
    types = [old] + [rand_type(rng, depth - 1, bases) for _ in range(m - 1)]
    bls, disps, pos = [], [], int(rng.integers(0, 9))
    for t in types:
        b = int(rng.integers(1, 4))
        bls.append(b)
        disps.append(pos)
        # past the member's last byte (typemaps must not overlap: an
        # overlapping receive type is erroneous, its unpack order-dependent)
        pos += (b - 1) * t.extent + max(t.true_span, t.ub) + int(rng.integers(0, 13))
    return dd.type_struct(bls, disps, types)


def span_of(dt, count):
    """Bytes from the buffer base to the last typed byte of `count` elements."""
    return (count - 1) * dt.extent + dt.true_span


# ---- a second generator: the typemaps rand_type cannot draw ----------------
LAYOUT_CLASSES = ["negstride", "descending", "negdisp", "interleaved", "padded", "backward",
                  "stacked"]
LAYOUT_SEEDS = 160                      # tests/test_ddt_layouts_{cpu,gpu}.py
LAYOUT_TOTALS = [1 << 10, 60 << 10, 300 << 10, 1 << 20]   # packed bytes aimed at
WIDTH = {"MPI_CHAR": 1, "MPI_SHORT": 2, "MPI_INT": 4, "MPI_DOUBLE": 8}


def _base(rng):
    return dd.predefined(BASES[rng.integers(len(BASES))])


def _negstride(rng):
    old = _base(rng)
    bl = int(rng.integers(1, 9))
    gap = int(rng.choice([1, 3, bl, 40, 600]))
    count = int(rng.integers(2, 60)) if rng.random() < 0.7 else int(rng.integers(1000, 20000))
    return dd.type_vector(count, bl, -(bl + gap), old)


def _descending(rng):
    """Typemap order != address order: an indexed type with strictly
    decreasing displacements, or a struct whose members' displacements are
    permuted; 2-13 runs."""
    if rng.random() < 0.5:
        old = _base(rng)
        nb = int(rng.integers(2, 14))
        bls = [int(rng.integers(1, 7)) for _ in range(nb)]
        disps, pos = [], int(rng.integers(0, 5))
        for b in reversed(bls):  # laid out upwards, last block first
            disps.append(pos)
            pos += b + int(rng.integers(1, 7))
        return dd.type_indexed(bls, disps[::-1], old)
    m = int(rng.integers(2, 6))
    types = [_base(rng) for _ in range(m)]
    bls = [int(rng.integers(1, 4)) for _ in range(m)]
    order = rng.permutation(m)
    while m > 1 and np.all(order == np.arange(m)):
        order = rng.permutation(m)
    disps, pos = [0] * m, int(rng.integers(0, 3)) * 4
    for i in order:  # member order[0] lowest in memory, ...
        w = types[i].extent
        pos = -(-pos // w) * w
        disps[i] = pos
        pos += bls[i] * w + int(rng.integers(0, 3)) * w + (1 if rng.random() < 0.2 else 0)
    return dd.type_struct(bls, disps, types)


def _small(rng):
    """A small instance (a few runs, well under a tile) for the resized
    classes; half of them with typemap order != address order."""
    k = int(rng.integers(3))
    if k == 0:
        return _descending(rng)
    if k == 1:
        old = _base(rng)
        bl = int(rng.integers(1, 5))
        return dd.type_vector(int(rng.integers(2, 9)), bl, bl + int(rng.choice([1, 2, 5])), old)
    i32, f64 = dd.predefined("MPI_INT"), dd.predefined("MPI_DOUBLE")
    return dd.type_struct([1, 1], [0, 8], [i32, f64])


def run_bounds(dt):
    """(lowest typed byte, one past the highest) of one instance."""
    runs = dt.runs
    return min(d for d, _ in runs), max(d + n for d, n in runs)


def typed_bounds(dt, count):
    """(lowest typed byte, one past the highest) over `count` instances,
    relative to the buffer origin; the extent may be zero or negative."""
    lo, hi = run_bounds(dt)
    last = (count - 1) * dt.extent
    return lo + min(0, last), hi + max(0, last)


def rand_layout(rng, cls=None):
    """(class name, datatype) of one of LAYOUT_CLASSES (cls: of that one) — the layouts
    rand_type cannot draw: negative strides, typemap order != address order,
    runs below the origin, resized extents smaller than the span
    (interleaved instances), larger, negative, or overlapping.  The type's
    `max_count` (None: any) is the largest count at which instances do not
    overlap; `stacked` types overlap at every count > 1 (send only)."""
    if cls is None:
        r = rng.random()
        cls = "stacked" if r < 0.075 else LAYOUT_CLASSES[int((r - 0.075) / 0.925 * 6)]
    max_count = None
    if cls == "negstride":
        dt = _negstride(rng)
    elif cls == "descending":
        dt = _descending(rng)
    elif cls == "negdisp":
        old = [_negstride, _descending, _small][int(rng.integers(3))](rng)
        lo, hi = run_bounds(old)
        # some or all runs below the origin
        down = int(rng.integers(1, hi - lo + 40))
        down = -(-down // old.align) * old.align if rng.random() < 0.7 else down
        dt = dd.type_struct([1], [-lo - down], [old])
    elif cls == "interleaved":
        old = _base(rng)
        bl = int(rng.integers(1, 5))
        m = int(rng.integers(2, 17))        # stride = m blocks: m instances interleave
        c = int(rng.integers(2, 40)) if rng.random() < 0.5 else int(rng.integers(500, 40000))
        dt = dd.type_create_resized(dd.type_vector(c, bl, bl * m, old), 0, bl * old.extent)
        max_count = m
    elif cls == "padded":
        old = _descending(rng) if rng.random() < 0.5 else _small(rng)
        lo, hi = run_bounds(old)
        dt = dd.type_create_resized(old, lo, hi - lo + int(rng.choice([1, 4, 16, 129, 5000])))
    elif cls == "backward":
        old = _small(rng)
        lo, hi = run_bounds(old)
        dt = dd.type_create_resized(old, lo, -(hi - lo + int(rng.choice([0, 1, 8, 40, 200]))))
    else:  # stacked: instances overlap
        old = _base(rng)
        bl = int(rng.integers(2, 9))
        v = dd.type_vector(int(rng.integers(2, 30)), bl, bl + int(rng.choice([1, 3, 40])), old)
        dt = dd.type_create_resized(v, 0, 0 if rng.random() < 0.4
                                    else int(rng.integers(1, bl)) * old.extent)
    dt.max_count = max_count
    return cls, dt


def layout_case(seed):
    """The case of one seed of the layout tests: (rng, class, datatype,
    count, lo, hi) with [lo, hi) the typed bytes of all instances relative to
    the buffer origin."""
    rng = np.random.default_rng(31000 + seed)
    cls, dt = rand_layout(rng)
    target = int(rng.choice(LAYOUT_TOTALS))
    count = max(1, target // dt.size)
    if dt.max_count is not None:  # interleaved: at least two instances, at most max_count
        count = max(2, min(count, dt.max_count))
    count = min(count, max(1, (32 << 20) // max(abs(dt.extent), 1)))
    if cls == "stacked":
        count = max(count, 2)
    lo, hi = typed_bounds(dt, count)
    return rng, cls, dt, count, lo, hi


def all_runs(dt, count):
    """(starts, lengths) of every run of every instance in packed-stream
    order (numpy int64), relative to the buffer origin."""
    runs = np.array(dt.runs, dtype=np.int64).reshape(-1, 2)
    inst = np.arange(count, dtype=np.int64) * dt.extent
    starts = (inst[:, None] + runs[None, :, 0]).ravel()
    lens = np.broadcast_to(runs[None, :, 1], (count, len(runs))).ravel()
    return starts, lens
