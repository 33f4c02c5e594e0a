"""Convertor parity over the typemaps rand_type cannot draw
(tests/ddt_random.py rand_layout): negative strides, typemap order != address
order, runs below the buffer origin, resized extents smaller than the span
(interleaved instances), larger, negative (instances march down in memory)
and overlapping (send only).  Shaped like test_convertor_random_types: pack
in random-length calls, unpack in other random-length calls into a pre-filled
buffer, one iovec train each way, packed buffers at odd offsets; byte-exact
against the oracle, gap bytes and the 64 guard bytes on each side of the typed
range unchanged.  A closing test reads the library's route counters: every
route the dispatcher has was taken by the seeds or by the directed cases
here.  One more test has typed offsets past 2^32."""
import time

import numpy as np
import pytest

from ddt_knob_worker import run_worker
from ddt_random import LAYOUT_SEEDS, layout_case, typed_bounds
from ompi_amd import _lib
from ompi_amd import datatype as dd
from test_ddt_fuzz_gpu import chunk_lengths, dev_rand

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
SEEN = {"seeds": 0, "directed": 0}


@pytest.fixture(scope="module", autouse=True)
def route_tally():
    _lib.ddt_route_reset()
    SEEN["seeds"] = SEEN["directed"] = 0
    yield


def run_case(orc, rng, dt, count, what, seed, shift, poff, unpack=True, whole=False):
    """Pack, unpack and one iovec train each way of `count` x dt against the
    oracle.  The device buffer holds [low, hi) of the typed bytes between two
    guards, after `shift` bytes; the oracle gets a numpy view at the same
    origin.  whole: the pack and the unpack in one call each."""
    total = dt.size * count
    lo, hi = typed_bounds(dt, count)

    def calls():
        return [total] if whole else chunk_lengths(rng, total)

    low = min(lo, 0)
    n = hi - low + 2 * GUARD
    origin = GUARD - low                       # in the compared region
    runs = dt.runs
    src = dev_rand(shift + n, 100 + seed)
    base = src.data_ptr() + shift + origin
    src_np = src.cpu().numpy()[shift:shift + n].copy()
    exp = orc.pack(runs, dt.extent, count, src_np[origin:], 0, total)
    assert exp.nbytes == total, what

    packed = torch.zeros(total + poff + 64, dtype=torch.uint8, device=DEV)
    conv = dd.Convertor()
    conv.prepare_for_send(dt, count, base)
    pos = 0
    for k in calls():
        done, moved = conv.pack(packed.data_ptr() + poff + pos, k)
        assert moved == min(k, total - pos), what
        pos += moved
    assert pos == total and done == 1, what
    torch.cuda.synchronize()
    got = packed.cpu().numpy()[poff:poff + total]
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: pack differs first at {bad[:1]}"

    def unpack_check(fill_seed, mover, label):
        fill = dev_rand(shift + n, fill_seed)
        exp_dst = fill.cpu().numpy()[shift:shift + n].copy()
        orc.unpack(runs, dt.extent, count, exp, exp_dst[origin:], 0)
        conv = dd.Convertor()
        conv.prepare_for_recv(dt, count, fill.data_ptr() + shift + origin)
        mover(conv)
        torch.cuda.synchronize()
        got_dst = fill.cpu().numpy()[shift:shift + n]
        bad = np.flatnonzero(got_dst != exp_dst)
        assert bad.size == 0, (f"{what}: {label} differs first at typed byte "
                               f"{bad[:1] - origin} (guards at {lo - GUARD}..{lo}, {hi}..{hi + GUARD})")

    def unpack_calls(conv):
        pos = 0
        for k in calls():
            pos += conv.unpack(packed.data_ptr() + poff + pos, k)[1]
        assert pos == total, what

    if unpack:
        unpack_check(200 + seed, unpack_calls, "unpack")

    # one iovec train: random fragment lengths at random gaps, two calls
    lens = chunk_lengths(rng, total, max_calls=120)
    gaps = rng.integers(0, 24, len(lens))
    offs = np.concatenate([[0], np.cumsum(np.array(lens) + gaps)[:-1]]).astype(np.int64)
    train = torch.zeros(int(offs[-1]) + lens[-1] + 64, dtype=torch.uint8, device=DEV)
    iovs = [(train.data_ptr() + int(o), int(k)) for o, k in zip(offs, lens)]
    half = max(1, len(iovs) // 2)
    conv = dd.Convertor()
    conv.prepare_for_send(dt, count, base)
    moved_all = 0
    for part in (iovs[:half], iovs[half:]):
        if part:
            moved_all += conv.pack_iov(part)[3]
    assert moved_all == total, what
    torch.cuda.synchronize()
    t_np = train.cpu().numpy()
    got = np.concatenate([t_np[o:o + k] for o, k in zip(offs, lens)])
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: iovec pack differs first at {bad[:1]}"

    def unpack_train(conv):
        for part in (iovs[:half], iovs[half:]):
            if part:
                conv.unpack_iov(part)

    if unpack:
        unpack_check(300 + seed, unpack_train, "iovec unpack")
    dt.free()


@pytest.mark.parametrize("seed", range(LAYOUT_SEEDS))
def test_convertor_layouts(orc, seed):
    rng, cls, dt, count, lo, hi = layout_case(seed)
    shift = int(rng.integers(0, 13))
    poff = int(rng.choice([0, 16, 1, 3, 8]))
    what = (f"seed {seed} [{cls}]: {dt.name} x {count} ({len(dt.elems)} elems, "
            f"{dt.size * count} B, extent {dt.extent}, typed [{lo}, {hi}), shift {shift}, poff {poff})")
    # overlapping instances are legal for a send only
    run_case(orc, rng, dt, count, what, seed, shift, poff, unpack=cls != "stacked")
    SEEN["seeds"] += 1


def directed_cases():
    f64, i32 = dd.predefined("MPI_DOUBLE"), dd.predefined("MPI_INT")
    return {
        # one run per period, 16-B granule, window past 256 KiB: the identity
        # tile each way and under an iovec train (the classes above have no
        # single positive-stride vector)
        "vector_bl2_gap16": (lambda: dd.type_vector(40000, 2, 4, f64), 1, 0, 0),
        # the same runs down in memory: a negative stride is never periodic
        # for the tile, so the 16-B walk takes the 640 KiB window
        "negvector_bl4": (lambda: dd.type_vector(20000, 4, -44, f64), 1, 0, 16),
        # the 16-B walk with a negative extent (instances march down)
        "backward_vector_bl2": (lambda: dd.type_create_resized(
            dd.type_vector(16, 2, 6, f64), 0, -1024), 2000, 0, 0),
        # a byte map in permuted typemap order under the tile, 4-B granules
        "permuted_struct": (lambda: dd.type_struct([1, 2, 1], [16, 0, 8], [f64, i32, i32]),
                            30000, 4, 0),
    }


@pytest.mark.parametrize("name", list(directed_cases()))
def test_directed_routes(orc, name):
    make, count, shift, poff = directed_cases()[name]
    dt = make()
    rng = np.random.default_rng(5)
    # one call each way: the windows are past the tile's 256 KiB
    run_case(orc, rng, dt, count, f"{name}: {dt.name} x {count}", 900, shift, poff, whole=True)
    SEEN["directed"] += 1


def test_every_route_taken():
    """Every route of the dispatcher was taken by this module's seeds and
    directed cases.  The 32-bit multiply-high search needs
    OMPI_AMD_DDT_FASTDIV=1 from the start of the process, so a fresh child
    runs three of the classes under it and its counters are added."""
    if SEEN["seeds"] != LAYOUT_SEEDS or SEEN["directed"] != len(directed_cases()):
        pytest.skip("needs the whole module run in this process")
    counts = _lib.ddt_route_counts()
    lines = run_worker({"OMPI_AMD_DDT_FASTDIV": "1", "OMPI_AMD_DDT_TILE": "0"},
                       cases="descending,interleaved,negstride", sizes=str(300 << 10))
    assert lines and all(ln["ok"] for ln in lines), [ln for ln in lines if not ln["ok"]][:3]
    for ln in lines:
        for k, v in ln["routes"].items():
            counts[k] += v
    missing = [r for r in _lib.DDT_ROUTES if counts[r] == 0]
    assert not missing, (missing, counts)


def test_typed_offsets_past_32_bits():
    """Typed offsets past 2^32 in a 4 GiB + 64 MiB buffer: k * stride in the
    16-B walk and in the 8-B walk, el * extent in the 64-bit element search
    (and its iovec form).  The runs are written and read with device index
    operations over the run addresses; the expected packed bytes are the
    written values in stream order; after the unpack the whole buffer equals
    the fill value outside the runs."""
    free, _ = torch.cuda.mem_get_info()
    if free < (12 << 30):
        pytest.skip("needs 12 GiB of free device memory")
    t0 = time.time()
    nbytes = (4 << 30) + (64 << 20)
    FILL = 0x5A
    buf = torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)
    f64, i32 = dd.predefined("MPI_DOUBLE"), dd.predefined("MPI_INT")
    layouts = [
        # 1024 runs of 64 B, stride 4 MiB + 64 KiB: 16-B walk, the last 16 runs past 2^32
        ("vec16", dd.type_vector(1024, 8, ((4 << 20) + (64 << 10)) // 8, f64), 1, 0, "vec16"),
        # 8192 runs of 8 B, stride 520 KiB + 8 B (8 mod 16), base 8 mod 16: 8-B walk
        ("vec8", dd.type_vector(8192, 1, (520 << 10) // 8 + 1, f64), 1, 8, "vec_g"),
        # struct{int,double} at an extent of 2,700,008 B x 1600: element search
        ("struct", dd.type_create_resized(dd.type_struct([1, 1], [0, 8], [i32, f64]), 0, 2700008),
         1600, 0, "generic64"),
    ]
    gen = torch.Generator(device=DEV).manual_seed(77)
    for name, dt, count, shift, route in layouts:
        runs = np.array(dt.runs, dtype=np.int64)
        inst = np.arange(count, dtype=np.int64) * dt.extent
        starts = (inst[:, None] + runs[None, :, 0]).ravel() + shift
        lens = np.broadcast_to(runs[None, :, 1], (count, len(runs))).ravel()
        total = int(lens.sum())
        assert total == dt.size * count
        top = int((starts + lens).max())
        assert (1 << 32) < top <= nbytes, (name, top)
        idx_np = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(total)
        idx = torch.from_numpy(idx_np).to(DEV)
        vals = torch.empty(total, dtype=torch.uint8, device=DEV).random_(0, 256, generator=gen)
        buf[idx] = vals
        _lib.ddt_route_reset()
        packed = torch.zeros(total + 64, dtype=torch.uint8, device=DEV)
        conv = dd.Convertor()
        conv.prepare_for_send(dt, count, buf.data_ptr() + shift)
        done, moved = conv.pack(packed, total)
        torch.cuda.synchronize()
        assert (done, moved) == (1, total), name
        assert torch.equal(packed[:total], vals), f"{name}: pack differs"
        assert _lib.ddt_route_counts()[route] == 1, (name, _lib.ddt_route_counts())
        # iovec pack: three entries
        train = torch.zeros(total + 64, dtype=torch.uint8, device=DEV)
        cut = [total // 3 + 5, total // 3 - 3]
        cut.append(total - sum(cut))
        offs = [0, cut[0], cut[0] + cut[1]]
        conv = dd.Convertor()
        conv.prepare_for_send(dt, count, buf.data_ptr() + shift)
        assert conv.pack_iov([(train.data_ptr() + o, k) for o, k in zip(offs, cut)])[3] == total
        torch.cuda.synchronize()
        assert torch.equal(train[:total], vals), f"{name}: iovec pack differs"
        # unpack other values over the runs, then an iovec unpack of a third set
        for how in ("unpack", "iovec unpack"):
            vals2 = torch.empty(total, dtype=torch.uint8, device=DEV).random_(0, 256, generator=gen)
            conv = dd.Convertor()
            conv.prepare_for_recv(dt, count, buf.data_ptr() + shift)
            if how == "unpack":
                assert conv.unpack(vals2, total) == (1, total)
            else:
                conv.unpack_iov([(vals2.data_ptr() + o, k) for o, k in zip(offs, cut)])
            torch.cuda.synchronize()
            assert torch.equal(buf[idx], vals2), f"{name}: {how} differs in the runs"
        buf[idx] = FILL
        piece = 256 << 20
        for o in range(0, nbytes, piece):
            assert bool((buf[o:o + piece] == FILL).all()), f"{name}: a byte outside the runs changed near {o}"
        dt.free()
    print(f"typed offsets past 2^32: {time.time() - t0:.2f} s")
