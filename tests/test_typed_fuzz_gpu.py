"""Fuzz of typed_copy_kernel and typed_walk (csrc/coll_kernels.h) in one
process: at N = 1 a *_typed call is one TCP_SRC_TYPED job (send side typed),
one TCP_DST_TYPED job (receive side typed), or a pack into a scratch half and
an unpack out of it (both typed).  Each seed of typed_random.single_case is
one call of one of the seven collectives with generated datatypes, byte-exact
against oracle.pack / oracle.unpack over the whole of both buffers: guards,
gap bytes over a random prefill, the source unchanged.

The seed list walks through every granule G x shape x size class: 0 bytes,
one granule, one element, 2047 / 2048 / 2049 granules of G (the end of a
workgroup's first trip of 256 x 8 granules), more than 16 KiB and more than
32 KiB packed (two and three workgroups per job, whose 16-B slice cuts fall
inside elements and runs), and 40 KiB with param blocks = 1 (2560 granules at
G = 16, 5120 at G = 8 in ONE workgroup: its second and third trip, which the
default grid of 16 KiB per workgroup never gives at G >= 8).  Every fourth
seed also runs the nonblocking form and a persistent plan started twice over
refilled buffers.  The closing tally asserts what was reached, from
typed_granule, typed_walk64 and the layouts.

What no legal call reaches: the bytewise tail loop of typed_pipe_copy (bytes
past the last whole granule of a slice).  A slice's lo is a multiple of 16
(a2a_slice rounds `per` up to 16; pass boundaries are multiples of 256), its
hi is such a cut or the end of the pair, and the pair is whole elements,
whose size G divides (G divides the datatype's granule, which divides every
run).  So hi - lo is a multiple of G on every slice;
tests/test_typed_fuzz_cpu.py::test_no_legal_call_reaches_the_tail_loop checks
that over these seeds.  Nor does any test move 2^32 granules in one pair
(typed_walk64's own threshold): the 64-bit walk runs through typed_force64.

typed_granule is the host's evaluation of coll_typed.h's rule for the last
launch; with both sides typed that is the unpack, and the pack's G is the
rule's value for the addresses the test chose, not a reading.
"""
import collections
import os
import secrets
import sys
import time

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import typed_random as tr  # noqa: E402
from ompi_amd import datatype as dd  # noqa: E402

SEEN = collections.Counter()
RAN = set()


@pytest.fixture(scope="module")
def comm():
    from ompi_amd import coll
    c = coll.Communicator(f"typfuzz_{os.getpid()}_{secrets.token_hex(4)}", 0, 1, 0)
    c.scratch = max(c.get_param("small_bytes"), 4 << 20)   # the constructor's scratch_bytes, per half
    SEEN.clear()
    RAN.clear()
    yield c
    c.free()


def record(case, plan):
    for e in plan:
        G = e["G"]
        SEEN[("G", G, e["unpack"], e["w64"])] += 1
        SEEN[("trips", G, e["unpack"], min(e["trips"], 3))] += 1
        SEEN[("blocks", G, min(e["blocks"], 3))] += 1
        SEEN[("cut", G)] += e["cut_elem"] and e["cut_run"]
        SEEN["many"] += e["nelems"] > 8
    for k, cls in case.cls.items():
        SEEN[("class", cls)] += 1
    for side in (0, 1):
        SEEN["below_origin"] += case.geometry(side, 0)[0] < 0
    SEEN[("bytes", min(case.B[0][0], 2))] += 1


@pytest.mark.parametrize("s", range(tr.SINGLE_SEEDS))
def test_typed_copy_fuzz(comm, s):
    import typed_worker as tw
    case, meta = tr.single_case(s)
    x = tw.GenCall(comm, case)
    blocks0 = comm.get_param("blocks")
    comm.set_param("typed_force64", meta["force64"])
    if meta["blocks"]:
        comm.set_param("blocks", meta["blocks"])
    try:
        plan = tr.single_plan(case, meta, saddr=x.sbuf.ptr, raddr=x.rbuf.ptr, max_blocks=blocks0)
        w0 = comm.get_param("typed_walk64")
        ok, msg = x.run()
        assert ok, msg
        if plan:
            # coll_typed.h's rule for the addresses of this run; the 64-bit walk exactly when forced
            assert comm.get_param("typed_granule") == plan[-1]["G"], (case.what(), plan)
            assert comm.get_param("typed_walk64") - w0 == (len(plan) if meta["force64"] else 0)
        if meta["forms"]:
            x.reset()
            ok, msg = x.run("post")
            assert ok, ("i" + case.kind, msg)
            p = x.init()
            try:
                assert p.kind == 4
                for epoch in (1, 2):
                    x.refill(epoch)
                    torch.cuda.synchronize()
                    p.start()
                    p.wait()
                    ok, msg = x.check()
                    assert ok, (case.kind + "_init", epoch, msg)
            finally:
                p.free()
    finally:
        comm.set_param("blocks", blocks0)
        comm.set_param("typed_force64", 0)
    record(case, plan)
    RAN.add(s)


def test_three_passes_through_the_scratch_half(comm):
    """Both sides typed at N = 1 with more than two scratch halves of packed
    data: alltoall_local_typed packs and unpacks in three passes, the stage
    pointer of pass k being sh.mine - k * scratch.  struct {int, double}
    (12 B packed) in, 4-B blocks at stride 12 out; with the 4 MiB half the
    boundaries 4194304 = 349525 * 12 + 4 and 8388608 = 699050 * 12 + 8 split
    an element and its double.  Once with the 32-bit walk, once forced to the
    64-bit one, where typed_walk64 counts the six launches."""
    import typed_worker as tw
    t0 = time.time()
    half = comm.scratch & ~255
    total = -(-(2 * half + (1 << 20) + 12) // 12) * 12
    assert half != (4 << 20) or total == (9 << 20) + 12
    assert half % 12 and (2 * half) % 12 in (4, 8)       # a boundary inside an element, one inside the double
    st = dd.from_runs("struct", [(0, 4), (8, 8)], 16)
    rt = dd.from_runs("v12", [(0, 4)], 12)
    st.max_count = rt.max_count = None
    case = tr.Case(77, 1, "alltoall", types={(0, 0): ("struct", st), (1, 0): ("v12", rt)},
                   soff=[0], roff=[0], exact=total // 12)
    assert case.B[0][0] == total and -(-total // half) == 3
    x = tw.GenCall(comm, case)
    t1 = time.time()
    try:
        for force64 in (0, 1):
            comm.set_param("typed_force64", force64)
            w0 = comm.get_param("typed_walk64")
            x.reset()
            ok, msg = x.run()
            assert ok, (force64, msg)
            assert comm.get_param("typed_walk64") - w0 == 6 * force64
            assert comm.get_param("typed_granule") == 4
    finally:
        comm.set_param("typed_force64", 0)
    print(f"three passes of {half} B: {time.time() - t1:.3f} s for two calls, {time.time() - t0:.3f} s with the images")
    SEEN["three_passes"] += 1


def test_everything_was_reached(comm):
    """Every granule on both copy directions under both walks; a second trip
    of every granule each way and a third at G = 8; two and three workgroups
    per job and a slice cut inside an element and a run at every granule; a
    search over more than eight elements; every layout class; types below the
    origin; 0 B, 1 B; the three-pass branch."""
    if RAN != set(range(tr.SINGLE_SEEDS)) or not SEEN["three_passes"]:
        pytest.skip("needs the whole module run in this process")
    missing = []
    for G in tr.GS:
        for unpack in (0, 1):
            missing += [k for k in (("G", G, unpack, False), ("G", G, unpack, True), ("trips", G, unpack, 2))
                        if not SEEN[k]]
        missing += [k for k in (("blocks", G, 2), ("blocks", G, 3), ("cut", G)) if not SEEN[k]]
    missing += [k for k in (("trips", 8, 0, 3), ("trips", 8, 1, 3), "many", "below_origin",
                            ("bytes", 0), ("bytes", 1)) if not SEEN[k]]
    missing += [("class", c) for c in ("negstride", "descending", "negdisp", "interleaved", "padded",
                                       "stacked", "g2", "many", "nested") if not SEEN[("class", c)]]
    assert not missing, (missing, dict(SEEN))
