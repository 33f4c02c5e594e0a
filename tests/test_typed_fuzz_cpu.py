"""The inputs of the typed-exchange fuzz (tests/typed_random.py), proved on
the CPU with numpy and the oracle alone: the seed lists that
tests/test_typed_fuzz_gpu.py (N = 1) and tests/typed_worker.py's `layouts`
case (here at N = 2 and 3) run.

Generator properties: receive layouts never overlap, inside a block or between
blocks; every pair's packed bytes are whole elements of both sides; typed
ranges and guards fit the buffers; every class the issue names is in the
lists; the share of rejected datatype draws is under its cap.  The plan of the
N = 1 list (typed_random.single_plan) reaches everything the GPU file's tally
asserts, and no slice of any seed has bytes past its last whole granule (the
tail loop of typed_pipe_copy).

Discrimination: typed_pipe_copy's walk restated in numpy (model_pack) gives the
oracle's packed stream on every seed, and each of six wrong walks changes the
bytes of at least one seed that reaches the code in question.  No GPU."""
import collections

import numpy as np
import pytest

import typed_random as tr
from ddt_random import LAYOUT_CLASSES, all_runs

NS = (2, 3)


@pytest.fixture(scope="module")
def singles():
    st = tr.Stats()
    return [tr.single_case(s, st) for s in range(tr.SINGLE_SEEDS)], st


@pytest.fixture(scope="module")
def workers():
    st = tr.Stats()
    return {n: [tr.worker_case(s, n, path, st) for path in range(3) for s in range(tr.WORKER_SEEDS)]
            for n in NS}, st


def every_case(singles, workers):
    return [c for c, _ in singles[0]] + [c for n in NS for c, _ in workers[0][n]]


def owners(case, side, r):
    """How many runs of how many blocks own each byte of that buffer's [low, high)."""
    t = (case.st, case.rt)[side][r]
    low, high = case.geometry(side, r)
    diff = np.zeros(high - low + 1, dtype=np.int64)
    for base, c in case.blocks(side, r):
        if t is None:
            starts, lens = np.array([base]), np.array([c])
        else:
            starts, lens = all_runs(t, c)
            starts = starts + base
        assert starts.min() >= low and (starts + lens).max() <= high
        np.add.at(diff, starts - low, 1)
        np.add.at(diff, starts + lens - low, -1)
    return np.cumsum(diff)[:-1]


def test_receive_layouts_never_overlap(singles, workers):
    for case in every_case(singles, workers):
        for q in range(case.n):
            if not case.recvs(q):
                continue
            own = owners(case, 1, q)
            assert own.max(initial=0) <= 1, case.what()
            # between blocks: disjoint typed ranges; a byte apart where the test chose the displacements
            rg = sorted(case.ranges(1, q))
            for (_, hi), (lo, _) in zip(rg, rg[1:]):
                assert hi <= lo if case.kind in tr.UNIFORM else hi < lo, case.what()
            t = case.rt[q]
            if t is not None and getattr(t, "max_count", None):
                assert max(case.rc[q]) <= t.max_count, case.what()


def test_pairs_are_whole_elements_and_buffers_hold_them(singles, workers):
    for case in every_case(singles, workers):
        n = case.n
        for p in range(n):
            for q in range(n):
                B = case.B[p][q]
                assert B == case.sc[p][q] * tr.size_of(case.st[p]) == case.rc[q][p] * tr.size_of(case.rt[q])
                assert B == 0 or (case.sends(p) and case.recvs(q))
        for side in (0, 1):
            for r in range(n):
                low, high = case.geometry(side, r)
                assert low <= 0 < high
                for lo, hi in case.ranges(side, r):
                    assert low <= lo and hi <= high
                o = case.origin(side, r)     # the guards: GUARD bytes before low, GUARD after high
                assert o + low == tr.GUARD and case.image_size(side, r) - (o + high) == tr.GUARD
                owners(case, side, r)        # asserts every run lies inside [low, high)
        for q in range(n):                   # the API's displacement of the uniform kinds
            if case.kind in ("alltoall", "gather") and case.recvs(q):
                assert case.rd[q] == [p * case.rc[q][0] for p in range(n)]
            if case.kind in ("alltoall", "scatter") and case.sends(q):
                assert case.sd[q] == [p * case.sc[q][0] for p in range(n)]


def classes_of(cases):
    seen = collections.Counter()
    for case in cases:
        for (side, r), cls in case.cls.items():
            t = (case.st, case.rt)[side][r]
            if t is None or not case.blocks(side, r):
                continue
            seen[cls] += 1
            seen["many"] += len(t.elems) > 8
            seen["below_origin"] += case.geometry(side, r)[0] < 0
            seen["off16"] += (case.soff, case.roff)[side][r] % 16 != 0
            seen["zero_extent"] += t.extent == 0
            seen["sub_run_extent"] += 0 < t.extent < max(n for _, n in t.runs)
            seen["wide_extent"] += t.extent > 4 * max(t.true_span, 1)
            for g in case.side_granules(side, r):
                seen[f"G{g}"] += 1
    return seen


WANTED = [c for c in LAYOUT_CLASSES if c != "backward"] + \
    ["g2", "many", "below_origin", "off16", "zero_extent", "wide_extent"] + [f"G{g}" for g in tr.GS]


def test_every_class_is_in_the_seed_lists(singles, workers):
    seen = classes_of([c for c, _ in singles[0]])
    assert all(seen[k] >= 1 for k in WANTED + ["sub_run_extent"]), seen
    for n in NS:
        seen = classes_of([c for c, _ in workers[0][n]])
        assert all(seen[k] >= 1 for k in WANTED), (n, seen)
        kinds = {c.kind for c, _ in workers[0][n]}
        assert kinds == set(tr.KINDS)
        assert any(c.inplace for c, _ in workers[0][n])
        assert any(0 in sum(c.B, []) and c.kind == "alltoallv" for c, _ in workers[0][n])
        # ranks of one call differ in their datatypes
        assert any(len({id(t) for t in c.rt}) > 1 for c, _ in workers[0][n])
    roots = {(c.kind, c.root) for c, _ in workers[0][3]}
    assert all((k, r) in roots for k in tr.ROOTED for r in range(3)), roots


def test_rejected_draws_stay_under_a_quarter(singles, workers):
    """A draw is thrown away when its class is not legal for the side (a
    negative extent anywhere, overlapping instances on a receive side), when
    one element packs to more than MAX_SIZE, or when the unit of its pair
    (group) would pass MAX_LCM.  The fixed lists need 21 redraws in 201 draws
    at N = 1, 37 in 157 at N = 2 and 3 together, 23 in 119 at N = 4 and 49 in
    241 at N = 8; the cap is a quarter."""
    lists = [singles[1], workers[1]]
    for n in (4, 8):
        lists.append(tr.Stats())
        for path in range(3):
            for s in range(tr.WORKER_SEEDS):
                tr.worker_case(s, n, path, lists[-1])
    for st in lists:
        print(f"draws {st.draws}, rejected {st.rejected}")
        assert 4 * st.rejected <= st.draws, (st.rejected, st.draws)


def test_single_plan_reaches_what_the_gpu_tally_asserts(singles):
    seen = collections.Counter()
    for case, meta in singles[0]:
        for e in tr.single_plan(case, meta):
            G = e["G"]
            seen[("G", G, e["unpack"], e["w64"])] += 1
            seen[("trips", G, e["unpack"], min(e["trips"], 3))] += 1
            seen[("blocks", G, min(e["blocks"], 3))] += 1
            seen[("cut", G)] += e["cut_elem"] and e["cut_run"]
            seen["many"] += e["nelems"] > 8
        # 2047 / 2048 / 2049 granules of the G aimed at
        if meta["size"] in tr.EDGE:
            assert case.B[0][0] == tr.EDGE[meta["size"]] * meta["aim"]
            assert all(e["G"] == meta["aim"] for e in tr.single_plan(case, meta)), case.what()
    for G in tr.GS:
        for unpack in (0, 1):
            assert seen[("G", G, unpack, False)] and seen[("G", G, unpack, True)], (G, unpack)
            assert seen[("trips", G, unpack, 2)], (G, unpack)
        assert seen[("blocks", G, 2)] and seen[("blocks", G, 3)] and seen[("cut", G)], G
    assert seen[("trips", 8, 0, 3)] and seen[("trips", 8, 1, 3)] and seen["many"]
    sizes = {case.B[0][0] for case, _ in singles[0]}
    assert 0 in sizes and 1 in sizes


def test_no_legal_call_reaches_the_tail_loop(singles):
    """typed_pipe_copy moves (hi - lo) / G granules and then, bytewise, what is
    left.  hi - lo is a multiple of G on every slice: lo is a multiple of 16
    (a2a_slice's `per`, a pass boundary of 256 k), hi is such a cut or the
    pair's end, and G divides the datatype's granule, which divides every run
    and so the size and the pair."""
    for case, meta in singles[0]:
        B = case.B[0][0]
        for e in tr.single_plan(case, meta):
            for g in range(e["blocks"]):
                lo, hi = tr.a2a_slice(B, g, e["blocks"])
                assert lo % 16 == 0 and (hi - lo) % e["G"] == 0, case.what()


# ---- the walk restated, and six wrong ones --------------------------------------
def walk(t, G, first, ng, wrong=None):
    """typed_offset_fast<G> of granules first .. first + ng of the packed stream."""
    c, bl, st, d = (np.array(x, dtype=np.int64) for x in zip(*t.elems))
    st = np.where(c > 1, st, bl)
    if wrong == "abs_stride":
        st = np.abs(st)
    prefix = np.concatenate([[0], np.cumsum(c * bl)[:-1]])
    pg = first + np.arange(ng, dtype=np.int64)
    size_g = t.size // G
    el = pg // size_g
    q = pg - el * size_g
    i = np.searchsorted(prefix, q * G, side="right") - 1
    r = q - prefix[i] // G
    k = r // (bl[i] if wrong == "byte_divide" else bl[i] // G)
    w = r - k * (bl[i] // G)
    return el * t.extent + d[i] + k * st[i] + w * G


def model_pack(case, e, oracle, wrong=None):
    """The packed stream the N = 1 call's pack launch writes (plan entry e),
    over a destination of other random bytes."""
    t, B, G = case.st[0], case.B[0][0], e["G"]
    img = case.send_image(0)
    base = case.origin(0, 0) + case.sd[0][0] * t.extent
    out = np.random.default_rng(7).integers(0, 256, B, dtype=np.uint8)
    for g in range(e["blocks"]):
        lo, hi = tr.a2a_slice(B, g, e["blocks"])
        ng = (hi - lo) // G
        offs = walk(t, G, (0 if wrong == "job_lo" else lo) // G, ng, wrong)
        j = np.arange(ng)
        if wrong == "one_trip":
            j = j[j < tr.TRIP]
        idx = (base + offs[j])[:, None] + np.arange(G)[None, :]
        out[lo:lo + ng * G].reshape(ng, G)[j] = img.take(idx, mode="wrap")
    return out


def test_inputs_catch_wrong_walks(orc, singles, workers):
    """Each wrong walk changes the bytes of a seed that reaches it: the
    stride's sign dropped, runs in address order, the block-length divide in
    bytes instead of granules, a slice's second trip skipped, a workgroup's
    slice started at the job's lo, and the SENDER's receive datatype used to
    unpack."""
    differs = collections.Counter()
    for case, meta in singles[0]:
        plan = [e for e in tr.single_plan(case, meta) if not e["unpack"]]
        if not plan:
            continue
        e, t = plan[0], case.st[0]
        right = case.packed(0, 0, orc)
        assert np.array_equal(model_pack(case, e, orc), right), case.what()
        for wrong in ("abs_stride", "byte_divide", "one_trip", "job_lo"):
            if wrong == "job_lo" and t.extent == 0:
                continue   # every instance at one address: the stream is periodic in the slice width
            differs[wrong] += not np.array_equal(model_pack(case, e, orc, wrong), right)
        by_address = orc.pack(sorted(t.runs), t.extent, case.sc[0][0], case.send_image(0)[
            case.origin(0, 0) + case.sd[0][0] * t.extent:], 0, case.B[0][0])
        differs["address_order"] += not np.array_equal(by_address, right)
        differs[("one_trip", e["G"])] += e["trips"] > 1
        differs[("job_lo", e["G"])] += e["blocks"] > 1 and t.extent > 0
    for n in NS:
        for case, _ in workers[0][n]:
            for q in range(n):
                if case.recvs(q) and not np.array_equal(
                        case.expected(q, orc), case.expected(q, orc, recv_type_of=lambda p, q: case.rt[p])):
                    differs[("senders_type", n)] += 1
    print(dict(differs))
    assert all(differs[k] >= 3 for k in ("abs_stride", "byte_divide", "address_order")), differs
    # every seed with a second trip / a second workgroup shows the mistake
    assert differs["one_trip"] == sum(differs[("one_trip", G)] for G in tr.GS) >= 10, differs
    assert differs["job_lo"] == sum(differs[("job_lo", G)] for G in tr.GS) >= 10, differs
    assert all(differs[("senders_type", n)] >= 5 for n in NS), differs
