"""The case table of tests/osc_slot_cases.py, checked without a GPU: it
covers exactly the slots the oracle defines, its shape constants are the
source's, and its inputs discriminate — at every count the GPU test runs,
the oracle's result is neither the untouched target nor a plain replace
nor, for the order-sensitive slots, f(origin, target).  Without that the
GPU test could pass on a kernel that does nothing, copies, or swaps its
operands."""
import os
import re
from collections import Counter

import numpy as np
import pytest

import osc_slot_cases as sc
from ompi_amd import op as mop
from oracle import oracle as _orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT_LIST = sc.slots(_orc)
IDS = [sc.slot_id(o, d) for o, d in SLOT_LIST]


def family(dt) -> str:
    if sc.is_pair(dt):
        return "pair"
    if dt.code in sc.FP_CODES:
        return "fp"
    if dt in (mop.MPIX_C_FLOAT16_COMPLEX, mop.MPI_C_FLOAT_COMPLEX, mop.MPI_C_DOUBLE_COMPLEX):
        return "complex"
    if dt is mop.MPI_C_BOOL:
        return "bool"
    if dt is mop.MPI_BYTE:
        return "byte"
    return "int"


def test_table_is_the_defined_slots(orc):
    for op, dt in sc.SLOTS:
        assert orc.defined(op.index, dt.code) == mop.supported(op, dt), (op.name, dt.name)
    assert len(SLOT_LIST) == 114 and len(set(IDS)) == 114
    assert Counter(family(dt) for _, dt in SLOT_LIST) == {
        "int": 80, "fp": 12, "complex": 6, "bool": 3, "byte": 3, "pair": 10}
    for op, dt in SLOT_LIST:
        paths = Counter(c.path for c in sc.cases_for(orc, op, dt))
        want = ["a", "b", "c1", "c", "p" if sc.is_pair(dt) else "d"]
        assert all(paths[p] > 0 for p in want), (op.name, dt.name, paths)
        assert (paths["w"] > 0) == ((op.index, dt.code) in sc.WRAP_SLOTS)
    # the cases that depend on the element size only run once per size
    sizes = Counter(dt.extent for op, dt in SLOT_LIST if sc.first_of_size(orc, op, dt))
    assert sizes == {1: 1, 2: 1, 4: 1, 8: 1, 16: 1}
    assert sum((o.index, d.code) in sc.WRAP_SLOTS for o, d in SLOT_LIST) == 4


def test_order_sensitive_slots(orc):
    got = {(o.name, d.name) for o, d in SLOT_LIST if sc.order_sensitive(o, d)}
    fp = ("MPIX_C_FLOAT16", "MPI_FLOAT", "MPI_DOUBLE")
    assert got == {(o, d) for o in ("MPI_MAX", "MPI_MIN") for d in fp} | {
        (o, d) for o in ("MPI_MAXLOC", "MPI_MINLOC") for d in ("MPI_FLOAT_INT", "MPI_DOUBLE_INT")}


@pytest.mark.parametrize("op,dt", SLOT_LIST, ids=IDS)
def test_inputs_discriminate(orc, op, dt):
    seen = set()
    for c in sc.cases_for(orc, op, dt):
        if c.op is not op or (c.n, c.seed) in seen:
            continue
        seen.add((c.n, c.seed))
        what = f"{sc.slot_id(op, dt)} {c.name} n={c.n}"
        if c.path == "c1":
            o, t = sc.inputs(dt, sc.N_SINGLE, c.seed)
            assert 1 <= len(c.picks) <= 3, what
            flags = [sc.discriminates(orc, op, dt, o[i:i + 1], t[i:i + 1]) for i in c.picks]
            moved, not_copied, ordered = (any(f[k] for f in flags) for k in range(3))
        else:
            o, t = sc.case_inputs(orc, c, dt)
            moved, not_copied, ordered = sc.discriminates(orc, op, dt, o, t)
            edges = sc.edge_elements(dt, c.n)
            assert edges[0] == 0 and edges[-1] == c.n - 1
            res = sc.apply_op(orc, op, dt, o, t)
            for i in edges:
                assert not sc.same_bits(res[i:i + 1], t[i:i + 1], dt), \
                    f"{what}: element {i} (a loop edge) keeps the target's value"
        assert moved, f"{what}: the result is the untouched target"
        assert not_copied, f"{what}: the result is a plain replace"
        if sc.order_sensitive(op, dt):
            assert ordered, f"{what}: f(origin, target) gives the same result"
    assert len(seen) >= 8


@pytest.mark.parametrize("dt", [mop.MPI_LONG_INT, mop.MPI_2INT, mop.MPI_SHORT_INT],
                         ids=lambda d: d.name)
@pytest.mark.parametrize("op", [mop.MPI_MAXLOC, mop.MPI_MINLOC], ids=lambda o: o.name)
def test_integer_pairs_commute(orc, op, dt):
    """Why the integer pair slots are not order-sensitive: on every value
    pair of a small range and every index order, LOC_FUNC gives the same
    members for f(target, origin) and f(origin, target)."""
    vals = np.arange(-3, 4)
    x = np.zeros(len(vals) ** 2 * 3, dtype=dt.np_dtype)
    y = np.zeros_like(x)
    g = np.array([(a, b, ka, kb) for a in vals for b in vals for ka, kb in ((1, 2), (2, 1), (5, 5))])
    x["v"], y["v"], x["k"], y["k"] = g[:, 0], g[:, 1], g[:, 2], g[:, 3]
    assert sc.same_bits(sc.apply_op(orc, op, dt, x, y), sc.apply_op(orc, op, dt, y, x), dt)


def test_shape_constants_match_the_source():
    src = {}
    for path in ("ompi_amd/csrc/osc_ipc.hip", "ompi_amd/csrc/ddt_device.h"):
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        for m in re.finditer(r"constexpr\s+(?:int|size_t|int64_t)\s+(k\w+)\s*=\s*([^;]+);", text):
            src[m.group(1)] = m.group(2).strip()

    def value(name):
        assert name in src, f"{name} is gone from the source: revisit tests/osc_slot_cases.py"
        expr = src[name]
        assert re.fullmatch(r"[\d\s<*()+]+", expr), f"{name} = {expr}: not a plain constant any more"
        return eval(expr)  # digits, <<, *, + and parentheses only

    revisit = {
        "kRmaSmallBytes": (sc.K_RMA_SMALL_BYTES, "n_small (the case c boundary counts)"),
        "kOscThreads": (sc.K_OSC_THREADS, "N_VECS, N_DDT, N_PAIR and the wrap counts"),
        "kOscUnroll": (sc.K_OSC_UNROLL, "N_VECS and N_WRAP_VECS"),
        "kAccUnroll": (sc.K_ACC_UNROLL, "N_DDT and N_WRAP_DDT"),
        "kOscMaxBlocks": (sc.K_OSC_MAX_BLOCKS, "N_WRAP_VECS, N_WRAP_ELEMS and N_WRAP_DDT"),
        "kDdtLdsElems": (sc.K_DDT_LDS_ELEMS, "the run count of layout('long')"),
    }
    for name, (mine, counts) in revisit.items():
        assert value(name) == mine, (
            f"{name} is {value(name)} in the source, {mine} in tests/osc_slot_cases.py: revisit {counts}")
    # the counts reach what they are meant to reach
    assert sc.N_VECS > sc.K_OSC_THREADS * sc.K_OSC_UNROLL and sc.N_VECS % sc.K_OSC_THREADS != 0
    assert sc.N_DDT > sc.K_OSC_THREADS * sc.K_ACC_UNROLL
    assert sc.N_PAIR > sc.K_OSC_THREADS
    for e in (1, 2, 4, 8, 16):
        assert sc.n_vec(e) * e > sc.K_RMA_SMALL_BYTES  # case a / b: past the one-launch path
        assert sc.n_small(e) * e == sc.K_RMA_SMALL_BYTES
        assert (sc.n_vec(e) + sc.K_OSC_THREADS - 1) // sc.K_OSC_THREADS >= 4  # case b workgroups
    assert sc.N_WRAP_VECS > sc.K_OSC_MAX_BLOCKS * sc.K_OSC_THREADS * sc.K_OSC_UNROLL
    assert sc.N_WRAP_ELEMS > sc.K_OSC_MAX_BLOCKS * sc.K_OSC_THREADS
    assert sc.N_WRAP_DDT > sc.K_OSC_MAX_BLOCKS * sc.K_OSC_THREADS * sc.K_ACC_UNROLL


def test_expectation_builder_round_trips(orc):
    """build() on a derived pair case: the expected window differs from the
    window before only in member bytes of the typemap, and extracting the
    target elements from it gives the oracle's result."""
    op, dt = mop.MPI_MINLOC, mop.MPI_SHORT_INT
    case = next(c for c in sc.cases_for(orc, op, dt) if c.path == "p" and c.tkind == "split"
                and c.op is op and c.fetch)
    b = sc.build(orc, case, dt)
    tl, _, rl = sc.case_layouts(case, dt)
    changed = b.win0 != b.win_exp
    assert changed.any() and not (changed & ~b.touched).any()
    assert b.touched.sum() == case.n * dt.size and not b.wfree.any()
    o, t = sc.case_inputs(orc, case, dt)
    got = sc.extract(orc, tl, dt, b.win_exp, case.disp, case.n)
    assert sc.same_bits(got, sc.apply_op(orc, op, dt, o, t), dt)
    assert sc.same_bits(sc.extract(orc, rl, dt, b.result_exp, case.roff, case.n), t, dt)
    assert b.rtouched.sum() == case.n * dt.size
