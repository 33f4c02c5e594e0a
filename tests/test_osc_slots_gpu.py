"""Every (op, type) slot of the one-sided accumulate kernels against the
oracle (ompi_amd/csrc/osc_ipc.hip: g_acc / acc_kernel, g_rma_small /
rma_small_kernel, g_ddt_acc / ddt_acc_kernel, pair_fn_of / ddt_pair_kernel),
one item per slot, on a communicator of one rank whose target is this GPU.

The cases, their counts and their expectations are tests/osc_slot_cases.py
(the paths a, b, c, d, p, w of its header); tests/test_osc_slots_cpu.py
shows that their inputs tell a kernel that does nothing, copies, or swaps
its operands from a right one.  Accumulated elements are compared with
same_bits (NaN payloads free where both are NaN); fetched elements and
every byte that is no member of an operated element — the window before the
displacement, the guard bytes after it, the bytes between the runs of a
derived target — byte for byte; on the pair kernel's path the whole window,
gap bytes of the pairs included.

All values here are measured on one GPU (target = origin device), not
across xGMI."""
import numpy as np
import pytest

import osc_slot_cases as sc
from ompi_amd import coll, osc
from ompi_amd import op as mop
from oracle import oracle as _orc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOT_LIST = sc.slots(_orc)


@pytest.fixture(scope="module")
def comm():
    c = coll.Communicator(f"oscslots_{np.random.randint(1 << 30)}", 0, 1, 0)
    yield c
    c.free()


@pytest.fixture(scope="module")
def window(orc, comm):
    """One window for the module: each case refills the bytes it uses."""
    nbytes = sc.window_bytes(orc)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert buf.data_ptr() % 16 == 0
    win = osc.Window.create(comm, buf, nbytes, disp_unit=1)
    yield buf, win
    win.free()


def dev(a: np.ndarray):
    t = torch.from_numpy(a).to(DEV)
    assert t.data_ptr() % 16 == 0
    return t


def check_table(case, tl):
    """The element table sits where the case means it to."""
    if case.tkind in ("vector", "wrap"):
        assert tl.ddt.nelems == 1, (case.name, tl.ddt.nelems)
    elif case.tkind == "indexed":
        assert 1 < tl.ddt.nelems <= sc.K_DDT_LDS_ELEMS, (case.name, tl.ddt.nelems)
    elif case.tkind == "long":
        assert tl.ddt.nelems > sc.K_DDT_LDS_ELEMS, (case.name, tl.ddt.nelems)


def run_case(orc, window, case, dt):
    """None, or what differs."""
    wbuf, win = window
    b = sc.build(orc, case, dt)
    tl, ol, rl = sc.case_layouts(case, dt)
    n, e = case.n, dt.extent
    W = b.win0.nbytes
    assert W <= wbuf.numel()
    wbuf[:W].copy_(torch.from_numpy(b.win0))
    org = dev(b.origin) if b.origin is not None else None
    res = dev(b.result0) if b.result0 is not None else None
    optr = org.data_ptr() + case.ooff if org is not None else None
    rptr = res.data_ptr() + case.roff if res is not None else None
    if tl is not None and not sc.is_pair(dt):  # ddt_pair_kernel reads its table in global memory
        check_table(case, tl)
    side = lambda lay: (lay.count, lay.ddt) if lay is not None else (n, None)  # noqa: E731
    win.lock(0, osc.LOCK_EXCLUSIVE)
    if case.call == "acc":
        win.accumulate(optr, n, dt, 0, case.disp, case.op)
    elif case.call == "gacc":
        win.get_accumulate(optr, rptr, n, dt, 0, case.disp, case.op)
    elif case.call == "fop":
        for i in case.picks:
            win.fetch_and_op(optr + i * e, rptr + i * e, dt, 0, case.disp + i * e, case.op)
    elif case.call == "acc_ddt":
        win.accumulate_ddt(optr, *side(ol), 0, case.disp, *side(tl), dt, case.op)
    else:
        win.get_accumulate_ddt(optr, *side(ol), rptr, *side(rl), 0, case.disp, *side(tl), dt, case.op)
    win.unlock(0)
    win.sync()
    torch.cuda.synchronize()
    got = wbuf[:W].cpu().numpy()
    m = sc.N_SINGLE if case.path == "c1" else n
    if not sc.same_bits(sc.extract(orc, tl, dt, got, case.disp, m),
                        sc.extract(orc, tl, dt, b.win_exp, case.disp, m), dt):
        ge = sc.to_stream(dt, sc.extract(orc, tl, dt, got, case.disp, m)).reshape(m, -1)
        ee = sc.to_stream(dt, sc.extract(orc, tl, dt, b.win_exp, case.disp, m)).reshape(m, -1)
        bad = np.flatnonzero((ge != ee).any(axis=1))
        return f"{len(bad)} of {m} target elements differ, first at element {bad[:1]}"
    rest = ~b.touched & ~b.wfree
    bad = np.flatnonzero((got != b.win_exp) & (rest if not case.exact else True))
    if bad.size:
        return f"window byte {bad[0]} of {W} changed ({bad.size} bytes; the target starts at {case.disp})"
    if case.fetch:
        gr = res.cpu().numpy()
        bad = np.flatnonzero((gr != b.result_exp) & ~b.rfree)
        if bad.size:
            kind = "fetched" if b.rtouched[bad[0]] else "untouched"
            return f"result byte {bad[0]} ({kind}) differs ({bad.size} bytes; the result starts at {case.roff})"
    return None


@pytest.mark.parametrize("op,dt", SLOT_LIST, ids=[sc.slot_id(o, d) for o, d in SLOT_LIST])
def test_slot(orc, window, op, dt):
    assert mop.supported(op, dt)
    failed = []
    for case in sc.cases_for(orc, op, dt):
        why = run_case(orc, window, case, dt)
        if why:
            failed.append(f"[{case.path}] {case.name} (n={case.n}, {case.op.name}): {why}")
    assert not failed, f"{sc.slot_id(op, dt)}: {len(failed)} cases differ from the oracle:\n" + "\n".join(failed)
