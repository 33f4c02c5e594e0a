"""ompi_amd_ddt_sndrcv: one kernel walks both datatypes.  The reference is p2p_typed_worker.py's
numpy pack / unpack into a sentinel-filled buffer; whole buffers are compared; each case asserts its counters."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gather_worker import Buf, PREFILL  # noqa: E402
from p2p_typed_worker import image, offs, span, types  # noqa: E402

# name: send, receive (type, count), receive base offset, (launches, both in LDS, 64-bit walk) moved, granule
CASES = [
    ("g16_into_g4", ("v16", 64), ("s16", 256), 0, (1, 1, 0), 4, {}),           # 4096 B
    ("many_groups", ("v8", 26215), ("w16", 32769), 8, (1, 1, 0), 8, {}),       # 1 MiB + 24, ends 8 B into a run
    ("byte_walk", ("idx", 410), ("v2", 2050), 0, (1, 1, 0), 1, {}),            # G 1 against G 2
    ("partial", ("s12", 5461), ("s24", 4096), 0, (1, 1, 0), 4, {}),            # 65532 B end inside an s24
    ("global_walk", ("big", 17), ("big2", 17), 0, (1, 0, 0), 1, {}),           # 300 + 300 elements
    ("one_global", ("big", 17), ("v4", 2040), 0, (1, 0, 0), 1, {}),            # 300 + 1: the larger stays out
    ("force64", ("v64", 512), ("v4", 2048), 0, (1, 1, 1), 4, {"force64": True}),
    ("truncate", ("v64", 512), ("v64b", 500), 0, (1, 1, 0), 4, {"truncate": True}),
    ("same_program", ("v8", 100), ("v8", 100), 8, (1, 1, 0), 8, {}),           # one program, two bases
    ("bytes_to_typed", (None, 4100), ("v2", 410), 0, (0, 0, 0), None, {}),
    ("typed_to_bytes", ("idx", 410), (None, 4100), 0, (0, 0, 0), None, {}),
    ("bytes_to_bytes", (None, 4100), (None, 4100), 0, (0, 0, 0), None, {}),
]


@pytest.fixture(scope="module")
def T():
    t, again = types(), types()
    t["big2"], t["v64b"] = again["big"], again["v64"]  # equal layouts, programs of their own
    return t


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_ddt_sndrcv(T, case):
    from ompi_amd import _lib, datatype as dt
    name, (st, sc), (rt, rc), roff, moved, gran, opt = case
    st, rt = T.get(st), T.get(rt)
    src = image(0, len(name), span(st, sc))
    sbuf, rbuf = Buf(src, 0), Buf(np.full(span(rt, rc), PREFILL, np.uint8), roff)
    stream, want = src[offs(st, sc)], np.full(rbuf.n, PREFILL, np.uint8)
    at = offs(rt, rc)[:stream.size]
    want[at] = stream[:at.size]
    rbuf.expect(want)
    before = _lib.ddt_sndrcv_counts()
    _lib.load().ompi_amd_ddt_sndrcv_force64(int(bool(opt.get("force64"))))
    try:
        dt.sndrcv(sbuf.ptr, sc, st, rbuf.ptr, rc, rt)
        assert not opt.get("truncate"), "a longer send side must not pass"
    except _lib.OmpiAmdError as e:
        assert opt.get("truncate") and e.code == _lib.ERR_TRUNCATE, e
    finally:
        _lib.load().ompi_amd_ddt_sndrcv_force64(0)
    torch.cuda.synchronize()
    for ok, msg in (rbuf.check("rbuf"), sbuf.check("sbuf")):
        assert ok, (name, msg)
    after = _lib.ddt_sndrcv_counts()
    got = tuple(after[k] - before[k] for k in ("launches", "both_lds", "walk64"))
    assert got == moved, f"{name}: (launches, both_lds, walk64) moved by {got}, expected {moved}"
    assert gran is None or after["granule"] == gran, (name, after["granule"])


def test_ddt_sndrcv_refusals(T):
    """BAD_PARAM for a host pointer, a negative extent, an overflow, a NULL buffer; no counter moves."""
    from ompi_amd import _lib, datatype as dt
    buf, host = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.uint8)
    V = dt.from_runs("v12", [(0, 4)], 12)  # (named: a Datatype destroys its program when collected)
    NEG = dt.type_create_resized(V, 0, -12)
    (v, neg), d, hp = (t.commit()._handle for t in (V, NEG)), buf.data_ptr(), host.data_ptr()
    before = (_lib.ddt_sndrcv_counts(), _lib.ddt_route_counts())
    for args in [(hp, 3, v, d, 3, v), (d, 3, v, hp, 3, v), (hp, 12, None, d, 12, None), (d, 3, neg, d + 4096, 3, v),
                 (d, 3, v, d + 4096, 3, neg), (d, 1 << 62, v, d + 4096, 3, v), (d, 3, v, d + 4096, 1 << 62, v),
                 (None, 3, v, d, 3, v), (d, 3, v, None, 3, v)]:
        assert _lib.load().ompi_amd_ddt_sndrcv(*args, None) == _lib.ERR_BAD_PARAM, args
    assert (_lib.ddt_sndrcv_counts(), _lib.ddt_route_counts()) == before
    assert _lib.load().ompi_amd_ddt_sndrcv(None, 0, neg, d, 3, v, None) == 0  # count 0: no datatype, no buffer
