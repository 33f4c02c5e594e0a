"""The convertor's environment settings, each in a fresh process
(tests/ddt_knob_worker.py: the library reads them once).  Every worker must
match the oracle byte for byte on every layout, and its route counters must
show that the setting took effect — a settings test that stayed on the
default route would prove nothing."""
import pytest

from ddt_knob_worker import run_worker

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TILES = {"tile_pack_ident", "tile_pack_map", "tile_unpack_ident", "tile_unpack_map",
         "iov_tile_ident", "iov_tile_map"}
MULTI = ("struct_int_double", "blacs", "indexed9", "indexed300", "descending")


def worker(env):
    lines = run_worker(env)
    bad = [(ln["case"], ln.get("size"), ln.get("bad")) for ln in lines if not ln["ok"]]
    assert not bad, bad
    cases = [ln for ln in lines if ln["case"] != "totals"]
    assert len(cases) == 2 * 12, [ln["case"] for ln in cases]
    return cases, lines[-1]["routes"]


def ops_of(cases, name):
    out = [ln["ops"] for ln in cases if ln["case"] == name]
    assert len(out) == 2, name
    return out


def test_fastdiv():
    """OMPI_AMD_DDT_FASTDIV=1: the multi-element layouts the tile does not
    take go through the 32-bit multiply-high search, none through the 64-bit."""
    cases, totals = worker({"OMPI_AMD_DDT_FASTDIV": "1"})
    for name in ("indexed9", "indexed300"):
        for ops in ops_of(cases, name):
            assert "generic32" in ops["pack"] and "generic32" in ops["unpack"], (name, ops)
    assert totals["generic32"] > 0 and totals["generic64"] == 0, totals


def test_fastdiv_without_tile():
    """… and with OMPI_AMD_DDT_TILE=0 the large windows of every
    multi-element layout reach it."""
    cases, totals = worker({"OMPI_AMD_DDT_FASTDIV": "1", "OMPI_AMD_DDT_TILE": "0"})
    for name in MULTI:
        for ops in ops_of(cases, name):
            assert ops["pack"] == ["generic32"] and ops["unpack"] == ["generic32"], (name, ops)
            assert ops["iov_pack"] == ["iov_generic"], (name, ops)
    assert totals["generic64"] == 0 and not [r for r in TILES if totals[r]], totals


def test_tile_off():
    """OMPI_AMD_DDT_TILE=0: no tile route at all; the walkers and the 64-bit
    search move the large periodic windows."""
    cases, totals = worker({"OMPI_AMD_DDT_TILE": "0"})
    assert not [r for r in TILES if totals[r]], totals
    assert totals["generic64"] and totals["vec16"] and totals["vec_g"] and totals["iov_generic"], totals
    for ops in ops_of(cases, "vector_bl1_gap8"):
        assert ops["pack"] == ["vec_g"] and ops["unpack"] == ["vec_g"], ops


def test_tile_wide_off():
    """OMPI_AMD_DDT_TILE_WIDE=0: single-run vectors at a 16-B granule take
    the 16-B walk, the sub-16-B ones still take the tile."""
    cases, _ = worker({"OMPI_AMD_DDT_TILE_WIDE": "0"})
    for name in ("vector_bl2_gap64", "vector_bl8_gap512", "vector_bl64_gap512"):
        for ops in ops_of(cases, name):
            assert ops["pack"] == ["vec16"] and ops["unpack"] == ["vec16"], (name, ops)
    for ops in ops_of(cases, "vector_bl1_gap8"):
        assert "tile_pack_ident" in ops["pack"] and "tile_unpack_ident" in ops["unpack"], ops
    for ops in ops_of(cases, "struct_int_double"):
        assert "tile_pack_map" in ops["pack"] and "tile_unpack_map" in ops["unpack"], ops


@pytest.mark.parametrize("nbytes", [4096, 60 << 10])
def test_tile_bytes(nbytes):
    """OMPI_AMD_DDT_TILE_BYTES at both accepted ends: the tile launches ask
    for LDS of that order (16 KiB by default), within a workgroup's 160 KiB."""
    cases, totals = worker({"OMPI_AMD_DDT_TILE_BYTES": str(nbytes)})
    assert totals["tile_pack_ident"] and totals["tile_pack_map"] and totals["iov_tile_map"], totals
    lds = [ln["lds"]["pack"] for ln in cases if "tile_pack_ident" in ln["ops"]["pack"]]
    assert lds and all(nbytes - 1024 <= x <= nbytes + 64 for x in lds), lds
    lds = [ln["lds"][op] for ln in cases for op in ln["ops"] if set(ln["ops"][op]) & TILES]
    assert lds and max(lds) <= 160 << 10, lds


@pytest.mark.parametrize("nbytes", [1024, 128 << 10])
def test_unpack_tile_bytes(nbytes):
    """OMPI_AMD_DDT_UNPACK_TILE_BYTES at both accepted ends (the upper one
    was 1 MiB, which no workgroup's LDS holds: ddt_plan.h)."""
    cases, totals = worker({"OMPI_AMD_DDT_UNPACK_TILE_BYTES": str(nbytes)})
    assert totals["tile_unpack_ident"] and totals["tile_unpack_map"], totals
    lds = [ln["lds"]["unpack"] for ln in cases if "tile_unpack_ident" in ln["ops"]["unpack"]]
    assert lds and all(nbytes - 1024 <= x <= nbytes + 64 for x in lds), lds
    lds = [ln["lds"]["pack"] for ln in cases if "tile_pack_ident" in ln["ops"]["pack"]]
    assert lds and all((15 << 10) <= x <= (16 << 10) + 64 for x in lds), lds   # the pack keeps its own


@pytest.mark.parametrize("nt", [0, 1])
def test_unpack_nt(nt):
    """OMPI_AMD_DDT_UNPACK_NT forced off and on: the same bytes either way,
    on the tile (the 512-B-gap vectors' unpack included, by default)."""
    cases, totals = worker({"OMPI_AMD_DDT_UNPACK_NT": str(nt)})
    assert totals["tile_unpack_ident"] and totals["tile_unpack_map"], totals
    for name in ("vector_bl8_gap512", "vector_bl64_gap512"):
        for ops in ops_of(cases, name):
            assert ops["unpack"][0] == "tile_unpack_ident", (name, ops)


@pytest.mark.parametrize("gap", [0, 128])
def test_run_maxgap(gap):
    """OMPI_AMD_DDT_RUN_MAXGAP=0 / 128: the 512-B-gap vectors' unpack leaves
    the tile for the 16-B walk."""
    cases, _ = worker({"OMPI_AMD_DDT_RUN_MAXGAP": str(gap)})
    for name in ("vector_bl8_gap512", "vector_bl64_gap512"):
        for ops in ops_of(cases, name):
            assert ops["unpack"] == ["vec16"] and ops["iov_unpack"] == ["iov_generic"], (name, ops)
    for ops in ops_of(cases, "vector_bl1_gap8"):
        want = ["vec_g"] if gap == 0 else ["tile_unpack_ident"]
        assert ops["unpack"][:1] == want, ops
