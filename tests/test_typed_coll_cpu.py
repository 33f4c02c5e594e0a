"""CPU checks of the typed exchange collectives: the 21 entry points are
exported with the header's signatures, and the granule / walk rule of
ompi_amd/csrc/coll_typed.h agrees with a brute-force statement of it."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np

from ompi_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("alltoall", "alltoallv", "allgatherv", "gather", "scatter", "gatherv", "scatterv")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

C = ctypes
CTYPES = {
    "ompi_amd_comm_t *": C.c_void_p, "const void *": C.c_void_p, "void *": C.c_void_p,
    "const ompi_amd_ddt_t *": C.c_void_p, "size_t": C.c_size_t, "int": C.c_int,
    "const size_t *": C.POINTER(C.c_size_t), "ompi_amd_request_t **": C.POINTER(C.c_void_p),
    "ompi_amd_plan_t **": C.POINTER(C.c_void_p),
}


def header_prototypes():
    """name -> [ctypes of the parameters], from the preprocessed header (the
    typed forms are declared through a macro)."""
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no host C compiler"
    out = subprocess.run([cc, "-E", "-P", os.path.join(ROOT, "include", "ompi_amd_coll.h")],
                         capture_output=True, text=True, check=True).stdout
    protos = {}
    for m in re.finditer(r"\bint\s+(ompi_amd_\w*_typed\w*)\s*\(([^)]*)\)\s*;", out):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            kind = re.sub(r"\s*\b\w+$", "", p) if not p.endswith("*") else p  # drop the parameter name
            kind = re.sub(r"\s*\*\s*", " *", kind).replace("* *", "**").strip()
            params.append(CTYPES[kind])
        protos[m.group(1)] = params
    return protos


def test_typed_symbols_match_header():
    want = {f"ompi_amd_{pre}{n}_typed{post}" for n in NAMES for pre, post in (("", ""), ("i", ""), ("", "_init"))}
    protos = header_prototypes()
    assert set(protos) == want, set(protos) ^ want
    lib = _lib.load()
    table = {p[0]: p for p in _lib.PROTOTYPES}
    for name, params in protos.items():
        assert hasattr(lib, name), name
        assert table[name][1] is C.c_int, name
        assert table[name][2] == params, (name, table[name][2], params)
        # the two datatypes sit right before the form's tail
        tail = {True: 1, False: 2}[not name.startswith("ompi_amd_i")]
        assert params[-tail - 2:-tail] == [C.c_void_p, C.c_void_p], name


def brute_granule(gran, typed, contig):
    for g in (16, 8, 4, 2, 1):
        if gran % g == 0 and typed % g == 0 and contig % g == 0:
            return g
    raise AssertionError


def test_typed_granule_and_walk_rule(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "typed_rule_check")
    src = os.path.join(ROOT, "tests", "harness", "typed_rule_check.cpp")
    base = [cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    errs = []
    # both variants are sanitized (runtime linked statically, or not): an
    # unsanitized build is no substitute, so there is none to fall back to
    for extra in (SANITIZE + ["-static-libasan", "-static-libubsan"], SANITIZE):
        cc = subprocess.run(base + extra, capture_output=True, text=True)
        if cc.returncode == 0:
            break
        errs.append(cc.stderr[-1500:])
    assert cc.returncode == 0, "\n".join(errs)
    rng = np.random.default_rng(20260)
    cases = []
    for i in range(400):
        gran = int(rng.choice([1, 2, 4, 8, 16, 3, 6, 12, 24, 48]))
        typed = int(rng.integers(1, 1 << 47)) & ~int(rng.choice([0, 1, 3, 7, 15, 255]))
        contig = int(rng.integers(1, 1 << 47)) & ~int(rng.choice([0, 1, 3, 7, 15, 255]))
        # pair sizes around the threshold of every granule: G * 2^32 - 1, exactly, + 1; and small ones
        g = int(rng.choice([1, 2, 4, 8, 16]))
        pair = int(rng.choice([g * (1 << 32) - 1, g * (1 << 32), g * (1 << 32) + 1, int(rng.integers(0, 1 << 20)),
                               int(rng.integers(1 << 30, 1 << 40))]))
        cases.append((gran, typed, contig, pair, int(i % 7 == 0)))
    path = tmp_path / "cases.txt"
    path.write_text("".join("%d %d %d %d %d\n" % c for c in cases))
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    lines = run.stdout.split("\n")
    assert lines[len(cases)] == f"typed rule: {len(cases)} cases"
    seen = set()
    for (gran, typed, contig, pair, force), line in zip(cases, lines):
        G = brute_granule(gran, typed, contig)
        w64 = 1 if force or pair // G >= 1 << 32 else 0
        assert line == f"{G} {w64}", ((gran, typed, contig, pair, force), line, (G, w64))
        seen.add((G, w64))
    assert {g for g, _ in seen} == {1, 2, 4, 8, 16} and {w for _, w in seen} == {0, 1}
