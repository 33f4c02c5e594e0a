"""coll/rocm's alltoallw slots (ROCM_HAVE_TYPED_XCH outside the harness builds) compile against
the reference's own headers, as tests/test_real_headers.py compiles the module without the macro."""
import os
import subprocess

from test_real_headers import HERE, REF, ROOT, config_dirs, pytestmark  # noqa: F401


def test_alltoallw_slots_compile_against_reference_headers(config_dirs):
    path = os.path.join(ROOT, "ompi_amd", "mca", "coll", "rocm", "coll_rocm_module.c")
    inc = [config_dirs[0], HERE, REF] + [os.path.join(REF, d) for d in (
        "opal/include", "ompi/include", "opal/mca/event/libevent2022/libevent",
        "opal/mca/event/libevent2022/libevent/include")] + [os.path.join(ROOT, "include"), os.path.dirname(path)]
    cmd = ["gcc", "-fsyntax-only", "-std=gnu11", "-Wall", "-Wextra", "-Wno-unused-parameter",
           "-Wno-missing-field-initializers", "-Wno-sign-compare", "-DROCM_HAVE_TYPED_XCH"]
    r = subprocess.run(cmd + [f"-I{d}" for d in inc] + [path], capture_output=True, text=True, timeout=120)
    ours = [ln for ln in r.stderr.splitlines() if ("error" in ln or "warning" in ln) and not ln.startswith(REF)]
    assert r.returncode == 0 and not ours, (r.returncode, "\n".join(ours) or r.stderr[-3000:])
