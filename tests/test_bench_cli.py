"""bench.py's command line: a plain run is the headline alone, --full turns
the CPU baselines and side rows on, --dump-outputs writes what the last
timed step computed (whole, or a fixed sample of a large output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
STUB = os.path.join(ROOT, "tests", "bench_allreduce_stub.py")
# child of the GPU test (argv: count, output path): bench_op's seeded inputs
# summed by torch, then bench_op itself (1 warmup, 3 steps) with the op
# launches and the timing events' records traced in order
EXPECTED = """
import sys, numpy, torch
sys.path.insert(0, %r)
import bench
from ompi_amd import op as mop
n = int(sys.argv[1])
g = torch.Generator(device="cuda").manual_seed(20261015)
a = torch.randn(n, device="cuda", generator=g)
b = torch.randn(n, device="cuda", generator=g)
numpy.save(sys.argv[2], (a + b).cpu().numpy())
trace, launch, record = [], mop.reduce_local_3buff_async, torch.cuda.Event.record
mop.reduce_local_3buff_async = lambda *a, **k: (trace.append("op"), launch(*a, **k))[1]
torch.cuda.Event.record = lambda *a, **k: (trace.append("event"), record(*a, **k))[1]
sys.argv = ["bench.py", "--steps", "3", "--warmup", "1", "--op-bytes", str(4 * n)]
bench.bench_op(bench.parse())
print(" ".join(trace))
""" % ROOT


def _parse(*argv):
    """bench.parse() in a child (importing bench sets process environment)."""
    r = subprocess.run([sys.executable, "-c", "import bench, json; print(json.dumps(vars(bench.parse())))",
                        *argv], cwd=ROOT, capture_output=True, text=True, timeout=60)
    return json.loads(r.stdout) if r.returncode == 0 else None


def test_plain_run_is_headline_only_and_full_restores_the_rest():
    a = _parse("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a["steps"], a["warmup"], a["full"], a["dump_outputs"]) == (7, 2, False, None)
    assert a["no_cpu_baseline"] and a["no_extras"]
    a = _parse("--full")
    assert a["full"] and not a["no_cpu_baseline"] and not a["no_extras"]
    a = _parse("--full", "--no-extras", "--dump-outputs", "d")
    assert a["no_extras"] and not a["no_cpu_baseline"] and a["dump_outputs"] == "d"
    assert _parse("--steps", "0") is None


def test_dump_outputs_whole_and_sampled(tmp_path):
    from ompi_amd import coll_bench as cb

    small = torch.arange(1000, dtype=torch.float32)
    n = cb.DUMP_WHOLE_BYTES // 4 + 5  # just over the whole-dump limit
    big = torch.arange(n, dtype=torch.float32)  # value == index (n < 2^24)
    wide = torch.arange(10, dtype=torch.float64) / 3
    for d in ("a", "b"):
        cb.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "wide": wide})
    s, b, w = (np.load(tmp_path / "a" / f"{k}.npy") for k in ("small", "big", "wide"))
    assert s.dtype == np.float32 and np.array_equal(s, small.numpy())
    assert w.dtype == np.float64 and np.array_equal(w, wide.numpy())
    assert b.dtype == np.float32 and b.size == cb.DUMP_SAMPLE + 2 * cb.DUMP_EDGE
    assert b.nbytes + s.nbytes + w.nbytes <= 64 << 20
    assert np.array_equal(b[:cb.DUMP_EDGE], np.arange(cb.DUMP_EDGE))
    assert np.array_equal(b[-cb.DUMP_EDGE:], np.arange(n - cb.DUMP_EDGE, n))
    mid = b[cb.DUMP_EDGE:-cb.DUMP_EDGE]
    assert np.all(np.diff(mid) >= 0) and 0 <= mid[0] and mid[-1] < n
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))  # the sample is fixed


@pytest.mark.gpu
def test_bench_plain_run_line_and_dumped_output(tmp_path):
    """A plain N = 1 run at 4 MiB per buffer: the line has ms_per_step and
    none of the --full rows, the dumped result is the fp32 sum of the seeded
    inputs, bit for bit, and --warmup 1 --steps 3 is one launch before the
    first timing event and three between the two."""
    nbytes = 4 << 20
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--op-bytes", str(nbytes), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
    assert res["unit"] == "GB/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    # value and ms_per_step are one measurement, rounded to 2 and 4 decimals
    ms = res["ms_per_step"]
    assert 3.0 * nbytes / (ms + 5e-5) / 1e6 - 0.01 <= res["value"] <= 3.0 * nbytes / (ms - 5e-5) / 1e6 + 0.01
    for k in ("cpu_baseline", "cpu_allreduce_configs0", "next_rows_n1", "config_rows_n1"):
        assert k not in res
    assert os.listdir(tmp_path / "out") == ["op_sum_out.npy"]
    got = np.load(tmp_path / "out" / "op_sum_out.npy")
    # the bench's inputs again, summed by torch, in a child as well, so that
    # this test leaves no GPU context behind in the pytest process
    r = subprocess.run([sys.executable, "-c", EXPECTED, str(nbytes // 4), str(tmp_path / "exp.npy")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == ["op", "event", "op", "op", "op", "event"], r.stdout
    exp = np.load(tmp_path / "exp.npy")
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


@pytest.mark.parametrize("full", [False, True], ids=["plain", "full"])
def test_allreduce_leg_plain_run_is_headline_only(tmp_path, full):
    """The N > 1 leg over a stand-in communicator (tests/bench_allreduce_stub.py):
    a plain run makes its warmup and timed calls and nothing else, and reports
    the per-phase figures, the exactness check and the RCCL comparator as
    None; --full runs the profiled pass and the check again.  Both dump
    rank 0's result."""
    r = subprocess.run([sys.executable, STUB, _free_port(), str(tmp_path)] + (["full"] if full else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["unit"] == "GB/s" and res["dtype"] == "f32"
    assert res["calls"] == {"allreduce": 5, "profiled": 3 if full else 0, "exact": 1 if full else 0}
    assert (res["roofline"]["phases"] is not None) == full
    assert res["config"]["bit_exact_dataset_E"] is (True if full else None)
    assert res["rccl_comparator"] is None  # one rank on a shared device: no comparator either way
    out = np.load(tmp_path / "allreduce_out.npy")
    assert out.dtype == np.float32 and out.size == (1 << 20) // 4 and np.all(np.abs(out) <= 1)
