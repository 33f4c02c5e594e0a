"""Typed alltoall against the composition it replaces, N ranks sharing one GPU.

    python tools/typed_alltoall_bench.py N [out.json]

Two workloads at 4 KiB, 256 KiB and 16 MiB packed per pair: the stride-12
vector of 4-byte blocks on both sides, and the same vector in / contiguous
out (the transpose).  Two contenders move the same data: alltoall_typed (one
call), and ompi_amd_ddt_pack + alltoall + ompi_amd_ddt_unpack through two
temporary device buffers (the unpack is dropped where the receive side is
contiguous).  The contenders alternate inside every round; a sample is INNER
calls ended by a synchronise, divided by INNER; the figure is the median of
ROUNDS rounds after WARM warm-up rounds on the worst rank, and the spread is
(max - min) / median of the same rank's rounds.  The ranks share ONE GPU:
"remote" stores are stores to the same HBM, and no xGMI figure follows.

The composed contender runs on whatever libompi_amd this checkout built; to
measure it on another build (the parent commit's), run the tool from that
checkout with TYPED_BENCH_ONLY=composed and compare the two files.
"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, WARM = 12, 3
SIZES = ((4096, 40), (262144, 20), (16777216, 3))  # packed bytes per pair, INNER


def worker():
    import torch
    import torch.distributed as dist
    from ompi_amd import _lib, coll, datatype as dt
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    only = os.environ.get("TYPED_BENCH_ONLY", "")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=0)
    comm.set_param("timeout_ms", 20000)
    lib = _lib.load()
    vec = dt.from_runs("vec4_stride12", [(0, 4)], 12).commit()  # one 4-byte block every 12 bytes
    res = {}
    for B, inner in SIZES:
        elems = B // 4
        typed = torch.zeros(n * elems * 12 + 64, dtype=torch.uint8, device="cuda")
        typed_r = torch.zeros(n * elems * 12 + 64, dtype=torch.uint8, device="cuda")
        flat_r = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        tmp_s = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        tmp_r = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        done = C.c_size_t(0)

        def composed(out_typed):
            assert lib.ompi_amd_ddt_pack(vec._handle, n * elems, typed.data_ptr(), tmp_s.data_ptr(), 0,
                                         n * B, C.byref(done), None) == 0
            if out_typed:
                comm.alltoall(tmp_s, tmp_r, B)
                assert lib.ompi_amd_ddt_unpack(vec._handle, n * elems, tmp_r.data_ptr(),
                                               typed_r.data_ptr(), 0, n * B, C.byref(done), None) == 0
            else:
                comm.alltoall(tmp_s, flat_r, B)

        variants = []
        if only != "composed" and hasattr(comm, "alltoall_typed"):
            variants += [("vector_typed", lambda: comm.alltoall_typed(typed, typed_r, elems, elems, vec, vec)),
                         ("transpose_typed", lambda: comm.alltoall_typed(typed, flat_r, elems, B, vec, None))]
        if only != "typed":
            variants += [("vector_composed", lambda: composed(True)),
                         ("transpose_composed", lambda: composed(False))]
        times = {name: [] for name, _ in variants}
        for rnd in range(WARM + ROUNDS):
            for name, fn in variants:
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                torch.cuda.synchronize()
                if rnd >= WARM:
                    times[name].append((time.perf_counter() - t0) / inner * 1e6)
        res[str(B)] = {k: {"us": round(statistics.median(v), 2),
                           "spread": round((max(v) - min(v)) / statistics.median(v), 3)}
                       for k, v in times.items()}
    if comm.error():
        res["error"] = comm.error()
    print("RESULT " + json.dumps(res), flush=True)
    comm.free()
    dist.destroy_process_group()


def main():
    n = int(sys.argv[1])
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), TYPED_BENCH_WORKER="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=env,
                                      stdout=subprocess.PIPE, text=True))
    per_rank, bad = [], False
    for p in procs:
        out, _ = p.communicate(timeout=400)
        bad = bad or p.returncode != 0
        per_rank += [json.loads(ln[7:]) for ln in out.splitlines() if ln.startswith("RESULT ")]
    if bad or len(per_rank) != n or any("error" in pr for pr in per_rank):
        sys.exit(f"a rank failed: {[p.returncode for p in procs]}")
    worst = {B: {k: max((pr[B][k] for pr in per_rank), key=lambda x: x["us"]) for k in per_rank[0][B]}
             for B in per_rank[0]}
    doc = {"what": f"typed alltoall vs pack + alltoall + unpack, {n} ranks sharing ONE MI355X (no xGMI figure)",
           "unit": "us per call; spread = (max - min) / median over the rounds",
           "method": f"median of {ROUNDS} rounds after {WARM} warm-ups, contenders alternating; worst rank",
           "ranks": n, "packed_bytes_per_pair": worst}
    print(json.dumps(doc))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    worker() if os.environ.get("TYPED_BENCH_WORKER") == "1" else main()
