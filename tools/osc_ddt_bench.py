"""One-sided calls between two derived datatypes: the fused kernels against the packed path, 2 ranks sharing one GPU.

    python tools/osc_ddt_bench.py [out.json]

Put, get and get_accumulate (fp64 SUM) from a vector into the same vector of the other rank's window, 4 KiB, 1 MiB
and 64 MiB packed, with a one-element program (64-byte runs every 128 bytes) and a multi-run one (runs of 16, 8, 32
and 8 bytes in 128).  The two contenders are one library under param osc_ddt_fuse = 1 (one kernel
walks every datatype) and = 0 (the origin packed into the window's scratch, the result unpacked from it); they
alternate inside every round.  A sample is INNER calls inside one lock_all .. unlock_all ended by a synchronise,
divided by INNER; the figure is the median of ROUNDS rounds after WARM warm-up rounds on the worst rank, the spread
(max - min) / median of that rank's rounds.  Both ranks run at once, each targeting the other, and share ONE GPU: a
"remote" store is a store to the same HBM, and no xGMI figure follows.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS, WARM = 10, 2
SIZES = ((4096, 200), (1 << 20, 100), (64 << 20, 8))  # packed bytes, INNER


def worker():
    import torch
    import torch.distributed as dist
    from ompi_amd import coll, datatype as dt, op as mop, osc
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    comm = coll.Communicator.from_torch_distributed(device=0)
    comm.set_param("timeout_ms", 20000)
    progs = {"one_element": dt.from_runs("vec64_stride128", [(0, 64)], 128).commit(),
             "multi_run": dt.from_runs("runs4_in128", [(0, 16), (24, 8), (40, 32), (80, 8)], 128).commit()}
    span = 2 * SIZES[-1][0]
    win = osc.Window.allocate(comm, span)
    src, res = (torch.zeros(span, dtype=torch.uint8, device="cuda") for _ in range(2))
    D, SUM, to = mop.MPI_DOUBLE, mop.MPI_SUM, 1 - rank
    out = {}
    for pname, vec in progs.items():
        for B, inner in SIZES:
            n = B // 64
            calls = {"put": lambda: win.put_ddt(src, n, vec, to, 0, n, vec),
                     "get": lambda: win.get_ddt(res, n, vec, to, 0, n, vec),
                     "get_accumulate": lambda: win.get_accumulate_ddt(src, n, vec, res, n, vec, to, 0, n, vec, D, SUM)}
            times = {(c, f): [] for c in calls for f in (1, 0)}
            for rnd in range(WARM + ROUNDS):
                for (c, fuse), samples in times.items():
                    comm.set_param("osc_ddt_fuse", fuse)
                    torch.cuda.synchronize()
                    dist.barrier()
                    t0 = time.perf_counter()
                    win.lock_all()
                    for _ in range(inner):
                        calls[c]()
                    win.unlock_all()
                    torch.cuda.synchronize()
                    if rnd >= WARM:
                        samples.append((time.perf_counter() - t0) / inner * 1e6)
            out[f"{pname}/{B}"] = {f"{c}/{'fused' if f else 'packed'}": {
                "us": round(statistics.median(v), 2), "spread": round((max(v) - min(v)) / statistics.median(v), 3)}
                for (c, f), v in times.items()}
    out["counters"] = {k: comm.get_param(k) for k in ("osc_ddt_fused", "osc_ddt_packed", "osc_ddt_lds")}
    if comm.error():
        out["error"] = comm.error()
    print("RESULT " + json.dumps(out), flush=True)
    win.free()
    comm.free()
    dist.destroy_process_group()


def main():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   OSC_DDT_BENCH_WORKER="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=env,
                                      stdout=subprocess.PIPE, text=True))
    per_rank, bad = [], False
    try:
        for p in procs:
            o, _ = p.communicate(timeout=400)
            bad = bad or p.returncode != 0
            per_rank += [json.loads(ln[7:]) for ln in o.splitlines() if ln.startswith("RESULT ")]
    finally:  # a rank that hung or outlived a failed peer must not keep the GPU
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    if bad or len(per_rank) != 2 or any("error" in pr for pr in per_rank):
        sys.exit(f"a rank failed: {[p.returncode for p in procs]}")
    shapes = [k for k in per_rank[0] if k != "counters"]
    worst = {s: {k: max((pr[s][k] for pr in per_rank), key=lambda x: x["us"]) for k in per_rank[0][s]}
             for s in shapes}
    for s in shapes:  # packed / fused: above 1 the fused path is faster
        for c in ("put", "get", "get_accumulate"):
            worst[s][f"{c}/ratio"] = round(worst[s][f"{c}/packed"]["us"] / worst[s][f"{c}/fused"]["us"], 2)
    doc = {"what": "derived-datatype put / get / get_accumulate, osc_ddt_fuse 1 vs 0, 2 ranks sharing ONE MI355X "
                   "(no xGMI figure)",
           "unit": "us per call; spread = (max - min) / median over the rounds; ratio = packed / fused",
           "method": f"median of {ROUNDS} rounds after {WARM} warm-ups, contenders alternating; worst rank",
           "counters_rank0": per_rank[0]["counters"], "program/packed_bytes": worst}
    print(json.dumps(doc))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    worker() if os.environ.get("OSC_DDT_BENCH_WORKER") == "1" else main()
