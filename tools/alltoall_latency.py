"""Small-message alltoall latency, N ranks sharing one GPU.

    python tools/alltoall_latency.py N [out.json]

Per size (8 B and 1 KiB per pair) and variant — the fused kernel, the same
call forced onto the staged path (fused_bytes = 0), alltoallv of the same
counts (its host agreement on top of the fused kernel) and an allgather of
the same bytes per rank as the yardstick — one sample is INNER calls back to
back on one stream ended by a stream synchronise, divided by INNER; the
variants alternate inside every round; the figure is the median of 20
rounds after 5 warm-up rounds, and the worst rank's median is reported.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INNER, ROUNDS, WARM = 50, 20, 5


def worker():
    import torch
    import torch.distributed as dist
    from ompi_amd import coll
    rank, n = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=n)
    comm = coll.Communicator.from_torch_distributed(device=0)
    comm.set_param("timeout_ms", 10000)
    fused_default = comm.get_param("fused_bytes")
    res = {}
    for B in (8, 1024):
        s = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        r = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        cnt, dsp = [B] * n, [B * p for p in range(n)]

        def fused():
            comm.alltoall(s, r, B)

        def staged():
            comm.alltoall(s, r, B)

        def vector():
            comm.alltoallv(s, cnt, dsp, r, cnt, dsp)

        def gather():
            comm.allgather(s, r, B)

        variants = [("alltoall_fused", fused, fused_default), ("alltoall_staged", staged, 0),
                    ("alltoallv_fused", vector, fused_default), ("allgather", gather, fused_default)]
        times = {name: [] for name, _, _ in variants}
        for rnd in range(WARM + ROUNDS):
            for name, fn, fb in variants:
                comm.set_param("fused_bytes", fb)
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(INNER):
                    fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / INNER
                if rnd >= WARM:
                    times[name].append(dt * 1e6)
        comm.set_param("fused_bytes", fused_default)
        res[str(B)] = {k: round(statistics.median(v), 2) for k, v in times.items()}
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
                   MASTER_PORT=str(port), A2A_LATENCY_WORKER="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=env,
                                      stdout=subprocess.PIPE, text=True))
    per_rank, bad = [], False
    for p in procs:
        out, _ = p.communicate(timeout=200)
        bad = bad or p.returncode != 0
        per_rank += [json.loads(ln[7:]) for ln in out.splitlines() if ln.startswith("RESULT ")]
    if bad or len(per_rank) != n:
        sys.exit(f"a rank failed: {[p.returncode for p in procs]}")
    worst = {B: {k: max(pr[B][k] for pr in per_rank) for k in per_rank[0][B]} for B in ("8", "1024")}
    doc = {"what": f"alltoall latency, {n} ranks sharing ONE MI355X (not xGMI)", "unit": "us per call",
           "method": f"median of {ROUNDS} rounds after {WARM} warm-ups; a round = {INNER} calls + sync; worst rank",
           "ranks": n, "bytes_per_pair": worst}
    print(json.dumps(doc))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    worker() if os.environ.get("A2A_LATENCY_WORKER") == "1" else main()
