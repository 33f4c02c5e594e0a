"""Small-message allgatherv / gather / scatter latency, N ranks sharing one GPU.

    python tools/gather_latency.py N [out.json]

Per size (8 B and 4 KiB per rank) and variant, one sample is INNER calls back
to back on one stream ended by a stream synchronise, divided by INNER; the
variants alternate inside every round; the figures are the median and the
quartiles of 20 rounds after 5 warm-up rounds, and the worst rank's are
reported.  Variants:

  allgatherv_fused    blocking allgatherv, fused_bytes raised so the size is fused
                      (fused_allgatherv_kernel: load once, store N times)
  allgatherv_default  the same call under the communicator's default fused_bytes
  allgatherv_staged   the same call with fused_bytes = 0 (copy / barrier / copy)
  allgatherv_plan     allgatherv_init started INNER times (no host agreement)
  alltoallv_plan      the equivalent alltoallv (every send displacement equal)
                      as a plan: fused_alltoall_kernel, the multicast's comparator
  allgather           the existing allgather at equal counts, for reference
  gather_fused / gather_staged, scatter_fused / scatter_staged   root 0

"paths" records which path each variant's calls took (fused, staged, landing).
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
SIZES = (8, 4096)
FUSED_ON = 1 << 20


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
    keys = ("gather_fused", "gather_staged", "gather_landing", "alltoall_fused", "alltoall_staged",
            "alltoall_landing")
    res = {"fused_bytes_default": fused_default}
    for B in SIZES:
        s = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        r = torch.zeros(n * B, dtype=torch.uint8, device="cuda")
        cnt, dsp, same = [B] * n, [B * p for p in range(n)], [0] * n
        comm.set_param("fused_bytes", FUSED_ON)
        agv_plan = comm.allgatherv_init(s, B, r, cnt, dsp)
        a2av_plan = comm.alltoallv_init(s, cnt, same, r, cnt, dsp)

        def started(plan):
            def go():
                plan.start()
                plan.wait()
            return go

        agv = lambda: comm.allgatherv(s, B, r, cnt, dsp)          # noqa: E731
        gat = lambda: comm.gather(s, r, B, 0)                     # noqa: E731
        sca = lambda: comm.scatter(s, r, B, 0)                    # noqa: E731
        variants = [("allgatherv_fused", agv, FUSED_ON), ("allgatherv_default", agv, fused_default),
                    ("allgatherv_staged", agv, 0), ("allgatherv_plan", started(agv_plan), FUSED_ON),
                    ("alltoallv_plan", started(a2av_plan), FUSED_ON),
                    ("allgather", lambda: comm.allgather(s, r, B), fused_default),
                    ("gather_fused", gat, FUSED_ON), ("gather_staged", gat, 0),
                    ("scatter_fused", sca, FUSED_ON), ("scatter_staged", sca, 0)]
        times = {name: [] for name, _, _ in variants}
        paths = {}
        for rnd in range(WARM + ROUNDS):
            for name, fn, fb in variants:
                comm.set_param("fused_bytes", fb)
                before = [comm.get_param(k) for k in keys]
                torch.cuda.synchronize()
                dist.barrier()
                t0 = time.perf_counter()
                for _ in range(INNER):
                    fn()
                torch.cuda.synchronize()
                dt = (time.perf_counter() - t0) / INNER
                if rnd >= WARM:
                    times[name].append(dt * 1e6)
                paths[name] = {k: comm.get_param(k) - b for k, b in zip(keys, before)
                               if comm.get_param(k) != b}
        comm.set_param("fused_bytes", fused_default)
        agv_plan.free()
        a2av_plan.free()
        out = {}
        for k, v in times.items():
            q = statistics.quantiles(v, n=4)
            out[k] = {"median": round(statistics.median(v), 2), "p25": round(q[0], 2), "p75": round(q[2], 2),
                      "min": round(min(v), 2), "max": round(max(v), 2)}
        res[str(B)] = {"us": out, "paths": paths}
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
                   MASTER_PORT=str(port), GATHER_LATENCY_WORKER="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=env,
                                      stdout=subprocess.PIPE, text=True))
    per_rank, bad = [], False
    for p in procs:
        out, _ = p.communicate(timeout=300)
        bad = bad or p.returncode != 0
        per_rank += [json.loads(ln[7:]) for ln in out.splitlines() if ln.startswith("RESULT ")]
    if bad or len(per_rank) != n or any("error" in pr for pr in per_rank):
        sys.exit(f"a rank failed: {[p.returncode for p in procs]}")
    worst = {}
    for B in map(str, SIZES):
        worst[B] = {"us": {}, "paths_rank0": per_rank[0][B]["paths"]}
        for k in per_rank[0][B]["us"]:
            w = max(per_rank, key=lambda pr: pr[B]["us"][k]["median"])
            worst[B]["us"][k] = w[B]["us"][k]
    doc = {"what": f"allgatherv / gather / scatter latency, {n} ranks sharing ONE MI355X (not xGMI)",
           "unit": "us per call",
           "method": (f"median and quartiles of {ROUNDS} rounds after {WARM} warm-ups; a round = {INNER} "
                      "calls + sync; the rank with the worst median"),
           "ranks": n, "fused_bytes_default": per_rank[0]["fused_bytes_default"], "bytes_per_rank": worst}
    print(json.dumps(doc))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    worker() if os.environ.get("GATHER_LATENCY_WORKER") == "1" else main()
