"""Typed sendrecv against the composition pml/rocm runs without it, 2 ranks sharing one GPU.

    python tools/typed_p2p_bench.py [--user-ipc] [out.json]

A vector of 64-byte runs every 128 bytes on both sides, 64 KiB, 1 MiB and
16 MiB packed, each rank exchanging with the other.  Two contenders move the
same data: sendrecv_typed (one call), and ompi_amd_ddt_pack + byte sendrecv +
ompi_amd_ddt_unpack through two temporary device buffers.  The contenders
alternate inside every round; a sample is INNER calls ended by a synchronise,
divided by INNER; the figure is the median of ROUNDS rounds after WARM
warm-up rounds on the worst rank, the spread (max - min) / median of that
rank's rounds.  The ranks share ONE GPU: a "remote" load is a load from the
same HBM, and no xGMI figure follows.  Both contenders run on the library
this checkout built; with TYPED_P2P_BENCH_LIB=<another libompi_amd.so> (one
built from the parent commit) only the composed contender runs, on that
library, as "composed_other": a second run, not alternated with the first.

--user-ipc sets p2p_user_ipc = 1, under which a large typed message goes by
typed rendezvous (the receiver's one kernel walks both
datatypes) and the composition is what the parent ran there: pack + a byte
rendezvous + unpack.  Send buffers are then at least 4 MiB, an allocation
peers can map; "rndv_sends" counts the typed sends that took the rendezvous.
Two local contenders join the rounds: ompi_amd_ddt_sndrcv from the vector into
itself shifted ("local_sndrcv"), and ompi_amd_ddt_pack + ompi_amd_ddt_unpack
through a temporary ("local_composed"); both ranks run them at once, so each
has half the GPU.
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
SIZES = ((65536, 200), (1048576, 200), (16777216, 40))  # packed bytes, INNER (a round lasts 4 ms or more)


def worker():
    import torch
    import torch.distributed as dist
    from ompi_amd import _lib
    other = os.environ.get("TYPED_P2P_BENCH_LIB")
    lib = _lib.load(other) if other else _lib.load()  # before anything loads the default
    from ompi_amd import coll, datatype as dt, pml
    rank = int(os.environ["RANK"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=2)
    comm = coll.Communicator.from_torch_distributed(device=0)
    comm.set_param("timeout_ms", 20000)
    user_ipc = os.environ.get("TYPED_P2P_BENCH_USER_IPC") == "1"
    comm.set_param("p2p_user_ipc", int(user_ipc))
    floor = (4 << 20) if user_ipc else 0  # an allocation peers can map
    vec = dt.from_runs("vec64_stride128", [(0, 64)], 128).commit()
    res = {}
    for B, inner in SIZES:
        elems = B // 64
        src, dst = (torch.zeros(max(elems * 128, floor), dtype=torch.uint8, device="cuda") for _ in range(2))
        tmp_s, tmp_r = (torch.zeros(max(B, floor), dtype=torch.uint8, device="cuda") for _ in range(2))
        done = C.c_size_t(0)

        def composed():
            assert lib.ompi_amd_ddt_pack(vec._handle, elems, src.data_ptr(), tmp_s.data_ptr(), 0, B,
                                         C.byref(done), None) == 0
            pml.sendrecv(comm, tmp_s, 1 - rank, 3, tmp_r, 1 - rank, 3)
            assert lib.ompi_amd_ddt_unpack(vec._handle, elems, tmp_r.data_ptr(), dst.data_ptr(), 0, B,
                                           C.byref(done), None) == 0

        variants = [("typed", lambda: pml.sendrecv_typed(comm, src, elems, vec, 1 - rank, 3, dst, elems, vec,
                                                         1 - rank, 3)), ("composed", composed)]
        if other:
            variants = [("composed_other", composed)]
        elif user_ipc:
            def local_composed():
                assert lib.ompi_amd_ddt_pack(vec._handle, elems, src.data_ptr(), tmp_s.data_ptr(), 0, B,
                                             C.byref(done), None) == 0
                assert lib.ompi_amd_ddt_unpack(vec._handle, elems, tmp_s.data_ptr(), dst.data_ptr() + 64, 0, B,
                                               C.byref(done), None) == 0

            variants += [("local_sndrcv", lambda: dt.sndrcv(src, elems, vec, dst.data_ptr() + 64, elems, vec)),
                         ("local_composed", local_composed)]
        rndv0 = comm.get_param("p2p_typed_rndv") if user_ipc else 0
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
        if user_ipc:
            res[str(B)]["rndv_sends"] = {"us": comm.get_param("p2p_typed_rndv") - rndv0, "spread": 0}
    if comm.error():
        res["error"] = comm.error()
    print("RESULT " + json.dumps(res), flush=True)
    comm.free()
    dist.destroy_process_group()


def main():
    import socket
    user_ipc = "--user-ipc" in sys.argv
    args = [a for a in sys.argv[1:] if a != "--user-ipc"]
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   TYPED_BENCH_WORKER="1", TYPED_P2P_BENCH_USER_IPC=str(int(user_ipc)))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)], env=env,
                                      stdout=subprocess.PIPE, text=True))
    per_rank, bad = [], False
    try:
        for p in procs:
            out, _ = p.communicate(timeout=300)
            bad = bad or p.returncode != 0
            per_rank += [json.loads(ln[7:]) for ln in out.splitlines() if ln.startswith("RESULT ")]
    finally:  # a rank that hung or outlived a failed peer must not keep the GPU
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    if bad or len(per_rank) != 2 or any("error" in pr for pr in per_rank):
        sys.exit(f"a rank failed: {[p.returncode for p in procs]}")
    worst = {B: {k: max((pr[B][k] for pr in per_rank), key=lambda x: x["us"]) for k in per_rank[0][B]}
             for B in per_rank[0]}
    doc = {"what": ("typed sendrecv vs pack + sendrecv + unpack" + (
                    " under p2p_user_ipc = 1 (typed rendezvous), and the local ddt_sndrcv vs pack + unpack"
                    if user_ipc else "") + ", 2 ranks sharing ONE MI355X (no xGMI figure)"),
           "unit": "us per call; spread = (max - min) / median over the rounds",
           "method": f"median of {ROUNDS} rounds after {WARM} warm-ups, contenders alternating; worst rank",
           "packed_bytes": worst}
    print(json.dumps(doc))
    if args:
        with open(args[0], "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    worker() if os.environ.get("TYPED_BENCH_WORKER") == "1" else main()
