"""Worker of tests/test_bench_cli.py: coll_bench.bench_allreduce at world
size 1 on the CPU, with the communicator and the device calls stood in for,
so that what a plain and a --full run put on the line can be checked without
a GPU.  argv: <free port> <dump dir> [full].  Prints the line."""
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
                  MASTER_PORT=sys.argv[1], OMPI_AMD_BENCH_SHARE_GPU="1",
                  OMPI_AMD_BENCH_NO_AUTOTUNE="1")

import torch  # noqa: E402

from ompi_amd import coll, coll_bench  # noqa: E402

torch.cuda.set_device = lambda d: None
torch.cuda.synchronize = lambda *a: None
torch.cuda.current_stream = lambda *a: None
_generator, _rand = torch.Generator, torch.rand
torch.Generator = lambda device=None: _generator()
torch.rand = lambda n, device=None, generator=None: _rand(n, generator=generator)

CALLS = {"allreduce": 0, "profiled": 0, "exact": 0}


class Comm:
    """Copies its input; counts its calls, those under profile=1 apart."""
    def __init__(self):
        self.p = {"algorithm": 2, "user_ipc": 0, "blocks": 256, "autotune_state": 2,
                  "autotune_algorithm": 2, "autotune_blocks": 256, "autotune_copy_nt": 1,
                  "autotune_ncand": 0, "ipc_mode_legacy": 0, "profile": 0}

    def get_param(self, k):
        return self.p[k]

    def set_param(self, k, v):
        self.p[k] = v

    def allreduce(self, x, y, n, dt, op, stream=None):
        CALLS["profiled" if self.p["profile"] else "allreduce"] += 1
        y.copy_(x)

    def error(self):
        return 0

    def phase_ms(self, k):
        return (1.0, 2)

    def free(self):
        pass


def exact(*a):
    CALLS["exact"] += 1
    return True


coll.Communicator.from_torch_distributed = staticmethod(lambda device=0: Comm())
coll_bench._watchdog = lambda *a: None
coll_bench._exact_ok = exact
args = types.SimpleNamespace(ar_bytes=1 << 20, steps=3, warmup=2, no_extras=True, no_cpu_baseline=True,
                             full=len(sys.argv) > 3, dump_outputs=sys.argv[2])
res = coll_bench.bench_allreduce(args, "m", 153.0)
res["calls"] = CALLS
print(json.dumps(res))
