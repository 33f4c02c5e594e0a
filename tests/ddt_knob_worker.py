"""One process of tests/test_ddt_knobs_gpu.py: the convertor's environment
settings are read once per process, so each setting gets a fresh child.  Runs
a fixed list of layouts at 300 KiB and 1 MiB packed — pack, unpack and a
12-entry iovec train each way — byte for byte against the oracle, and prints
one JSON line per case with the routes each operation took (the library's
route counters), then one line with the totals.

DDT_KNOB_CASES (comma list of layout names) and DDT_KNOB_SIZES (comma list of
packed bytes) restrict the run."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [300 << 10, 1 << 20]
BLACS_LENS = [13, 13, 13, 13, 13, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1]
BLACS_DISPS = [286, 308, 330, 352, 374, 396, 419, 442, 465, 488, 511, 534, 557, 580, 603, 626,
               649, 672]
# (doubles per run, gap bytes): bl1, bl2, bl8 and bl64 at gaps of 8, 64, 512 and
# 5000 B, and bl64 at the 512-B gap too (1-KiB stride: the widest the tile takes)
VECTORS = [(1, 8), (2, 64), (8, 512), (64, 5000), (64, 512)]


def run_worker(env, cases=None, sizes=None, timeout=300):
    """Start one worker as a fresh child with `env` added to the environment
    and return its JSON lines (raises with the output's tail if it failed)."""
    e = dict(os.environ)
    e.update(env)
    if cases:
        e["DDT_KNOB_CASES"] = cases
    if sizes:
        e["DDT_KNOB_SIZES"] = sizes
    p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=e, capture_output=True,
                       text=True, timeout=timeout)
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert p.returncode == 0 and lines, (p.returncode, p.stdout[-1500:], p.stderr[-3000:])
    return lines


def layouts(dd, np):
    """name -> (datatype maker, instance size is the whole stream?)."""
    f64, i32 = dd.predefined("MPI_DOUBLE"), dd.predefined("MPI_INT")
    out = {}
    for bl, gap in VECTORS:  # one long vector: n runs of bl doubles, gap bytes apart
        out[f"vector_bl{bl}_gap{gap}"] = (
            lambda total, bl=bl, gap=gap: (dd.type_vector(total // (8 * bl), bl, bl + gap // 8, f64), 1))
    out["struct_int_double"] = lambda total: (dd.type_struct([1, 1], [0, 8], [i32, f64]), total // 12)
    out["blacs"] = lambda total: (dd.type_indexed(BLACS_LENS, BLACS_DISPS, i32),
                                  total // (4 * sum(BLACS_LENS)))
    # 9 and 300 elements, each two equal runs 256 B apart (so the search
    # divides by the run length) and 200 B or more from the next (no instance
    # tile): the element table searched in LDS, and read from global memory
    for n in (9, 300):
        lens = [1 + ((i // 2) * 7) % 5 for i in range(2 * n)]
        disps = [64 * i for i in range(2 * n)]
        out[f"indexed{n}"] = (lambda total, lens=lens, disps=disps:
                              (dd.type_indexed(lens, disps, i32), max(1, total // (4 * sum(lens)))))

    def drawn(cls):
        from ddt_random import rand_layout
        rng = np.random.default_rng(4242)
        while True:
            c, dt = rand_layout(rng)
            if c == cls and (dt.max_count is None or dt.size * dt.max_count >= (256 << 10)):
                return dt
    for cls in ("negstride", "descending", "interleaved"):
        def make(total, cls=cls):
            dt = drawn(cls)
            count = max(1, total // dt.size)
            return dt, count if dt.max_count is None else max(2, min(count, dt.max_count))
        out[cls] = make
    return out


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    from ddt_random import typed_bounds
    from ompi_amd import _lib
    from ompi_amd import datatype as dd
    from oracle import oracle as orc

    orc.lib()
    dev = "cuda:0"
    want = os.environ.get("DDT_KNOB_CASES")
    sizes = [int(x) for x in os.environ.get("DDT_KNOB_SIZES", "").split(",") if x] or SIZES
    table = layouts(dd, np)
    names = [n for n in table if not want or n in want.split(",")]
    totals = dict.fromkeys(_lib.DDT_ROUTES, 0)
    failed = 0
    gen = torch.Generator(device=dev).manual_seed(9)
    for name in names:
        for size in sizes:
            dt, count = table[name](size)
            total = dt.size * count
            lo, hi = typed_bounds(dt, count)
            low = min(lo, 0)
            n = hi - low + 128
            origin = 64 - low
            src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
            src_np = src.cpu().numpy()
            exp = orc.pack(dt.runs, dt.extent, count, src_np[origin:], 0, total)
            line = {"case": name, "size": size, "total": total, "count": count, "ok": True,
                    "routes": dict.fromkeys(_lib.DDT_ROUTES, 0), "ops": {}, "lds": {}, "bad": []}
            cut = [total // 12 + (3 if i % 2 else -3) for i in range(11)]
            cut.append(total - sum(cut))
            offs = np.concatenate([[0], np.cumsum(np.array(cut) + 16)[:-1]])

            def op(label, fn):
                _lib.ddt_route_reset()
                fn()
                torch.cuda.synchronize()
                c = _lib.ddt_route_counts()
                line["ops"][label] = [r for r in _lib.DDT_ROUTES if c[r]]
                line["lds"][label] = c["last_lds"]
                for r in _lib.DDT_ROUTES:
                    line["routes"][r] += c[r]
                    totals[r] += c[r]

            packed = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
            conv = dd.Convertor()
            conv.prepare_for_send(dt, count, src.data_ptr() + origin)
            op("pack", lambda: conv.pack(packed, total))
            if not np.array_equal(packed.cpu().numpy()[:total], exp):
                line["bad"].append("pack")

            def recv(label, mover):
                fill = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256, generator=gen)
                exp_dst = fill.cpu().numpy().copy()
                orc.unpack(dt.runs, dt.extent, count, exp, exp_dst[origin:], 0)
                c2 = dd.Convertor()
                c2.prepare_for_recv(dt, count, fill.data_ptr() + origin)
                op(label, lambda: mover(c2))
                if not np.array_equal(fill.cpu().numpy(), exp_dst):
                    line["bad"].append(label)

            good = torch.from_numpy(exp).to(dev)
            recv("unpack", lambda c2: c2.unpack(good, total))
            train = torch.zeros(int(offs[-1]) + cut[-1] + 64, dtype=torch.uint8, device=dev)
            iovs = [(train.data_ptr() + int(o), int(k)) for o, k in zip(offs, cut)]
            conv = dd.Convertor()
            conv.prepare_for_send(dt, count, src.data_ptr() + origin)
            op("iov_pack", lambda: conv.pack_iov(iovs))
            t_np = train.cpu().numpy()
            if not np.array_equal(np.concatenate([t_np[o:o + k] for o, k in zip(offs, cut)]), exp):
                line["bad"].append("iov_pack")
            recv("iov_unpack", lambda c2: c2.unpack_iov(iovs))
            line["ok"] = not line["bad"]
            failed += len(line["bad"])
            print(json.dumps(line), flush=True)
            dt.free()
    print(json.dumps({"case": "totals", "ok": failed == 0, "routes": totals, "ops": {}, "lds": {}}),
          flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
