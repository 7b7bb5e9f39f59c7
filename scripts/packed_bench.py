#!/usr/bin/env python3
"""blosc_gpu_compress_packed against the two routes a caller had before it, on the benchmark's config 2 batch (128 chunks of 64 MiB
bench19, typesize 8, LZ4 clevel 5, shuffle):

  batch        blosc_gpu_compress_batch alone: one destination of nbytes + 16 per chunk
  batch_pack   ... followed by the device-to-device pack of the results (c-blosc_amd/multigpu.py: pack_local)
  packed       blosc_gpu_compress_packed into one buffer of exactly the size a sizing call (dest NULL) reported

Every route runs in a process of its own, so that its peak device memory is its own: torch.cuda.max_memory_allocated for the caller's
tensors, and what the device reports in use beyond torch's pool for the library's arenas (BLOSC_AMD_DEBUG=1 prints each of them).
Prints one JSON line per route.  DESIGN.md 3.6 has the figures.

    python scripts/packed_bench.py [--chunks 128] [--chunk-mib 64] [--steps 10] [--warmup 3]
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("batch", "batch_pack", "packed")


def run_route(a):
    import torch
    torch.cuda.init()                    # torch's HIP runtime first (tests/conftest.py)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import bench19
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); sys.modules["c_blosc_amd"] = pkg; spec.loader.exec_module(pkg)
    mspec = importlib.util.spec_from_file_location("c_blosc_amd_multigpu", os.path.join(ROOT, "c-blosc_amd", "multigpu.py"))
    multigpu = importlib.util.module_from_spec(mspec); mspec.loader.exec_module(multigpu)
    dev = torch.device("cuda:0")
    n, size = a.chunks, a.chunk_mib << 20
    one = torch.from_numpy(bench19(size)).to(dev)
    src = [one.clone() for _ in range(n)]
    sizes = [size] * n
    torch.cuda.synchronize()
    base_alloc = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    times = []
    if a.route == "packed":
        b = pkg.PackedBatch(n)
        assert b.compress([t.data_ptr() for t in src], sizes, None, 0, 8, 5, 1, b"lz4") == 0        # the sizing call
        need = b.offsets()[-1]
        cont = torch.empty(need, dtype=torch.uint8, device=dev)
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            assert b.compress([t.data_ptr() for t in src], sizes, cont.data_ptr(), need, 8, 5, 1, b"lz4") == 0
            times.append((time.perf_counter() - t0) * 1e3)
        cb = b.results()
        assert all(c > 0 for c in cb) and b.offsets()[-1] == need
        payload = need
    else:
        dst = [torch.empty(size + 16, dtype=torch.uint8, device=dev) for _ in range(n)]
        b = pkg.DeviceBatch([t.data_ptr() for t in src], sizes, [t.data_ptr() for t in dst], [size + 16] * n)
        for k in range(a.warmup + a.steps):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            assert b.compress(8, 5, 1, b"lz4") == 0
            if a.route == "batch_pack":
                out = multigpu.pack_local(dst, b.results())
                torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        cb = b.results()
        assert all(c > 0 for c in cb)
        payload = sum(cb)
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    t = times[a.warmup:]
    print(json.dumps({"route": a.route, "chunks": n, "chunk_mib": a.chunk_mib, "ms_median": round(statistics.median(t), 3), "ms_min": round(min(t), 3),
                      "ms_max": round(max(t), 3), "payload_bytes": payload,
                      "caller_peak_mib_beyond_sources": round((torch.cuda.max_memory_allocated() - base_alloc) / 2 ** 20, 1),
                      "library_mib": round((total - free - torch.cuda.memory_reserved()) / 2 ** 20, 1)}), flush=True)
    pkg.load().blosc_destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=128)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--route", choices=ROUTES)
    a = ap.parse_args()
    if a.route:
        return run_route(a)
    for route in ROUTES:                 # a fresh process per route
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--route", route, "--chunks", str(a.chunks), "--chunk-mib", str(a.chunk_mib),
                              "--steps", str(a.steps), "--warmup", str(a.warmup)], timeout=600)
        if rc != 0:
            sys.exit(f"route {route} failed with exit status {rc}")


if __name__ == "__main__":
    main()
