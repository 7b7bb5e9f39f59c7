#!/usr/bin/env python3
"""Rate of index_select on a compressed table: 2^20 random row indices, resident on the device, over 64 LZ4 chunks of 4 MiB (typesize 8, byte
shuffle, 1 MiB blocks) - ONE blosc_gpu_take_batch (include/blosc_gpu_take.h) against the only route without it: the indices to the host, one
(chunk, start, nitems) range and one destination pointer per row, blosc_gpu_getitem_batch (include/blosc_gpu_getitem.h).  The second route's
time includes the download of the indices and the building of its tables (numpy, vectorised): that is what its caller pays.
Row sizes 8, 64 and 1024 bytes.  Each side: a warm-up, then the median of ten; both run in one session and their outputs must be equal.
One more call of each under blosc_gpu_profile gives the kernels' own times.

    python scripts/take_rate.py [--out profiles/take_rate.json] [--indices 1048576]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNELS = ("k_take_mark", "k_take_gather", "k_getitem_gather", "k_decode_plan", "k_decode_streams")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "take_rate.json"))
    ap.add_argument("--indices", type=int, default=1 << 20)
    ap.add_argument("--chunks", type=int, default=64)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from helpers import bench19
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
    L = pkg.load()
    dev = torch.device("cuda:0")
    n, T = 4 << 20, 8
    plain = [np.roll(bench19(n).view("<i8"), 1009 * k).view(np.uint8) for k in range(args.chunks)]
    src = [torch.from_numpy(p.copy()).to(dev) for p in plain]
    comp = [torch.empty(n + 16, dtype=torch.uint8, device=dev) for _ in plain]
    b = pkg.DeviceBatch([t.data_ptr() for t in src], [n] * args.chunks, [t.data_ptr() for t in comp], [n + 16] * args.chunks)
    assert b.compress(T, 5, 1, b"lz4", (1 << 20) // T) == 0 and all(c > 0 for c in b.results())      # (a split block is typesize x the forced size)
    blocksize = int(comp[0][8:12].cpu().numpy().view("<i4")[0])
    del src
    srcs = [t.data_ptr() for t in comp]
    table = np.concatenate(plain)
    ip = C.POINTER(C.c_int)
    res = {}
    for row_bytes in (8, 64, 1024):
        nrows, per_chunk, items = table.size // row_bytes, n // row_bytes, row_bytes // T
        g = torch.Generator(device=dev); g.manual_seed(row_bytes)
        index = torch.randint(0, nrows, (args.indices,), dtype=torch.int64, device=dev, generator=g)
        want = table.reshape(nrows, row_bytes)[index.cpu().numpy()]
        out = torch.zeros(args.indices * row_bytes, dtype=torch.uint8, device=dev)
        status = torch.zeros(args.indices, dtype=torch.int32, device=dev)
        take = pkg.RowTake(row_bytes)
        keep = {}

        def one_take():
            assert take.batch(srcs, index.data_ptr(), args.indices, out.data_ptr(), status.data_ptr()) == 0 and take.failed() == 0

        def through_the_host():
            idx = index.cpu().numpy()
            chunk = (idx // per_chunk).astype(np.int32)
            start = ((idx % per_chunk) * items).astype(np.int32)
            nitems = np.full(idx.size, items, np.int32)
            dest = np.uint64(out.data_ptr()) + np.arange(idx.size, dtype=np.uint64) * np.uint64(row_bytes)
            result = np.empty(idx.size, np.int32)
            keep["result"] = result
            assert L.blosc_gpu_getitem_batch(args.chunks, (C.c_void_p * args.chunks)(*srcs), idx.size, chunk.ctypes.data_as(ip), start.ctypes.data_as(ip),
                                             nitems.ctypes.data_as(ip), dest.ctypes.data_as(C.POINTER(C.c_void_p)), result.ctypes.data_as(ip), None) == 0

        key = f"row_bytes_{row_bytes}"
        res[key] = {}
        for name, fn in (("one_blosc_gpu_take_batch", one_take), ("host_ranges_blosc_gpu_getitem_batch", through_the_host)):
            out.zero_()
            fn()                                            # warm-up (arenas, code objects)
            assert np.array_equal(out.cpu().numpy().reshape(args.indices, row_bytes), want), (name, row_bytes)
            ts = []
            for _ in range(10):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
            res[key][name + "_ms"] = round(statistics.median(ts), 3)
            res[key][name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
            L.blosc_gpu_profile(1); L.blosc_gpu_profile_reset()
            fn()
            res[key][name + "_kernels_ms"] = {k: round(pkg.profile_get(k)[0], 3) for k in KERNELS if pkg.profile_get(k)[1]}
            L.blosc_gpu_profile(0)
        assert bool((status == row_bytes).all()) and bool((keep["result"] == row_bytes).all())
        res[key]["host_route_over_take"] = round(res[key]["host_ranges_blosc_gpu_getitem_batch_ms"] / res[key]["one_blosc_gpu_take_batch_ms"], 2)
    res.update(indices=args.indices, chunks=args.chunks, chunk_bytes=n, typesize=T, codec="lz4", shuffle=1, blocksize=blocksize, device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
