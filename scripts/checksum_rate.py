#!/usr/bin/env python3
"""Rates of include/blosc_gpu_checksum.h and of the device path of c-blosc_amd/blpk.py, each against what a caller had before.

Digest rate: 128 runs of 64 MiB of random bytes resident in HBM through one blosc_gpu_checksum_batch per kind - a warm-up, then the median
of `--reps` calls (wall clock around the synchronous call).  Next to it the earlier way to the same digests: a device-to-host copy of a
run and Python's zlib over it, timed on `--host-runs` of the runs (median of three per run) and scaled to all of them.

File write: 1 GiB of bench19 data and 1 GiB of random bytes resident on the device into an io.BytesIO - blpk.pack_device against a
device-to-host copy of the plain data followed by blpk.pack.  Extra device memory: what the device reports as used after the route, above
what it reported before it, with the library's arenas and torch's cache released in front of each route (both keep what they grew to).

    python scripts/checksum_rate.py [--out profiles/checksum_rate.json]
"""
import argparse
import importlib.util
import io
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_BYTES_PER_S = 8e12


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checksum_rate.json"))
    ap.add_argument("--runs", type=int, default=128)
    ap.add_argument("--run-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=8)
    ap.add_argument("--file-mib", type=int, default=1024)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from helpers import bench19

    def module(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", path))
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
        return m
    pkg, blpk = module("c_blosc_amd", "__init__.py"), module("blpk", "blpk.py")
    L = pkg.load()
    L.blosc_init()                                                               # blosc_free_resources below releases nothing without it
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "digest": {}, "file_write": {}}

    # ---- digest rate ----
    n = args.run_mib << 20
    data = torch.randint(0, 256, (args.runs * n,), dtype=torch.uint8, device=dev)
    ptrs, sizes = [data.data_ptr() + k * n for k in range(args.runs)], [n] * args.runs
    total = args.runs * n
    for kind, name, f in ((1, "adler32", zlib.adler32), (2, "crc32", zlib.crc32)):
        got = pkg.checksums(kind, ptrs, sizes)                                   # warm-up
        ms = median_ms(lambda: pkg.checksums(kind, ptrs, sizes), args.reps)
        host_ms, want = [], []
        for k in range(args.host_runs):
            one = []
            for _ in range(3):
                torch.cuda.synchronize()
                t = time.perf_counter()
                h = data[k * n:(k + 1) * n].cpu().numpy()
                d = f(h) & 0xffffffff
                one.append((time.perf_counter() - t) * 1e3)
            host_ms.append(statistics.median(one)); want.append(d)
        assert got[:args.host_runs] == want, name
        per_run = statistics.median(host_ms)
        res["digest"][name] = {
            "runs": args.runs, "run_bytes": n, "reps": args.reps,
            "device_ms": round(ms, 3), "device_GBps": round(total / ms / 1e6, 1), "fraction_of_8TBps": round(total / (ms * 1e-3) / HBM_BYTES_PER_S, 4),
            "host_runs_timed": args.host_runs, "host_ms_per_run_copy_plus_zlib": round(per_run, 2),
            "host_ms_all_runs_scaled": round(per_run * args.runs, 1), "host_GBps": round(n / per_run / 1e6, 2),
            "device_is_faster": bool(ms < per_run * args.runs),
        }
        print(name, json.dumps(res["digest"][name]), flush=True)
    del data

    # ---- file write ----
    def used():
        torch.cuda.synchronize()
        free, tot = torch.cuda.mem_get_info()
        return tot - free

    fn = args.file_mib << 20
    sets = {"bench19": lambda: torch.from_numpy(bench19(fn)).to(dev),
            "random": lambda: torch.randint(0, 256, (fn,), dtype=torch.uint8, device=dev)}
    for dname, make in sets.items():
        src = make()

        def by_device():
            out = io.BytesIO()
            blpk.pack_device(L, src.data_ptr(), fn, out, chunk_size=1 << 20, typesize=8, cname=b"lz4", checksum=1)
            return out

        def by_host():
            out = io.BytesIO()
            blpk.pack(L, src.cpu().numpy(), out, chunk_size=1 << 20, typesize=8, cname=b"lz4", checksum=1)
            return out
        entry = {"bytes": fn, "chunk_size": 1 << 20, "cname": "lz4", "checksum": "adler32", "reps": 3}
        files = {}
        for route, fnc in (("pack_device", by_device), ("copy_then_pack", by_host)):
            L.blosc_free_resources(); torch.cuda.empty_cache()
            base = used()
            files[route] = fnc().getvalue()                                       # warm-up; the arenas and the cache grow to what the route needs
            extra = used() - base
            ms = median_ms(fnc, 3)
            entry[route] = {"ms": round(ms, 1), "GBps_of_plain_data": round(fn / ms / 1e6, 2), "extra_device_MiB": round(extra / 2**20, 1),
                            "file_bytes": len(files[route])}
        entry["same_file"] = files["pack_device"] == files["copy_then_pack"]
        entry["device_is_faster"] = entry["pack_device"]["ms"] < entry["copy_then_pack"]["ms"]
        res["file_write"][dname] = entry
        print(dname, json.dumps(entry), flush=True)
        del src, files
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
