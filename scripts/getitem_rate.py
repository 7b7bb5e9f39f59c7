#!/usr/bin/env python3
"""Rate of many small getitem requests: 4096 random ranges of 16 items over 64 LZ4 chunks of 4 MiB (typesize 8, byte shuffle) resident on
the device - a loop of blosc_gpu_getitem, one call per range, against ONE blosc_gpu_getitem_batch (include/blosc_gpu_getitem.h).
Each side: a warm-up, then the median of ten.  blosc_gpu_getitem is a caller of the batched pipeline with one chunk and one range, so the
loop against the batch is the price of 4096 calls against one, not of another decoder.

The single calls by themselves, for comparing two builds of the library (BLOSC_AMD_LIB names the one to load; --label names it in the output):
  (a) that loop of blosc_gpu_getitem;
  (b) the first 512 of the ranges through blosc_getitem, chunks and destinations in host memory;
  (c) one whole-chunk call on a 64 MiB chunk (bench19, typesize 8, LZ4 with byte shuffle): blosc_gpu_getitem device to device, blosc_getitem
      host to host.

    python scripts/getitem_rate.py [--out profiles/getitem_ranges_rate.json] [--label NAME]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "getitem_ranges_rate.json"))
    ap.add_argument("--ranges", type=int, default=4096)
    ap.add_argument("--chunks", type=int, default=64)
    ap.add_argument("--host-ranges", type=int, default=512)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from helpers import bench19
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
    L = pkg.load()
    dev = torch.device("cuda:0")
    n, T, items = 4 << 20, 8, 16
    plain = [np.roll(bench19(n).view("<i8"), 1009 * k).view(np.uint8) for k in range(args.chunks)]
    src = [torch.from_numpy(p.copy()).to(dev) for p in plain]
    dst = [torch.empty(n + 16, dtype=torch.uint8, device=dev) for _ in plain]
    b = pkg.DeviceBatch([t.data_ptr() for t in src], [n] * args.chunks, [t.data_ptr() for t in dst], [n + 16] * args.chunks)
    assert b.compress(T, 5, 1, b"lz4") == 0 and all(c > 0 for c in b.results())
    rng = np.random.default_rng(1)
    ranges = [(int(rng.integers(0, args.chunks)), int(rng.integers(0, n // T - items)), items) for _ in range(args.ranges)]
    out = torch.zeros(args.ranges * items * T, dtype=torch.uint8, device=dev)
    slots = [out.data_ptr() + r * items * T for r in range(args.ranges)]
    want = np.concatenate([plain[c][s * T:(s + k) * T] for c, s, k in ranges])

    def loop():
        for (c, s, k), p in zip(ranges, slots):
            assert L.blosc_gpu_getitem(dst[c].data_ptr(), s, k, p, None) == k * T

    ir = pkg.ItemRanges(ranges)
    srcs = [t.data_ptr() for t in dst]

    def batch():
        assert ir.batch(srcs, slots) == 0

    # (b): the same ranges, everything in host memory
    nh = min(args.host_ranges, args.ranges)
    hchunks = [t[:c].cpu().numpy() for t, c in zip(dst, b.results())]
    hout = np.zeros(nh * items * T, np.uint8)

    def host_loop():
        for r, (c, s, k) in enumerate(ranges[:nh]):
            assert L.blosc_getitem(hchunks[c].ctypes.data, s, k, hout.ctypes.data + r * items * T) == k * T

    # (c): one whole chunk of 64 MiB
    nbig = 64 << 20
    big = bench19(nbig)
    dbig = torch.from_numpy(big).to(dev)
    dcomp = torch.empty(nbig + 16, dtype=torch.uint8, device=dev)
    bb = pkg.DeviceBatch([dbig.data_ptr()], [nbig], [dcomp.data_ptr()], [nbig + 16])
    assert bb.compress(T, 5, 1, b"lz4") == 0 and bb.results()[0] > 0
    hcomp = dcomp[:bb.results()[0]].cpu().numpy()
    dwhole = torch.zeros(nbig, dtype=torch.uint8, device=dev)
    hwhole = np.zeros(nbig, np.uint8)

    def whole_dd():
        assert L.blosc_gpu_getitem(dcomp.data_ptr(), 0, nbig // T, dwhole.data_ptr(), None) == nbig

    def whole_hh():
        assert L.blosc_getitem(hcomp.ctypes.data, 0, nbig // T, hwhole.ctypes.data) == nbig

    checks = {"loop_of_blosc_gpu_getitem": lambda: np.array_equal(out.cpu().numpy(), want),
              "one_blosc_gpu_getitem_batch": lambda: np.array_equal(out.cpu().numpy(), want),
              "loop_of_blosc_getitem_host": lambda: np.array_equal(hout, want[:hout.size]),
              "whole_chunk_device_to_device": lambda: np.array_equal(dwhole.cpu().numpy(), big),
              "whole_chunk_host_to_host": lambda: np.array_equal(hwhole, big)}
    res = {}
    for name, fn in (("loop_of_blosc_gpu_getitem", loop), ("one_blosc_gpu_getitem_batch", batch), ("loop_of_blosc_getitem_host", host_loop),
                     ("whole_chunk_device_to_device", whole_dd), ("whole_chunk_host_to_host", whole_hh)):
        out.zero_()
        fn()                                            # warm-up (arenas, code objects)
        assert checks[name](), name
        ts = []
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); ts.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = round(statistics.median(ts), 3)
        res[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
    assert ir.results() == [items * T] * args.ranges
    if args.label: res["label"] = args.label
    res.update(ranges=args.ranges, host_ranges=nh, whole_chunk_bytes=nbig, items_per_range=items, typesize=T, chunks=args.chunks, chunk_bytes=n, codec="lz4", shuffle=1,
               blocksize=int(dst[0][8:12].cpu().numpy().view("<i4")[0]), device=torch.cuda.get_device_name(0),
               speedup=round(res["loop_of_blosc_gpu_getitem_ms"] / res["one_blosc_gpu_getitem_batch_ms"], 1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
