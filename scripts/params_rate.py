#!/usr/bin/env python3
"""What the compress calls with parameters per chunk (include/blosc_gpu_params.h) cost and buy, at the benchmark's geometry: 128 chunks
of 64 MiB of bench19 data resident in HBM, hipEvents around the calls, warm (bench.py itself is not involved).

 (a) configuration 2 (byte-shuffle + LZ4, clevel 5, typesize 8) as ONE setting: blosc_gpu_compress_packed against
     blosc_gpu_compress_packed_params with the same parameters in every slot.  The launches are the same; the difference is host side.
 (b) the same 128 chunks with four settings, 32 chunks each and interleaved - lz4 / typesize 8, lz4 / typesize 4, zstd clevel 3 /
     typesize 8, zstd clevel 3 / typesize 2 - as four blosc_gpu_compress_packed calls (one per setting, their times added up) against
     one blosc_gpu_compress_packed_params; with the synchronisations and kernel launches each way (blosc_gpu_profile's counts).

`--lib` names another build of the library, e.g. the parent commit's, which has only the existing calls: its legs are then the ones
measured.  Repetitions are interleaved (`--reps` rounds of every leg in turn) and every round's figure is kept, so that a difference
between two builds or two calls can be held against the spread of one of them.

    python scripts/params_rate.py [--lib PATH] [--out profiles/params_rate.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNELS = ["k_encode_streams", "k_zstd_encode", "k_lz4hc_encode", "k_zlib_encode", "k_shuffle", "k_bitshuffle", "k_chunk_scan", "k_packed_layout",
           "k_chunk_compact"]
# blosc_gpu_profile counts one entry per timed scope; what a scope launches (engine.hip): the scan, the compaction, an encoder variant and
# k_shuffle are one kernel each, k_packed_layout's scope holds the layout and the header kernel, k_bitshuffle's the fast and the generic one.
# k_encode_plan (one launch per call) has no scope.
PER_SCOPE = {"k_packed_layout": 2, "k_bitshuffle": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "params_rate.json"))
    ap.add_argument("--chunks", type=int, default=128)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5, help="timed calls per leg and round (the median is the round's figure)")
    args = ap.parse_args()
    if args.lib:
        os.environ["BLOSC_AMD_LIB"] = os.path.abspath(args.lib)
    import torch
    torch.cuda.init()
    from helpers import bench19
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
    L = pkg.load()
    has_params = hasattr(L, "blosc_gpu_compress_packed_params")
    dev = torch.device("cuda:0")
    n, size = args.chunks, args.chunk_mib << 20
    one = torch.from_numpy(bench19(size)).to(dev)
    data = one.repeat(n)
    ptrs, sizes = [data.data_ptr() + k * size for k in range(n)], [size] * n
    cap = n * (size // 4)
    cont = torch.empty(cap, dtype=torch.uint8, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b)

    cfg2 = (8, 5, 1, b"lz4")
    four = [(8, 5, 1, b"lz4"), (4, 5, 1, b"lz4"), (8, 3, 1, b"zstd"), (2, 3, 1, b"zstd")]
    groups = [[k for k in range(n) if k % 4 == g] for g in range(4)]
    whole = pkg.PackedBatch(n)
    parts = [pkg.PackedBatch(len(g)) for g in groups]

    def old_one():
        assert whole.compress(ptrs, sizes, cont.data_ptr(), cap, *cfg2, 0, 256) == 0 and min(whole.results()) > 0

    def new_one():
        assert whole.compress_params(ptrs, sizes, [pkg.cparams(*cfg2)] * n, cont.data_ptr(), cap, 256) == 0 and min(whole.results()) > 0

    def four_calls():
        at = 0
        for g, b, s in zip(groups, parts, four):
            assert b.compress([ptrs[k] for k in g], [size] * len(g), cont.data_ptr() + at, cap - at, *s, 0, 256) == 0 and min(b.results()) > 0
            at += b.offsets()[-1]

    def one_call():
        assert whole.compress_params(ptrs, sizes, [pkg.cparams(*four[k % 4]) for k in range(n)], cont.data_ptr(), cap, 256) == 0 and min(whole.results()) > 0

    legs = {"a_packed": old_one, "b_four_calls": four_calls}
    if has_params:
        legs.update({"a_packed_params": new_one, "b_one_call": one_call})
    res = {"device": torch.cuda.get_device_name(0), "library": args.lib or "the tree's", "chunks": n, "chunk_bytes": size, "reps": args.reps,
           "steps": args.steps, "settings_b": [f"{s[3].decode()} clevel {s[1]} typesize {s[0]}" for s in four], "ms": {k: [] for k in legs}}
    for fn in legs.values():
        fn(); fn()                                           # warm: arenas, the table cache, the trained queue order
    for _ in range(args.reps):
        for name, fn in legs.items():
            fn()                                             # (the leg in front of this one left other tables behind)
            res["ms"][name].append(round(statistics.median(timed(fn) for _ in range(args.steps)), 3))
    res["median_ms"] = {k: statistics.median(v) for k, v in res["ms"].items()}
    res["spread_ms"] = {k: round(max(v) - min(v), 3) for k, v in res["ms"].items()}
    # synchronisations (one per call) and kernel launches each way
    counts = {}
    for name, fn, calls in (("b_four_calls", four_calls, 4), ("b_one_call", one_call, 1), ("a_packed", old_one, 1), ("a_packed_params", new_one, 1)):
        if name not in legs:
            continue
        L.blosc_gpu_profile(1); L.blosc_gpu_profile_reset()
        fn()
        scopes = {k: pkg.profile_get(k)[1] for k in KERNELS}
        L.blosc_gpu_profile(0); L.blosc_gpu_profile_reset()
        counts[name] = {"calls": calls, "synchronisations": calls, "kernel_launches": sum(c * PER_SCOPE.get(k, 1) for k, c in scopes.items()) + calls,
                        "timed_scopes": {k: c for k, c in scopes.items() if c}}
    res["counts"] = counts
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
