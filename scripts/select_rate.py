#!/usr/bin/env python3
"""What trial compression (include/blosc_gpu_select.h) costs against what a caller does without it, at the benchmark's geometry: 128
chunks of 64 MiB resident in HBM, hipEvents around the calls, warm (bench.py itself is not involved).  Three candidates per chunk: lz4
clevel 5 at typesize 8 with no filter, byte shuffle, bitshuffle.  Two data sets: bench19 throughout, and a quarter each of bench19, a
linear ramp, a random walk and random bytes.

 route A  what a caller has without the calls: one blosc_gpu_compress_packed_params sizing call (dest NULL, align 1: the offsets'
          differences are the sizes) per candidate over the whole batch, the argmin on the host, one real call with the winning rows.
          K + 1 encoder passes, K + 1 synchronisations.
 route B  one blosc_gpu_compress_packed_select.  K encoder passes, one synchronisation.

Repetitions are interleaved (`--reps` rounds of both routes in turn) and every round's figure is kept.  Memory: the caller's is the
sources plus the container (the same both ways); the library's is what the device's free memory drops by over a route that starts with
the workspace released (blosc_free_resources) - the arenas only grow, so that is its peak.

    python scripts/select_rate.py [--out profiles/select_rate.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_rate.json"))
    ap.add_argument("--chunks", type=int, default=128)
    ap.add_argument("--chunk-mib", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3, help="timed calls per route and round (the median is the round's figure)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from helpers import DATASETS
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
    L = pkg.load()
    L.blosc_init()      # (blosc_free_resources releases the workspace of an initialised library only)
    dev = torch.device("cuda:0")
    n, size = args.chunks, args.chunk_mib << 20
    sizes = [size] * n
    cands = [pkg.cparams(8, 5, shuffle, b"lz4") for shuffle in (0, 1, 2)]
    K = len(cands)
    first = [K * i for i in range(n + 1)]
    whole = pkg.PackedBatch(n)
    cap = whole.bound(sizes, 256)
    cont = torch.empty(cap, dtype=torch.uint8, device=dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        return a.elapsed_time(b)

    res = {"device": torch.cuda.get_device_name(0), "chunks": n, "chunk_bytes": size, "reps": args.reps, "steps": args.steps,
           "candidates": ["lz4 clevel 5 typesize 8 noshuffle", "... shuffle", "... bitshuffle"], "data": {}}
    for label, names in (("bench19", ["bench19"]), ("mixed", ["bench19", "linspace", "randwalk", "random"])):
        kinds = [torch.from_numpy(DATASETS[nm](size)).to(dev) for nm in names]
        data = torch.cat([kinds[k * len(kinds) // n] for k in range(n)])
        ptrs = [data.data_ptr() + k * size for k in range(n)]
        state = {}

        def route_a():
            table = []
            for c in cands:
                assert whole.compress_params(ptrs, sizes, [c] * n, None, 0, 1) == 0
                off = whole.offsets()
                table.append([off[i + 1] - off[i] for i in range(n)])
            choice = [min(range(K), key=lambda k: (table[k][i], k)) for i in range(n)]
            assert whole.compress_params(ptrs, sizes, [cands[c] for c in choice], cont.data_ptr(), cap, 256) == 0 and min(whole.results()) > 0
            state["a"] = (choice, whole.results(), whole.offsets())

        def route_b():
            assert whole.compress_select(ptrs, sizes, first, cands * n, cont.data_ptr(), cap, 256) == 0 and min(whole.results()) > 0
            state["b"] = (whole.choices(), whole.results(), whole.offsets())

        legs = {"route_a": route_a, "route_b": route_b}
        lib_bytes = {}
        for name, fn in legs.items():      # the library's memory, from a released workspace; the calls after it are warm
            assert L.blosc_free_resources() == 0
            torch.cuda.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            fn(); fn()
            lib_bytes[name] = free0 - torch.cuda.mem_get_info()[0]
        assert state["a"] == state["b"], "the two routes disagree about winners, sizes or offsets"
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for name, fn in legs.items():
                fn()                                             # (the route in front of this one left other tables behind)
                ms[name].append(round(statistics.median(timed(fn) for _ in range(args.steps)), 3))
        choice = state["b"][0]
        res["data"][label] = {"ms": ms, "median_ms": {k: statistics.median(v) for k, v in ms.items()},
                              "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ms.items()},
                              "library_bytes": lib_bytes, "caller_bytes": {k: n * size + cap for k in legs},
                              "winners": [choice.count(k) for k in range(K)], "container_bytes": state["b"][2][-1],
                              "encoder_passes": {"route_a": K + 1, "route_b": K}, "synchronisations": {"route_a": K + 1, "route_b": 1}}
        del data, kinds
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
