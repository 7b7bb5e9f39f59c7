#!/usr/bin/env python3
"""Rate of a filtered reduction on a compressed table: where_rate.py's table - 1 GiB of float32 with values 0 ... 999 packed by
tensors.pack_rows with the bench's setting (byte shuffle + LZ4 clevel 5, chunks of 64 MiB), once as rows of 4 bytes and once as rows of 64
bytes with the field at offset 0 - and its filter `< bound` at about 1 % and about 50 % of the rows.  Count, sum, min and max of the column over
the matching rows, three ways:
  arm A   tensors.aggregate_rows(where=("lt", bound, 0)): ONE blosc_gpu_aggregate_packed (include/blosc_gpu_aggregate.h)
  arm B   tensors.where_rows(max_matches=nrows), tensors.take_rows of the matches, torch reductions over the copy
  arm C   tensors.unpack_tensors of the whole container, a torch comparison and torch reductions over the masked column
The arms take turns, three repetitions after a warm-up of each; the four answers must be equal (the sums are exact: integers below 2^53).
One more call of each arm under blosc_gpu_profile gives the kernels' own times; torch's peak of allocated bytes and the device memory a call
takes are where_rate.py's.

    python scripts/aggregate_rate.py [--out profiles/aggregate_rate.json] [--mib 1024]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_aggregate_tiles", "k_aggregate_chunks", "k_where_mark", "k_where_scan", "k_where_write", "k_take_mark", "k_take_gather", "k_decode_streams")


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", file))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggregate_rate.json"))
    ap.add_argument("--mib", type=int, default=1024)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    pkg = load("c_blosc_amd", "__init__.py")
    tensors = load("c_blosc_amd_tensors", "tensors.py")
    L = pkg.load()
    L.blosc_init()
    dev = torch.device("cuda:0")
    elements = (args.mib << 20) // 4
    g = torch.Generator(device=dev); g.manual_seed(19)
    flat = torch.randint(0, 1000, (elements,), device=dev, generator=g).to(torch.float32)
    res = {"table_bytes": elements * 4, "dtype": "float32", "codec": "lz4", "clevel": 5, "shuffle": 1, "chunk_bytes": 64 << 20, "device": torch.cuda.get_device_name(0)}

    def taken(fn):
        """(torch's peak of allocated bytes during fn, the device's free memory fn took away: library arenas + torch's reservations)"""
        torch.cuda.synchronize()
        assert L.blosc_free_resources() == 0
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base, free0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
        out = fn()
        torch.cuda.synchronize()
        peak, drop = torch.cuda.max_memory_allocated() - base, free0 - torch.cuda.mem_get_info()[0]
        del out
        return int(peak), int(drop)

    def reduced(v):
        return (int(v.numel()), v.double().sum().item(), v.min().item(), v.max().item())

    for row_bytes in (4, 64):
        table = flat if row_bytes == 4 else flat.view(-1, row_bytes // 4)
        nrows = int(table.shape[0])
        cont, off, meta = tensors.pack_rows(L, table, rows_per_chunk=(64 << 20) // row_bytes, cname=b"lz4", clevel=5, shuffle=1)
        for share, bound in (("1_percent", 10.0), ("50_percent", 500.0)):
            def arm_a():
                a = tensors.aggregate_rows(L, cont, off, meta, column=0, where=("lt", bound, 0))
                return (a.count, a.sum, a.min, a.max)

            def arm_b():
                index, _ = tensors.where_rows(L, cont, off, meta, "lt", bound, column=0, max_matches=nrows)
                rows = tensors.take_rows(L, cont, off, meta, index)
                return reduced(rows if rows.dim() == 1 else rows[:, 0])

            def arm_c():
                t = torch.cat(tensors.unpack_tensors(L, cont, off, meta)) if len(meta) > 1 else tensors.unpack_tensors(L, cont, off, meta)[0]
                col = t if t.dim() == 1 else t[:, 0]
                return reduced(col[col < bound])

            arms = (("aggregate_rows", arm_a), ("where_take_reduce", arm_b), ("unpack_compare_reduce", arm_c))
            key = f"row_bytes_{row_bytes}_{share}"
            r = res[key] = {"rows": nrows, "container_bytes": int(off[-1])}
            answers = [fn() for _, fn in arms]      # the warm-up, and the answers
            assert answers[0] == answers[1] == answers[2], (key, answers)
            r["matches"], r["sum"] = answers[0][0], answers[0][1]
            times = {name: [] for name, _ in arms}
            for _ in range(3):
                for name, fn in arms:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); times[name].append((time.perf_counter() - t0) * 1e3)
            for name, fn in arms:
                r[name + "_ms"] = [round(t, 3) for t in times[name]]
                r[name + "_ms_median"] = round(statistics.median(times[name]), 3)
                L.blosc_gpu_profile(1); L.blosc_gpu_profile_reset()
                fn()
                torch.cuda.synchronize()
                r[name + "_kernels_ms"] = {k: round(pkg.profile_get(k)[0], 3) for k in KERNELS if pkg.profile_get(k)[1]}
                r[name + "_launches"] = {k: pkg.profile_get(k)[1] for k in KERNELS if pkg.profile_get(k)[1]}
                L.blosc_gpu_profile(0)
                r[name + "_torch_peak_bytes"], r[name + "_device_bytes_taken"] = taken(fn)
        del cont
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
