#!/usr/bin/env python3
"""Rate of select-by-several-tests on a compressed table (include/blosc_gpu_clauses.h): scripts/where_rate.py's table - 1 GiB of float32
packed by tensors.pack_rows with the bench's setting (byte shuffle + LZ4 clevel 5, chunks of 64 MiB) - as rows of 4 bytes and as rows of 64
bytes (16 columns), every element a whole number in 0 ... 999.
  arm A   tensors.where_rows, one predicate (column 0 < 500): the existing call, k_where_mark
  arm B   the same predicate as a list of one term: tensors.where_rows_clauses, k_where_mark_terms
  arm C   a range, two terms on one field: 250 <= column 0 < 750
  arm D   8 terms on 8 different fields, ANDed (rows of 64 bytes only): column k < 900 for k = 0 ... 7
  arm E   what a caller does today for C: two where_rows calls and an intersection of the two tables in torch
  arm F   tensors.aggregate_rows_clauses over C's rows, against arm G: where + where + intersect + take_rows + torch's count / sum / min / max
The arms take turns in one process, three repetitions after a warm-up of each, and every arm's answer is checked equal to torch's on the
plaintext.  One more call of each arm under blosc_gpu_profile gives the kernels' own times.

    python scripts/clauses_rate.py [--out profiles/clauses_rate.json] [--mib 1024]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_where_mark", "k_where_mark_terms", "k_where_scan", "k_where_write", "k_aggregate_tiles", "k_aggregate_tiles_terms", "k_aggregate_chunks",
           "k_take_mark", "k_take_gather", "k_decode_streams")


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", file))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clauses_rate.json"))
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
    range_clauses = [(">=", 250.0, 0), ("<", 750.0, 0)]

    for row_bytes in (4, 64):
        table = flat.view(-1, row_bytes // 4)
        nrows = int(table.shape[0])
        cont, off, meta = tensors.pack_rows(L, table, rows_per_chunk=(64 << 20) // row_bytes, cname=b"lz4", clevel=5, shuffle=1)
        c0 = table[:, 0]
        in_range = (c0 >= 250.0) & (c0 < 750.0)

        def intersect():
            a = tensors.where_rows(L, cont, off, meta, "ge", 250.0, column=0, max_matches=nrows)[0]
            b = tensors.where_rows(L, cont, off, meta, "lt", 750.0, column=0, max_matches=nrows)[0]
            mark = torch.zeros(nrows, dtype=torch.bool, device=dev)
            mark[a] = True
            return b[mark[b]]

        def reduce_rows():
            col = tensors.take_rows(L, cont, off, meta, intersect())[:, 0]
            return int(col.numel()), float(col.sum(dtype=torch.float64)), float(col.min()), float(col.max())

        def reduce_clauses():
            a = tensors.aggregate_rows_clauses(L, cont, off, meta, column=0, clauses=range_clauses)
            return a.count, a.sum, a.min, a.max

        picked = c0[in_range]
        reduced = (int(picked.numel()), float(picked.sum(dtype=torch.float64)), float(picked.min()), float(picked.max()))
        arms = {
            "A_where_rows": (lambda: tensors.where_rows(L, cont, off, meta, "lt", 500.0, column=0, max_matches=nrows)[0], lambda: torch.nonzero(c0 < 500.0).flatten()),
            "B_one_term": (lambda: tensors.where_rows_clauses(L, cont, off, meta, [("lt", 500.0, 0)], max_matches=nrows)[0], lambda: torch.nonzero(c0 < 500.0).flatten()),
            "C_range": (lambda: tensors.where_rows_clauses(L, cont, off, meta, range_clauses, max_matches=nrows)[0], lambda: torch.nonzero(in_range).flatten()),
            "E_two_calls_intersected": (intersect, lambda: torch.nonzero(in_range).flatten()),
            "F_aggregate_clauses": (reduce_clauses, lambda: reduced),
            "G_where_where_take_torch": (reduce_rows, lambda: reduced),
        }
        if row_bytes == 64:
            eight = [("<", 900.0, k) for k in range(8)]
            arms["D_eight_fields"] = (lambda: tensors.where_rows_clauses(L, cont, off, meta, eight, max_matches=nrows)[0],
                                      lambda: torch.nonzero((table[:, :8] < 900.0).all(dim=1)).flatten())
        r = res[f"row_bytes_{row_bytes}"] = {"rows": nrows, "container_bytes": int(off[-1])}
        for name, (fn, want) in arms.items():      # the warm-up, and the answers
            got, expected = fn(), want()
            assert (torch.equal(got, expected) if torch.is_tensor(got) else got == expected), (row_bytes, name, got if not torch.is_tensor(got) else got.numel())
            r[name] = {"matches": int(got.numel()) if torch.is_tensor(got) else int(got[0])}
            del got, expected
        times = {name: [] for name in arms}
        for _ in range(3):
            for name, (fn, _) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); times[name].append((time.perf_counter() - t0) * 1e3)
                del out
        for name, (fn, _) in arms.items():
            r[name]["ms"] = [round(t, 3) for t in times[name]]
            r[name]["ms_median"] = round(statistics.median(times[name]), 3)
            L.blosc_gpu_profile(1); L.blosc_gpu_profile_reset()
            out = fn()
            torch.cuda.synchronize()
            del out
            r[name]["kernels_ms"] = {k: round(pkg.profile_get(k)[0], 3) for k in KERNELS if pkg.profile_get(k)[1]}
            r[name]["launches"] = {k: pkg.profile_get(k)[1] for k in KERNELS if pkg.profile_get(k)[1]}
            L.blosc_gpu_profile(0)
        med = lambda name: r[name]["ms_median"]
        r["B_over_A"] = round(med("B_one_term") / med("A_where_rows"), 3)
        r["A_spread_ms"] = round(max(times["A_where_rows"]) - min(times["A_where_rows"]), 3)
        r["C_over_B"] = round(med("C_range") / med("B_one_term"), 3)
        r["C_over_E"] = round(med("C_range") / med("E_two_calls_intersected"), 3)
        r["F_over_G"] = round(med("F_aggregate_clauses") / med("G_where_where_take_torch"), 3)
        if row_bytes == 64:
            r["D_per_term_ms_over_B"] = round((med("D_eight_fields") - med("B_one_term")) / 7, 3)
        del cont
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
