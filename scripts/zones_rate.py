#!/usr/bin/env python3
"""Rate of zone maps on a compressed table (include/blosc_gpu_zones.h): scripts/where_rate.py's table - 1 GiB of float32 packed by
tensors.pack_rows with the bench's setting (byte shuffle + LZ4 clevel 5, chunks of 64 MiB, 16 of them) - as rows of 64 bytes (16 columns).
Column 0 is the row number (it ascends; 2^24 rows are exact in float32), every other element a whole number in 0 ... 999.
  arm A   tensors.zone_map over the 16 columns (one blosc_gpu_aggregate_fields_packed) against 16 tensors.aggregate_rows calls
  arm B   a range of column 0 that lives in 1 of the 16 chunks: tensors.where_rows_clauses and aggregate_rows_clauses with and without zones
  arm C   a range that excludes no chunk (every row of column 0, column 1 < 500), with and without zones: what the rule costs on the host
The arms take turns in one process, three repetitions after a warm-up of each, and every arm's answer is checked: the map against the 16
calls, the zoned calls against the unzoned ones and against torch on the plaintext.  One more call of each arm under blosc_gpu_profile gives
the kernels' own times.

    python scripts/zones_rate.py [--out profiles/zones_rate.json] [--mib 1024]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("k_where_mark_terms", "k_where_scan", "k_where_write", "k_aggregate_tiles", "k_aggregate_tiles_terms", "k_aggregate_tiles_fields", "k_aggregate_chunks",
           "k_aggregate_chunks_fields", "k_decode_streams")


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", file))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zones_rate.json"))
    ap.add_argument("--mib", type=int, default=1024)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    pkg = load("c_blosc_amd", "__init__.py")
    tensors = load("c_blosc_amd_tensors", "tensors.py")
    L = pkg.load()
    L.blosc_init()
    dev = torch.device("cuda:0")
    nrows = (args.mib << 20) // 64
    assert nrows <= 1 << 24, "the row number is exact in float32 up to 2^24 rows"
    g = torch.Generator(device=dev); g.manual_seed(19)
    table = torch.randint(0, 1000, (nrows, 16), device=dev, generator=g).to(torch.float32)
    table[:, 0] = torch.arange(nrows, device=dev, dtype=torch.float32)
    per_chunk = (64 << 20) // 64
    cont, off, meta = tensors.pack_rows(L, table, rows_per_chunk=per_chunk, cname=b"lz4", clevel=5, shuffle=1)
    nchunks = len(meta)
    res = {"table_bytes": nrows * 64, "rows": nrows, "row_bytes": 64, "chunks": nchunks, "container_bytes": int(off[-1]), "dtype": "float32", "codec": "lz4",
           "clevel": 5, "shuffle": 1, "chunk_bytes": 64 << 20, "device": torch.cuda.get_device_name(0)}
    columns = list(range(16))
    zones = tensors.zone_map(L, cont, off, meta, columns)

    # ---- the ranges: inside chunk nchunks / 2, half of its rows; and one that no chunk's entry excludes ----
    k = nchunks // 2
    lo, hi = float(k * per_chunk + per_chunk // 4), float(k * per_chunk + 3 * per_chunk // 4)
    one_chunk = [(">=", lo, 0), ("<", hi, 0)]
    everywhere = [(">=", 0.0, 0), ("<", 500.0, 1)]
    c0, c1 = table[:, 0], table[:, 1]
    masks = {"B": (c0 >= lo) & (c0 < hi), "C": (c0 >= 0.0) & (c1 < 500.0)}

    def sixteen_calls():
        return [tensors.aggregate_rows(L, cont, off, meta, column=c) for c in columns]

    def summary(a):
        return (a.count, a.sum, a.min, a.max)

    def where(clauses, z):
        return tensors.where_rows_clauses(L, cont, off, meta, clauses, max_matches=nrows, zones=z)[0]

    def aggregate(clauses, z):
        return summary(tensors.aggregate_rows_clauses(L, cont, off, meta, column=2, clauses=clauses, zones=z))

    def reduced(mask):
        col = table[:, 2][mask]
        return (int(col.numel()), float(col.sum(dtype=torch.float64)), float(col.min()), float(col.max()))

    import struct

    def entries(got):
        """(count, min, max) per chunk and column, of a Zones or of sixteen Aggregated: compared outside the timed call"""
        if isinstance(got, tensors.Zones):
            return [[(int(e["count"]), struct.unpack("<f", bytes(e["min"])[:4])[0], struct.unpack("<f", bytes(e["max"])[:4])[0]) for e in row] for row in got.entries]
        return [[(got[c].chunks[i].count, got[c].chunks[i].min, got[c].chunks[i].max) for c in columns] for i in range(nchunks)]

    want_map = entries(sixteen_calls())
    assert all(want_map[i][0] == (per_chunk, float(i * per_chunk), float((i + 1) * per_chunk - 1)) for i in range(nchunks))
    arms = {
        "A_zone_map_16_columns": (lambda: tensors.zone_map(L, cont, off, meta, columns), lambda: want_map),
        "A_sixteen_aggregate_calls": (sixteen_calls, lambda: want_map),
        "B_where_one_chunk_zoned": (lambda: where(one_chunk, zones), lambda: torch.nonzero(masks["B"]).flatten()),
        "B_where_one_chunk": (lambda: where(one_chunk, None), lambda: torch.nonzero(masks["B"]).flatten()),
        "B_aggregate_one_chunk_zoned": (lambda: aggregate(one_chunk, zones), lambda: reduced(masks["B"])),
        "B_aggregate_one_chunk": (lambda: aggregate(one_chunk, None), lambda: reduced(masks["B"])),
        "C_where_everywhere_zoned": (lambda: where(everywhere, zones), lambda: torch.nonzero(masks["C"]).flatten()),
        "C_where_everywhere": (lambda: where(everywhere, None), lambda: torch.nonzero(masks["C"]).flatten()),
        "C_aggregate_everywhere_zoned": (lambda: aggregate(everywhere, zones), lambda: reduced(masks["C"])),
        "C_aggregate_everywhere": (lambda: aggregate(everywhere, None), lambda: reduced(masks["C"])),
    }
    r = res["arms"] = {}
    for name, (fn, want) in arms.items():      # the warm-up, and the answers
        got, expected = fn(), want()
        if name.startswith("A_"): got = entries(got)
        assert (torch.equal(got, expected) if torch.is_tensor(got) else got == expected), (name, got if not torch.is_tensor(got) else got.numel())
        r[name] = {"matches": int(got.numel())} if torch.is_tensor(got) else {}
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
    spread = lambda name: round(max(times[name]) - min(times[name]), 3)
    res["A_map_over_sixteen_calls"] = round(med("A_zone_map_16_columns") / med("A_sixteen_aggregate_calls"), 4)
    res["B_where_zoned_over_unzoned"] = round(med("B_where_one_chunk_zoned") / med("B_where_one_chunk"), 3)
    res["B_aggregate_zoned_over_unzoned"] = round(med("B_aggregate_one_chunk_zoned") / med("B_aggregate_one_chunk"), 3)
    res["C_where_zoned_minus_unzoned_ms"] = round(med("C_where_everywhere_zoned") - med("C_where_everywhere"), 3)
    res["C_where_unzoned_spread_ms"] = spread("C_where_everywhere")
    res["C_aggregate_zoned_minus_unzoned_ms"] = round(med("C_aggregate_everywhere_zoned") - med("C_aggregate_everywhere"), 3)
    res["C_aggregate_unzoned_spread_ms"] = spread("C_aggregate_everywhere")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
