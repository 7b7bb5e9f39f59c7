#!/usr/bin/env python3
"""Rate of index_copy_ on a compressed table: distinct random rows, resident on the device, written into a packed container of 64 LZ4 chunks
of 4 MiB (typesize 8, byte shuffle, 1 MiB blocks - scripts/take_rate.py's table).  ONE blosc_gpu_put_packed (include/blosc_gpu_put.h) against
the route a caller has without it: blosc_gpu_decompress_packed of the whole container, Tensor.index_copy_ on the plaintext,
blosc_gpu_compress_packed of all of it.  Row sizes 8, 64 and 1024 bytes; the indices touch 1, 8 and all 64 chunks.
Each side: a warm-up, then the median of ten; both run in one session, and the plaintexts of their containers must be equal (and equal numpy's).
One more call of the put under blosc_gpu_profile gives the kernels' own times.  Library memory: the device memory the library's grow-only
arenas take for one call after blosc_free_resources, read from the device's free memory; the second route also needs the whole plaintext,
which its caller holds.

    python scripts/put_rate.py [--out profiles/put_rate.json] [--indices 65536]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KERNELS = ("k_take_mark", "k_put_claim", "k_put_scatter", "k_put_assemble", "k_decode_streams", "k_encode_streams")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "put_rate.json"))
    ap.add_argument("--indices", type=int, default=1 << 16)
    ap.add_argument("--chunks", type=int, default=64)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from helpers import bench19
    spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
    L = pkg.load()
    L.blosc_init()
    dev = torch.device("cuda:0")
    n, T, nch, align = 4 << 20, 8, args.chunks, 256
    forced = (1 << 20) // T      # (a split block is typesize x the forced size)
    plain = [np.roll(bench19(n).view("<i8"), 1009 * k).view(np.uint8) for k in range(nch)]
    table = np.concatenate(plain)
    flat = torch.from_numpy(table).to(dev)
    pb = pkg.PackedBatch(nch)
    cap = pb.bound([n] * nch, align)
    cont = torch.empty(cap, dtype=torch.uint8, device=dev)
    assert pb.compress([flat.data_ptr() + k * n for k in range(nch)], [n] * nch, cont.data_ptr(), cap, T, 5, 1, b"lz4", forced, align) == 0
    off = pb.offsets()
    assert all(c > 0 for c in pb.results())
    params = [pkg.cparams(T, 5, 1, b"lz4", forced) for _ in range(nch)]
    new_put = torch.empty(cap, dtype=torch.uint8, device=dev)
    new_old = torch.empty(cap, dtype=torch.uint8, device=dev)
    work = torch.empty(nch * n, dtype=torch.uint8, device=dev)      # the second route's plaintext
    back = torch.empty(nch * n, dtype=torch.uint8, device=dev)

    def library_bytes(fn):
        torch.cuda.synchronize()
        assert L.blosc_free_resources() == 0
        free0 = torch.cuda.mem_get_info()[0]
        fn()
        torch.cuda.synchronize()
        return int(free0 - torch.cuda.mem_get_info()[0])

    res = {}
    for row_bytes in (8, 64, 1024):
        per_chunk = n // row_bytes
        for touch in (1, 8, nch):
            g = torch.Generator(device=dev); g.manual_seed(row_bytes * 100 + touch)
            nidx = min(args.indices, touch * per_chunk // 2)
            index = torch.randperm(touch * per_chunk, device=dev, generator=g)[:nidx].contiguous()
            rows = torch.randint(0, 256, (nidx, row_bytes), dtype=torch.uint8, device=dev, generator=g)
            want = table.reshape(-1, row_bytes).copy()
            want[index.cpu().numpy()] = rows.cpu().numpy()
            put = pkg.RowPut(row_bytes)
            sizes = pkg.PackedBatch(nch)
            again = pkg.PackedBatch(nch)

            def one_put():
                assert put.packed(cont.data_ptr(), off[-1], off, index.data_ptr(), nidx, rows.data_ptr(), params, new_put.data_ptr(), cap, align) == 0
                assert put.failed() == 0 and put.rewritten().count(1) == touch

            def whole_table():
                assert sizes.decompress(cont.data_ptr(), off[-1], off, work.data_ptr(), nch * n) == 0
                work.view(-1, row_bytes).index_copy_(0, index, rows)
                assert again.compress([work.data_ptr() + k * n for k in range(nch)], [n] * nch, new_old.data_ptr(), cap, T, 5, 1, b"lz4", forced, align) == 0

            def plaintext_of(container, offsets):
                rd = pkg.PackedBatch(nch)
                assert rd.decompress(container.data_ptr(), offsets[-1], offsets, back.data_ptr(), nch * n) == 0 and rd.results() == [n] * nch
                return back.cpu().numpy().reshape(-1, row_bytes)

            key = f"row_bytes_{row_bytes}_chunks_touched_{touch}"
            res[key] = {"indices": nidx}
            for name, fn, outputs in (("one_blosc_gpu_put_packed", one_put, lambda: (new_put, put.offsets())),
                                      ("decompress_index_copy_compress", whole_table, lambda: (new_old, again.offsets()))):
                res[key][name + "_library_bytes"] = library_bytes(fn)      # (the first call: arenas, code objects)
                assert np.array_equal(plaintext_of(*outputs()), want), (name, key)
                ts = []
                for _ in range(10):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
                res[key][name + "_ms"] = round(statistics.median(ts), 3)
                res[key][name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
                L.blosc_gpu_profile(1); L.blosc_gpu_profile_reset()
                fn()
                res[key][name + "_kernels_ms"] = {k: round(pkg.profile_get(k)[0], 3) for k in KERNELS if pkg.profile_get(k)[1]}
                L.blosc_gpu_profile(0)
            res[key]["containers_byte_equal"] = bool(put.offsets() == again.offsets() and torch.equal(new_put[:put.offsets()[-1]], new_old[:again.offsets()[-1]]))
            res[key]["whole_table_over_put"] = round(res[key]["decompress_index_copy_compress_ms"] / res[key]["one_blosc_gpu_put_packed_ms"], 2)
    res.update(chunks=nch, chunk_bytes=n, typesize=T, codec="lz4", shuffle=1, align=align, caller_plaintext_bytes_of_the_whole_table_route=nch * n,
               device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1); f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
