"""blosc_gpu_take_batch / blosc_gpu_take_packed on the device (include/blosc_gpu_take.h): rows of compressed chunks by an index table in
device memory.  The checks and cases are tests/take_checks.py's: expected rows are numpy slices of the oracle's plaintexts, a damaged
block's code is the oracle's orc_getitem."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import TorchMem, pick_damage, plain
from helpers import header, orc_compress, ref_compress
from take_checks import (BLOCKSIZE, MANY_COUNTS, N, ROW_SIZES, TakeSource, batch_chunks, check_census_failure, check_take, chunk_rows, damaged_rows,
                         index_sets, many_chunks, offsets_for, pack_container, plaintext)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = ["lz4", "blosclz", "zstd", "zlib"]
GRID = [(cname, T, shuffle) for T in (1, 4, 8, 17) for shuffle in (0, 1, 2) for cname in CODECS]      # 48 settings
STRIDE = 11                                                                                            # ... every 11th of them per row size, from a start of its own


@pytest.fixture(scope="module")
def mem(pkg):
    return TorchMem()


def lib_chunk(pkg, mem, data, T, shuffle, cname, blocksize):
    """blosc_gpu_compress_batch of one buffer"""
    src, dst = mem.put(data), mem.filled(data.size + 16, 0)
    b = pkg.DeviceBatch([src[1]], [data.size], [dst[1]], [data.size + 16])
    assert b.compress(T, 5, shuffle, cname.encode(), blocksize) == 0 and b.results()[0] > 0, b.results()
    return mem.get(dst[0])[:b.results()[0]].copy()


def writer(pkg, mem, oracle, ref, cname, T, shuffle, turn):
    """chunk k by the oracle (LZ4, BloscLZ), by the reference where it is built, by this library, in turns"""
    def write(k, data):
        who = (k + turn) % 3
        if who == 0 and cname in ("lz4", "blosclz"): return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        if who != 2 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
        return lib_chunk(pkg, mem, data, T, shuffle, cname, BLOCKSIZE)
    return write


def batch(pkg, mem, oracle, ref, setting, row_bytes, turn=0):
    cname, T, shuffle = setting
    chunks = batch_chunks(oracle, writer(pkg, mem, oracle, ref, cname, T, shuffle, turn), row_bytes, 1 if T == 17 else 8)      # the blocks of a split typesize are widened to 64 KiB
    assert -(-header(chunks[0])["nbytes"] // header(chunks[0])["blocksize"]) >= 3 and not header(chunks[0])["flags"] & 2, header(chunks[0])
    return chunks, plaintext(oracle, chunks)


@pytest.mark.parametrize("row_bytes", ROW_SIZES)
def test_rows_of_every_index_set(pkg, lib, mem, oracle, ref, row_bytes):
    """every index set with and without a status table, dest at its offsets from a 16-byte boundary, both entry points"""
    at = ROW_SIZES.index(row_bytes)
    settings = GRID[(5 * at) % STRIDE::STRIDE]
    assert len(settings) >= 4
    for n, setting in enumerate(settings):
        chunks, rows_plain = batch(pkg, mem, oracle, ref, setting, row_bytes, turn=at + n)
        src = TakeSource(mem, chunks=chunks) if n % 2 == 0 else TakeSource(mem, *(None,) + pack_container(chunks))
        sets = index_sets(chunks, row_bytes)
        for name, index in sets.items():
            for with_status in (True, False):
                check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 0, with_status, what=(setting, name))
        edges = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"][:500]])
        for offset in offsets_for(row_bytes):
            check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, edges, offset, offset % 2 == 1, what=(setting, "edges"))


def test_passes_depend_on_bytes_and_give_the_same(pkg, lib, mem, oracle, ref):
    """a pass bound of 16 KiB: one gather launch per pass, as many passes as the touched bytes ask for, the answers those of one pass"""
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    lib.blosc_gpu_profile(1)
    try:
        for row_bytes, setting in ((17, ("blosclz", 17, 2)), (4080, ("zstd", 17, 1)), (96, ("lz4", 8, 1))):
            chunks, rows_plain = batch(pkg, mem, oracle, ref, setting, row_bytes, turn=1)
            sets = index_sets(chunks, row_bytes)
            index = np.concatenate([sets["out of bounds"], sets["random"], sets["edges"]])
            decoded = sum(1 for c in chunks if header(c)["nbytes"] and not header(c)["flags"] & 2)
            for src in (TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks))):
                lib.blosc_gpu_profile_reset()
                check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 3, True, what=("16 KiB passes", setting))
                assert pkg.profile_get("k_take_gather")[1] == decoded and pkg.profile_get("k_take_mark")[1] == 1      # every chunk beyond the bound: a pass of its own
                check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 0, False, what=("16 KiB passes", setting))
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", CODECS)
def test_a_damaged_block_fails_the_rows_that_touch_it(pkg, lib, mem, oracle, ref, cname):
    """a chunk with block 2 damaged next to its intact copy in one call: the rows of the block and the rows crossing into it answer the oracle's
    code and are unwritten, all other rows of both chunks are served"""
    data = plain(N)
    if cname in ("lz4", "blosclz"): chunk = orc_compress(oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
    elif ref is not None: chunk = ref_compress(ref, data, 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
    else: chunk = lib_chunk(pkg, mem, data, 17, 1, cname, BLOCKSIZE)
    found, _ = pick_damage(oracle, chunk)
    for kind, bad in found:
        for row_bytes in (1, 17, 96, 4080, 20400):
            chunks = [bad, chunk]
            rows_plain = plaintext(oracle, [chunk, chunk])
            codes, code = damaged_rows(oracle, chunks, row_bytes, 0, bad, 2)
            sets = index_sets(chunks, row_bytes)
            index = np.concatenate([sets["in order"], sets["edges"]])
            want = check_take(pkg, lib, mem, TakeSource(mem, chunks=chunks), chunks, rows_plain, row_bytes, index, 1, True, codes, what=(cname, kind))
            nbad = int((want == code).sum())
            assert nbad >= max(8177 // row_bytes, 1) and int((want > 0).sum()) == index.size - nbad, (cname, kind, row_bytes, nbad)
            check_take(pkg, lib, mem, TakeSource(mem, chunks=chunks), chunks, rows_plain, row_bytes, index, 0, False, codes, what=(cname, kind))


@pytest.fixture(scope="module")
def many(pkg, mem, oracle, ref):
    """nchunks -> (the chunks of take_checks.many_chunks, their plaintext, the batch source, the packed one), made once"""
    made, batches = {}, {}
    write = writer(pkg, mem, oracle, ref, "lz4", 4, 1, 0)

    def get(nchunks):
        if nchunks not in batches:
            chunks = many_chunks(oracle, write, 48, nchunks, made)
            batches[nchunks] = (chunks, plaintext(oracle, chunks), TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks)))
        return batches[nchunks]
    return get


@pytest.mark.parametrize("row_bytes", [4, 12, 48])
@pytest.mark.parametrize("nchunks", MANY_COUNTS)
def test_more_chunks_than_the_lds_table_holds(pkg, lib, mem, many, nchunks, row_bytes):
    """1024 chunks bisect k_take.hip's LDS copy of row_first, 1025 and 1300 the table in global memory: every index set - the first and last row
    of every chunk among them - from both sources, with and without a status table, dest at offsets 0 and 5, and once under a pass bound of
    16 KiB.  Rows of 4 bytes move at their natural width, 12 by bytes in one lane, 48 in several lanes"""
    chunks, rows_plain, batch, packed = many(nchunks)
    if nchunks == 1025:
        assert all(np.array_equal(a, b) for a, b in zip(chunks[:1024], many(1024)[0])), "the batch of 1025 is the batch of 1024 and one chunk"
    sets = index_sets(chunks, row_bytes)
    assert sets["edges"].size >= 2 * sum(1 for r in chunk_rows(chunks, row_bytes) if r)
    for name, index in sets.items():
        for src in (batch, packed):
            check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 0, True, what=(nchunks, name, src.packed))
            check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 5, False, what=(nchunks, name, src.packed))
    mixed = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"]])
    check_take(pkg, lib, mem, batch, chunks, rows_plain, row_bytes, mixed, 5, True, what=(nchunks, "mixed"))
    check_take(pkg, lib, mem, packed, chunks, rows_plain, row_bytes, mixed, 0, False, what=(nchunks, "mixed"))
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        check_take(pkg, lib, mem, batch, chunks, rows_plain, row_bytes, mixed, 0, True, what=(nchunks, "16 KiB passes"))
    finally:
        lib.blosc_amd_getitem_pass_bytes(0)


def test_census_failures(pkg, lib, mem, oracle):
    """a chunk whose nbytes is no multiple of row_bytes, a header with a wrong version byte, a packed slot eight bytes short: -1, the code at
    its place in chunk_rows_out, dest and status untouched"""
    good = orc_compress(oracle, plain(N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    odd = orc_compress(oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    check_census_failure(pkg, lib, mem, TakeSource(mem, chunks=[good, odd, good]), 16, [rows, -1, rows], "no multiple")
    check_census_failure(pkg, lib, mem, TakeSource(mem, chunks=[good, good, version]), 16, [rows, rows, -9], "version")
    check_census_failure(pkg, lib, mem, TakeSource(mem, *(None,) + pack_container([version, odd])), 16, [-9, -1], "both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_census_failure(pkg, lib, mem, TakeSource(mem, container=np.concatenate(parts), offsets=offs), 16, [rows, -1, rows], "a slot eight bytes short")
    take = pkg.RowTake(16, lib=lib)
    assert TakeSource(mem, chunks=[good, good]).call(take, None, 0, None, None) == 0 and take.chunk_rows() == [rows, rows] and take.failed() == 0


def test_one_pipeline_per_call(pkg, lib, mem, oracle):
    """100 000 random indices over 8 LZ4 chunks: one launch each of k_take_mark, k_decode_streams and k_take_gather, whatever the number of rows"""
    chunks = [orc_compress(oracle, plain(8 * N, seed=20 + k), 8, 5, 1, "lz4", blocksize=BLOCKSIZE)[1] for k in range(8)]
    rows_plain = plaintext(oracle, chunks)
    row_bytes = 8
    index = np.random.default_rng(9).integers(0, rows_plain.size // row_bytes, 100000).astype(np.int64)
    src = TakeSource(mem, chunks=chunks)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        check_take(pkg, lib, mem, src, chunks, rows_plain, row_bytes, index, 0, True, what="one pipeline")
        launches = {k: pkg.profile_get(k)[1] for k in ("k_take_mark", "k_decode_streams", "k_take_gather", "k_getitem_gather")}
        assert launches == {"k_take_mark": 1, "k_decode_streams": 1, "k_take_gather": 1, "k_getitem_gather": 0}, launches
    finally:
        lib.blosc_gpu_profile(0)


def test_tensors_take_rows(pkg, lib):
    import torch
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_take", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    tensors = importlib.util.module_from_spec(spec); spec.loader.exec_module(tensors)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(5)
    table = torch.cumsum(torch.randn(6000 * 17, device=dev, generator=g) * 1e-3, 0).reshape(6000, 17)
    steps = torch.arange(4096, dtype=torch.int64, device=dev) * 7 - 1000
    for t, per_chunk, nchunks in ((table, 1000, 6), (steps, None, 1)):
        cont, off, meta = tensors.pack_rows(lib, t, rows_per_chunk=per_chunk, cname=b"lz4", shuffle=1)
        assert len(meta) == nchunks and len(off) == nchunks + 1 and [m[1][0] for m in meta] == [t.shape[0] // nchunks] * nchunks
        index = torch.randint(0, t.shape[0], (5000,), dtype=torch.int64, device=dev, generator=g)
        got = tensors.take_rows(lib, cont, off, meta, index)
        assert got.dtype == t.dtype and tuple(got.shape) == (5000,) + tuple(t.shape[1:])
        assert torch.equal(got, t.index_select(0, index))
        assert tuple(tensors.take_rows(lib, cont, off, meta, index[:0]).shape) == (0,) + tuple(t.shape[1:])
        index[17] = t.shape[0]
        with pytest.raises(RuntimeError, match="1 of 5000 rows failed"):
            tensors.take_rows(lib, cont, off, meta, index)
