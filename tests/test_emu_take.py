"""CPU: blosc_gpu_take_batch / blosc_gpu_take_packed (include/blosc_gpu_take.h) on the emulated library - the host engine's census, chunk
table, runs from the touched-block flags and passes, k_take_mark and k_take_gather in every lane mapping.  The checks are those of
tests/test_gpu_take.py (tests/take_checks.py), the grid thinned to what the emulator runs in about a minute."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import NumpyMem, pick_damage, plain
from helpers import header, orc_compress, ptr, ref_compress
from take_checks import (BLOCKSIZE, N, TakeSource, batch_chunks, check_census_failure, check_take, chunk_rows, damaged_rows, index_sets,
                         many_chunks, offsets_for, pack_container, plaintext)
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_SIZES = [1, 8, 12, 17, 96, 4080, 20400]
# (codec, typesize, filter, the factor on N): typesize 17 with each filter, the split typesizes shuffled at 8 N
SETTINGS = [("lz4", 17, 0, 1), ("blosclz", 17, 1, 1), ("lz4", 17, 2, 1), ("blosclz", 4, 1, 8), ("lz4", 8, 1, 8)]


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_take", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def elib(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_take_batch"), "the library has no take calls"
    pkgmod.declare_take(emulib)
    pkgmod.declare_packed(emulib)
    return emulib


def lib_compress(L, data, T, shuffle, cname, blocksize):
    out = np.zeros(data.size + 16, np.uint8)
    r = L.blosc_compress_ctx(5, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname.encode(), blocksize, 1)
    assert r > 0
    return out[:r].copy()


def writer(elib, oracle, ref, cname, T, shuffle, turn):
    """chunk k by the oracle, by the reference where it is built, by the emulated library, in turns"""
    def write(k, data):
        who = (k + turn) % 3
        if who == 1 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
        if who == 2: return lib_compress(elib, data, T, shuffle, cname, BLOCKSIZE)
        return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
    return write


def batch(elib, oracle, ref, setting, row_bytes, turn=0):
    cname, T, shuffle, scale = setting
    chunks = batch_chunks(oracle, writer(elib, oracle, ref, cname, T, shuffle, turn), row_bytes, scale)
    assert -(-header(chunks[0])["nbytes"] // header(chunks[0])["blocksize"]) == 5 and not header(chunks[0])["flags"] & 2
    return chunks, plaintext(oracle, chunks)


@pytest.mark.parametrize("row_bytes", ROW_SIZES)
def test_rows_of_every_index_set(elib, pkgmod, oracle, ref, row_bytes):
    """typesize 17, LZ4 shuffled: every index set with and without a status table, dest at its offsets from a 16-byte boundary"""
    mem = NumpyMem()
    chunks, rows_plain = batch(elib, oracle, ref, ("lz4", 17, 1, 1), row_bytes, turn=row_bytes)
    src = TakeSource(mem, chunks=chunks)
    sets = index_sets(chunks, row_bytes)
    if row_bytes == 1:
        sets["in order"], sets["reversed"] = sets["in order"][::7], sets["reversed"][::5]      # (one fiber per row: the emulator's minute)
    for name, index in sets.items():
        for with_status in (True, False):
            check_take(pkgmod, elib, mem, src, chunks, rows_plain, row_bytes, index, 0, with_status, what=name)
    for offset in offsets_for(row_bytes):
        check_take(pkgmod, elib, mem, src, chunks, rows_plain, row_bytes, np.concatenate([sets["edges"], sets["out of bounds"]]), offset, offset % 2 == 0, what="edges")


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}-T{s[1]}-filter{s[2]}")
def test_settings_and_both_entry_points(elib, pkgmod, oracle, ref, setting):
    """every codec and filter setting through blosc_gpu_take_batch, and out of a container that PackedBatch.compress wrote"""
    mem = NumpyMem()
    cname, T, shuffle, scale = setting
    for row_bytes in (12, 4080) if scale == 1 else ((8,) if T == 4 else (20400,)):      # (the emulator compresses 8 N in ten seconds)
        chunks, rows_plain = batch(elib, oracle, ref, setting, row_bytes, turn=T)
        sets = index_sets(chunks, row_bytes)
        index = np.concatenate([sets["random"][:600], sets["edges"], sets["out of bounds"]])
        check_take(pkgmod, elib, mem, TakeSource(mem, chunks=chunks), chunks, rows_plain, row_bytes, index, 5, True, what=("batch", setting))
        # the packed form: the library writes the container, with align 256
        hosts = [plain(N * scale), plain(0), plain(N * scale // 2, seed=12)] if (N * scale // 2) % row_bytes == 0 else [plain(N * scale), plain(0)]
        pb = pkgmod.PackedBatch(len(hosts), lib=elib)
        cap = pb.bound([h.size for h in hosts], 256)
        cont = np.zeros(cap, np.uint8)
        assert pb.compress([h.ctypes.data if h.size else None for h in hosts], [h.size for h in hosts], cont.ctypes.data, cap, T, 5, shuffle, cname.encode(), BLOCKSIZE, 256) == 0
        off, cb = pb.offsets(), pb.results()
        assert all(c > 0 for c in cb) and all(o % 256 == 0 for o in off)
        written = [cont[off[i]:off[i] + cb[i]].copy() for i in range(len(hosts))]
        packed_plain = plaintext(oracle, written)
        assert np.array_equal(packed_plain, np.concatenate(hosts))
        sets = index_sets(written, row_bytes)
        index = np.concatenate([sets["random"][:600], sets["edges"], sets["out of bounds"]])
        for with_status in (True, False):
            check_take(pkgmod, elib, mem, TakeSource(mem, container=cont, offsets=off), written, packed_plain, row_bytes, index, 0, with_status, what=("packed", setting))


def test_passes_depend_on_bytes_and_give_the_same(elib, pkgmod, oracle, ref):
    """a pass bound of 16 KiB: every chunk of more than two touched blocks is a pass of its own, and the answers are those of one pass"""
    mem = NumpyMem()
    elib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        for row_bytes in (17, 4080):
            chunks, rows_plain = batch(elib, oracle, ref, ("blosclz", 17, 2, 1), row_bytes, turn=1)
            sets = index_sets(chunks, row_bytes)
            index = np.concatenate([sets["out of bounds"], sets["random"][:800], sets["edges"]])
            for src in (TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks))):
                check_take(pkgmod, elib, mem, src, chunks, rows_plain, row_bytes, index, 3, True, what="16 KiB passes")
                check_take(pkgmod, elib, mem, src, chunks, rows_plain, row_bytes, index, 0, False, what="16 KiB passes")
    finally:
        elib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_a_damaged_block_fails_the_rows_that_touch_it(elib, pkgmod, oracle, cname):
    """a chunk with block 2 damaged next to its intact copy in one call: the rows of the block and the rows crossing into it answer the oracle's
    code and are unwritten, all other rows of both chunks are served"""
    mem = NumpyMem()
    chunk = orc_compress(oracle, plain(N), 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
    found, _ = pick_damage(oracle, chunk)
    for kind, bad in found:
        for row_bytes in (17, 96, 4080):
            chunks = [bad, chunk]
            rows_plain = plaintext(oracle, [chunk, chunk])
            codes, code = damaged_rows(oracle, chunks, row_bytes, 0, bad, 2)
            sets = index_sets(chunks, row_bytes)
            index = np.concatenate([sets["in order"][::max(17 // row_bytes, 1) if row_bytes < 96 else 1], sets["edges"]])
            want = check_take(pkgmod, elib, mem, TakeSource(mem, chunks=chunks), chunks, rows_plain, row_bytes, index, 1, True, codes, what=(cname, kind))
            nbad = int((want == code).sum())
            assert nbad >= 8177 // row_bytes and int((want > 0).sum()) == index.size - nbad, (cname, kind, row_bytes, nbad)
            check_take(pkgmod, elib, mem, TakeSource(mem, chunks=chunks), chunks, rows_plain, row_bytes, index, 0, False, codes, what=(cname, kind))


def test_more_chunks_than_the_lds_table_holds(elib, pkgmod, oracle, ref):
    """take_checks.many_chunks: 1024 chunks out of a container (row_first bisected in LDS), then the same and one more as src[] (bisected in
    global memory): the first and last row of every chunk, block edges, random rows and out-of-bounds values, in rows of 12 bytes (the
    device: 1300 chunks too, rows of 4 and 48 bytes, every index set, both sources each)"""
    mem = NumpyMem()
    made = {}
    write = writer(elib, oracle, ref, "lz4", 4, 1, 0)
    for nchunks in (1024, 1025):
        chunks = many_chunks(oracle, write, 48, nchunks, made)
        rows_plain = plaintext(oracle, chunks)
        src = TakeSource(mem, chunks=chunks) if nchunks == 1025 else TakeSource(mem, *(None,) + pack_container(chunks))
        sets = index_sets(chunks, 12)
        index = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"][:600]])
        check_take(pkgmod, elib, mem, src, chunks, rows_plain, 12, index, 5, nchunks == 1025, what=("many chunks", nchunks))


def test_census_failures(elib, pkgmod, oracle):
    """a chunk whose nbytes is no multiple of row_bytes, a header with a wrong version byte, a packed slot eight bytes short: -1, the code at
    its place in chunk_rows_out, dest and status untouched"""
    mem = NumpyMem()
    good = orc_compress(oracle, plain(N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    odd = orc_compress(oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, chunks=[good, odd, good]), 16, [rows, -1, rows], "no multiple")
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, chunks=[good, good, version]), 16, [rows, rows, -9], "version")
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, *(None,) + pack_container([version, odd])), 16, [-9, -1], "both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, container=np.concatenate(parts), offsets=offs), 16, [rows, -1, rows], "a slot eight bytes short")
    # ... and the census of usable chunks alone
    take = pkgmod.RowTake(16, lib=elib)
    src = TakeSource(mem, chunks=[good, good])
    assert src.call(take, None, 0, None, None) == 0 and take.chunk_rows() == [rows, rows] and take.failed() == 0
