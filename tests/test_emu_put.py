"""CPU: blosc_gpu_put_batch / blosc_gpu_put_packed (include/blosc_gpu_put.h) on the emulated library - the host engine's census, the touched-chunk
flags, the passes, the decode and the encode in one context, k_put_claim, k_put_scatter in every lane mapping and k_put_assemble.  The checks
are those of tests/test_gpu_put.py (tests/put_checks.py), the grid thinned to what the emulator runs in about a minute."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import NumpyMem, pick_damage, plain
from helpers import header, orc_compress, ptr, ref_compress
from put_checks import ALIGNS, SENTINEL, bound, check_census_failure, check_put, expected, new_rows, put_index_sets, run_put
from take_checks import BLOCKSIZE, N, TakeSource, batch_chunks, chunk_rows, many_chunks, offsets_for, pack_container
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_SIZES = [1, 8, 12, 17, 96, 4080, 20400]
# (codec, typesize, filter, the factor on N): test_emu_take.py's
SETTINGS = [("lz4", 17, 0, 1), ("blosclz", 17, 1, 1), ("lz4", 17, 2, 1), ("blosclz", 4, 1, 8), ("lz4", 8, 1, 8)]


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_put", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def elib(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_put_batch"), "the library has no put calls"
    pkgmod.declare_put(emulib)
    pkgmod.declare_params(emulib)
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
    return chunks


def table(pkgmod, chunks, setting):
    cname, T, shuffle, _ = setting
    return [pkgmod.cparams(T, 5, shuffle, cname.encode(), BLOCKSIZE) for _ in chunks]


@pytest.mark.parametrize("row_bytes", ROW_SIZES)
def test_rows_of_every_index_set(elib, pkgmod, oracle, ref, row_bytes):
    """typesize 17, LZ4 shuffled: the index sets, `rows` at its offsets from a 16-byte boundary, the three alignments of the container"""
    mem = NumpyMem()
    setting = ("lz4", 17, 1, 1)
    chunks = batch(elib, oracle, ref, setting, row_bytes, turn=row_bytes)
    params = table(pkgmod, chunks, setting)
    src = TakeSource(mem, chunks=chunks)
    sets = put_index_sets(chunks, row_bytes)
    if row_bytes == 1:
        sets["in order"], sets["reversed"] = sets["in order"][::7], sets["reversed"][::5]      # (one fiber per index: the emulator's minute)
    named = ("one row a thousand times", "one chunk only", "none", "out of bounds") + (("reversed",) if row_bytes in (8, 96, 20400) else ())
    for n, name in enumerate(named):
        _, put, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, sets[name], params, ALIGNS[n % 3], 0, n % 2 == 0, what=name)
        if name == "one chunk only":
            assert put.rewritten().count(1) == 1 and put.rewritten().count(0) == len(chunks) - 1
        if name == "none":
            assert put.rewritten() == [0] * len(chunks) and put.failed() == 0
    mixed = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"][:300], sets["edges"][::-1]])
    check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, mixed, params, 256, 5, True, what="mixed")
    # `rows` at its offsets from a 16-byte boundary: the rows of the last chunk alone (the emulator encodes 100 KB in a second)
    bad = np.array([-1, sum(chunk_rows(chunks, row_bytes)), 2 ** 40, -2 ** 63, 2 ** 63 - 1], np.int64)
    few = np.concatenate([sets["one chunk only"], bad, sets["one chunk only"][:50]])
    for offset in offsets_for(row_bytes):
        check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, few, params, ALIGNS[offset % 3], offset, offset % 2 == 1, what="offsets")


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: f"{s[0]}-T{s[1]}-filter{s[2]}")
def test_settings_and_both_entry_points(elib, pkgmod, oracle, ref, setting):
    """every codec and filter setting through blosc_gpu_put_batch and blosc_gpu_put_packed; rewritten LZ4 / BloscLZ chunks are, byte for byte, what
    blosc_gpu_compress_batch_params writes for the same plaintext"""
    mem = NumpyMem()
    cname, T, shuffle, scale = setting
    for row_bytes in (12, 4080) if scale == 1 else ((8,) if T == 4 else (20400,)):
        chunks = batch(elib, oracle, ref, setting, row_bytes, turn=T)
        params = table(pkgmod, chunks, setting)
        sets = put_index_sets(chunks, row_bytes)
        index = np.concatenate([sets["random"][:400], sets["edges"], sets["out of bounds"]])
        if scale > 1:      # (8 N: the rows of the last chunk alone)
            index = np.concatenate([sets["one chunk only"], [-1, 2 ** 40], sets["one chunk only"][::-1]]).astype(np.int64)
        sources = [TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks))]
        for src in sources[:2 if scale == 1 else 1] if row_bytes != 4080 else sources[1:]:
            dest, put, want_plain = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, index, params, 16, 5, True, what=(setting, src.packed))
        off, cb = put.offsets(), put.results()
        for i, p in enumerate(want_plain):
            if p is None:
                continue
            out = np.zeros(p.size + 16, np.uint8)
            b = pkgmod.DeviceBatch([p.ctypes.data], [p.size], [out.ctypes.data], [out.size])
            assert b.compress_params([params[i]], lib=elib) == 0 and b.results()[0] == cb[i], (setting, i, b.results(), cb[i])
            assert np.array_equal(out[:cb[i]], dest[off[i]:off[i] + cb[i]]), (setting, "chunk", i, "is not the compress call's")


def test_passes_give_the_same_container(elib, pkgmod, oracle, ref):
    """a pass bound of 16 KiB: every touched chunk is a pass of its own, and the container is, byte for byte, that of one pass"""
    mem = NumpyMem()
    setting = ("blosclz", 17, 2, 1)
    for row_bytes in (17, 4080):
        chunks = batch(elib, oracle, ref, setting, row_bytes, turn=1)
        params = table(pkgmod, chunks, setting)
        sets = put_index_sets(chunks, row_bytes)
        index = np.concatenate([sets["out of bounds"], sets["random"][:500], sets["edges"]])
        src = TakeSource(mem, chunks=chunks) if row_bytes == 17 else TakeSource(mem, *(None,) + pack_container(chunks))
        one, put1, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, index, params, 256, 3, True, what="one pass")
        elib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            many, put2, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, index, params, 256, 3, True, what="16 KiB passes")
        finally:
            elib.blosc_amd_getitem_pass_bytes(0)
        assert put1.offsets() == put2.offsets() and put1.results() == put2.results() and np.array_equal(one, many)


def test_a_damaged_chunk_is_carried_over(elib, pkgmod, oracle):
    """a chunk with a damaged block next to its intact copy: the damaged one comes through byte for byte with rewritten_out -1 and its indices
    answer -1, the intact one takes its rows"""
    mem = NumpyMem()
    setting = ("lz4", 17, 1, 1)
    chunk = orc_compress(oracle, plain(N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    found, _ = pick_damage(oracle, chunk)
    kind, bad = found[0]
    for row_bytes in (17, 4080):
        chunks = [bad, chunk]
        params = table(pkgmod, chunks, setting)
        sets = put_index_sets(chunks, row_bytes)
        index = np.concatenate([sets["random"][:300], sets["edges"], sets["out of bounds"]])
        _, put, _ = check_put(pkgmod, elib, mem, oracle, TakeSource(mem, chunks=chunks), chunks, row_bytes, index, params, 16, 1, True, what=kind)
        assert put.rewritten() == [-1, 1] and put.failed() > 5


def test_more_chunks_than_the_lds_table_holds(elib, pkgmod, oracle, ref):
    """take_checks.many_chunks, 1025 chunks out of a container: k_put_claim and k_put_scatter bisect row_first in global memory.  The first and
    last row of every 13th chunk and of the chunks around the stretches without rows, and out-of-bounds values, in rows of 12 bytes; every
    chunk's rewritten_out, every rewritten chunk read back by the oracle (the emulator encodes 40 KB a second; the device: 1024 and 1300
    chunks too, rows of 4 and 48 bytes, every index set, both sources)"""
    mem = NumpyMem()
    chunks = many_chunks(oracle, writer(elib, oracle, ref, "lz4", 4, 1, 0), 48, 1025)
    params = [pkgmod.cparams(4, 5, 1, b"lz4", BLOCKSIZE) for _ in chunks]
    rows = chunk_rows(chunks, 12)
    first = np.concatenate([[0], np.cumsum(rows)])
    picked = [k for k in sorted(set(range(1, 1025, 13)) | {98, 99, 103, 104, 698, 699, 704, 1019, 1021}) if rows[k]]
    sets = put_index_sets(chunks, 12)
    index = np.concatenate([[int(first[k]), int(first[k + 1]) - 1] for k in picked] + [sets["out of bounds"][1::4]]).astype(np.int64)
    _, put, _ = check_put(pkgmod, elib, mem, oracle, TakeSource(mem, *(None,) + pack_container(chunks)), chunks, 12, index, params, 1, 5, True, what="many chunks")
    assert [k for k, w in enumerate(put.rewritten()) if w] == picked and len(picked) > 60


def test_census_failures(elib, pkgmod, oracle):
    """take's three census failures, a clevel of 10, a Snappy compcode and a dest that overlaps the source: a negative answer, the code at its
    place in chunk_rows_out, nothing else written"""
    mem = NumpyMem()
    setting = ("lz4", 17, 1, 1)
    good = orc_compress(oracle, plain(N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    odd = orc_compress(oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    ok = lambda chunks: table(pkgmod, chunks, setting)
    for chunks, want, what in (([good, odd, good], [rows, -1, rows], "no multiple"), ([good, good, version], [rows, rows, -9], "version")):
        check_census_failure(pkgmod, elib, mem, TakeSource(mem, chunks=chunks), chunks, 16, ok(chunks), want, what=what)
    chunks = [version, odd]
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, *(None,) + pack_container(chunks)), chunks, 16, ok(chunks), [-9, -1], what="both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_census_failure(pkgmod, elib, mem, TakeSource(mem, container=np.concatenate(parts), offsets=offs), [good] * 3, 16, ok([good] * 3), [rows, -1, rows],
                         what="a slot eight bytes short")
    chunks = [good, good, good]
    for k, row, code in ((2, pkgmod.cparams(17, 10, 1, b"lz4"), -10), (0, pkgmod.cparams(17, 5, 1, b"snappy"), -5), (1, pkgmod.cparams(0, 5, 1, b"lz4"), -10)):
        params = ok(chunks); params[k] = row
        want = [rows] * 3; want[k] = code
        check_census_failure(pkgmod, elib, mem, TakeSource(mem, chunks=chunks), chunks, 16, params, want, what=("params", k, code))
    # dest inside the source container, and on top of one src[i] chunk
    cont, off = pack_container(chunks)
    room = np.full(cont.size + bound(chunks, 1) + 64, SENTINEL, np.uint8)
    room[:cont.size] = cont
    idx = np.array([0, 1, 2], np.int64)
    new = new_rows(3, 16)
    for packed in (True, False):
        put = pkgmod.RowPut(16, lib=elib)
        dest = room.ctypes.data + (cont.size - 8 if packed else off[2] + 20)      # (the batch form: inside the last chunk's bytes)
        if packed: rc = put.packed(room.ctypes.data, cont.size, off, idx.ctypes.data, 3, new.ctypes.data, ok(chunks), dest, bound(chunks, 1), 1, None)
        else: rc = put.batch([room.ctypes.data + o for o in off[:3]], idx.ctypes.data, 3, new.ctypes.data, ok(chunks), dest, bound(chunks, 1), 1, None)
        assert rc < 0 and np.array_equal(room[:cont.size], cont) and np.all(room[cont.size:] == SENTINEL) and put.offsets() == [0] * 4, ("overlap", packed, rc)
    # ... and the census of usable chunks alone is the pure copy
    put = pkgmod.RowPut(16, lib=elib)
    out = np.zeros(bound(chunks[:2], 1), np.uint8)
    assert put.batch([ptr(good), ptr(good)], None, 0, None, ok(chunks[:2]), out.ctypes.data, out.size, 1, None) == 0
    assert put.chunk_rows() == [rows, rows] and put.failed() == 0 and put.rewritten() == [0, 0] and np.array_equal(out[:good.size], good)


def test_a_short_dest(elib, pkgmod, oracle, ref):
    """a dest that ends inside the container: cbytes_out 0 behind the cut, offsets_out[nchunks] still the size needed, nothing written behind destsize"""
    mem = NumpyMem()
    setting = ("lz4", 17, 1, 1)
    row_bytes = 96
    chunks = batch(elib, oracle, ref, setting, row_bytes, turn=0)
    params = table(pkgmod, chunks, setting)
    src = TakeSource(mem, chunks=chunks)
    # untouched chunks: every size is known to the test, and the table is checked to its end
    none = np.zeros(0, np.int64)
    full, put, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, none, params, 16, 0, False, what="whole")
    need, off = put.offsets()[-1], put.offsets()
    for cut in (off[2] + 5, off[1] - 1, 0):
        dest, short, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, none, params, 16, 0, False, destsize=cut, what=("cut", cut))
        assert short.offsets() == off and short.offsets()[-1] == need
        assert [c > 0 for c in short.results()] == [off[i] + put.results()[i] <= cut for i in range(len(chunks))]
    # rewritten chunks in front of the cut
    index = put_index_sets(chunks, row_bytes)["random"][:300]
    whole, put, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, index, params, 16, 0, True, what="whole, rewritten")
    off = put.offsets()
    dest, short, _ = check_put(pkgmod, elib, mem, oracle, src, chunks, row_bytes, index, params, 16, 0, True, destsize=off[-2] + 3, what="cut, rewritten")
    assert short.offsets() == off and short.results()[:-1] == put.results()[:-1] and short.results()[-1] == 0
    assert np.array_equal(dest[:off[-2]], whole[:off[-2]])
