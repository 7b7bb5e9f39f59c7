"""blosc_gpu_put_batch / blosc_gpu_put_packed on the device (include/blosc_gpu_put.h): rows written into compressed chunks by an index table in
device memory.  The checks and cases are tests/put_checks.py's: the expected plaintext is the oracle's, updated by numpy in index order, and
every chunk of the new container is read back by the oracle."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import TorchMem, pick_damage, plain
from helpers import header, orc_compress, ref_compress
from put_checks import ALIGNS, check_census_failure, check_put, put_index_sets
from take_checks import BLOCKSIZE, MANY_COUNTS, N, ROW_SIZES, TakeSource, batch_chunks, chunk_rows, many_chunks, offsets_for, pack_container

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODECS = ["lz4", "blosclz", "zstd", "zlib"]
GRID = [(cname, T, shuffle) for T in (1, 4, 8, 17) for shuffle in (0, 1, 2) for cname in CODECS]      # test_gpu_take.py's 48 settings
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
    return chunks


def table(pkg, chunks, setting):
    cname, T, shuffle = setting
    return [pkg.cparams(T, 5, shuffle, cname.encode(), BLOCKSIZE) for _ in chunks]


@pytest.mark.parametrize("row_bytes", ROW_SIZES)
def test_rows_of_every_index_set(pkg, lib, mem, oracle, ref, row_bytes):
    """every index set with and without a status table, `rows` at its offsets from a 16-byte boundary, the three alignments, both entry points"""
    at = ROW_SIZES.index(row_bytes)
    settings = GRID[(5 * at) % STRIDE::STRIDE]
    assert len(settings) >= 4
    for n, setting in enumerate(settings):
        chunks = batch(pkg, mem, oracle, ref, setting, row_bytes, turn=at + n)
        params = table(pkg, chunks, setting)
        src = TakeSource(mem, chunks=chunks) if n % 2 == 0 else TakeSource(mem, *(None,) + pack_container(chunks))
        sets = put_index_sets(chunks, row_bytes)
        for m, (name, index) in enumerate(sets.items()):
            _, put, _ = check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, index, params, ALIGNS[(m + n) % 3], 0, (m + n) % 2 == 0, what=(setting, name))
            if name == "one chunk only":
                assert put.rewritten().count(1) == 1 and put.rewritten().count(0) == len(chunks) - 1
            if name == "none":
                assert put.rewritten() == [0] * len(chunks) and put.failed() == 0
        edges =np.concatenate([sets["edges"], sets["out of bounds"], sets["random"][:500], sets["edges"][::-1]])
        for offset in offsets_for(row_bytes):
            check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, edges, params, ALIGNS[offset % 3], offset, offset % 2 == 1, what=(setting, "edges"))


def test_passes_depend_on_bytes_and_give_the_same(pkg, lib, mem, oracle, ref):
    """a pass bound of 16 KiB: every touched chunk is a pass of its own - k_put_scatter and k_put_assemble once per pass, the mark kernel once -
    and the container is, byte for byte, that of one pass"""
    lib.blosc_gpu_profile(1)
    try:
        for row_bytes, setting in ((17, ("blosclz", 17, 2)), (4080, ("zstd", 17, 1)), (96, ("lz4", 8, 1))):
            chunks = batch(pkg, mem, oracle, ref, setting, row_bytes, turn=1)
            params = table(pkg, chunks, setting)
            sets = put_index_sets(chunks, row_bytes)
            index = np.concatenate([sets["out of bounds"], sets["random"], sets["edges"]])
            touched = sum(1 for c in chunks if header(c)["nbytes"])      # (the random rows reach every chunk that has rows)
            for src in (TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks))):
                one, put1, _ = check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, index, params, 256, 3, True, what=("one pass", setting))
                assert put1.rewritten().count(1) == touched
                lib.blosc_amd_getitem_pass_bytes(16 << 10)
                try:
                    lib.blosc_gpu_profile_reset()
                    many, put2, _ = check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, index, params, 256, 3, True, what=("16 KiB passes", setting))
                    launches = {k: pkg.profile_get(k)[1] for k in ("k_take_mark", "k_put_claim", "k_put_scatter", "k_put_assemble")}
                finally:
                    lib.blosc_amd_getitem_pass_bytes(0)
                assert launches == {"k_take_mark": 1, "k_put_claim": touched, "k_put_scatter": touched, "k_put_assemble": touched}, launches
                assert put1.offsets() == put2.offsets() and put1.results() == put2.results()
                if setting[0] != "zlib":
                    assert np.array_equal(one, many), (setting, "the passes changed the container")
    finally:
        lib.blosc_gpu_profile(0)


@pytest.mark.parametrize("cname", CODECS)
def test_a_damaged_chunk_is_carried_over(pkg, lib, mem, oracle, ref, cname):
    """a chunk with a damaged block next to its intact copy: the damaged one comes through byte for byte with rewritten_out -1 and its indices
    answer -1, the intact one takes its rows"""
    data = plain(N)
    if cname in ("lz4", "blosclz"): chunk = orc_compress(oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
    elif ref is not None: chunk = ref_compress(ref, data, 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
    else: chunk = lib_chunk(pkg, mem, data, 17, 1, cname, BLOCKSIZE)
    found, _ = pick_damage(oracle, chunk)
    for kind, bad in found:
        for row_bytes in (1, 17, 96, 4080, 20400):
            chunks = [bad, chunk]
            params = table(pkg, chunks, (cname, 17, 1))
            sets = put_index_sets(chunks, row_bytes)
            index = np.concatenate([sets["in order"], sets["edges"]])
            _, put, _ = check_put(pkg, lib, mem, oracle, TakeSource(mem, chunks=chunks), chunks, row_bytes, index, params, 16, 1, True, what=(cname, kind))
            assert put.rewritten() == [-1, 1] and put.failed() >= N // row_bytes


@pytest.fixture(scope="module")
def many(pkg, mem, oracle, ref):
    """nchunks -> (the chunks of take_checks.many_chunks, the batch source, the packed one), made once"""
    made, batches = {}, {}
    write = writer(pkg, mem, oracle, ref, "lz4", 4, 1, 0)

    def get(nchunks):
        if nchunks not in batches:
            chunks = many_chunks(oracle, write, 48, nchunks, made)
            batches[nchunks] = (chunks, TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks)))
        return batches[nchunks]
    return get


@pytest.mark.parametrize("row_bytes", [4, 12, 48])
@pytest.mark.parametrize("nchunks", MANY_COUNTS)
def test_more_chunks_than_the_lds_table_holds(pkg, lib, mem, oracle, many, nchunks, row_bytes):
    """1024 chunks bisect the LDS copy of row_first in k_put_claim and k_put_scatter, 1025 and 1300 the table in global memory: every index set
    from both sources at aligns 1 and 256, with and without a status table, `rows` at offsets 0 and 5, and once under a pass bound of 16 KiB;
    rewritten_out is the expectation for every chunk and the oracle reads every rewritten one (check_put)"""
    chunks, batch, packed = many(nchunks)
    params = [pkg.cparams(4, 5, 1, b"lz4", BLOCKSIZE) for _ in chunks]
    sets = put_index_sets(chunks, row_bytes)
    holding = sum(1 for r in chunk_rows(chunks, row_bytes) if r)
    for m, (name, index) in enumerate(sets.items()):
        src, align, offset = (batch, packed)[m % 2], (1, 256)[(m // 2) % 2], (0, 5)[(m // 4) % 2]
        _, put, _ = check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, index, params, align, offset, m % 3 != 2, what=(nchunks, name))
        if name in ("in order", "edges"):
            assert put.rewritten().count(1) == holding and put.rewritten().count(0) == nchunks - holding
    mixed = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"], sets["edges"][::-1]])
    check_put(pkg, lib, mem, oracle, packed, chunks, row_bytes, mixed, params, 1, 5, True, what=(nchunks, "mixed, packed"))
    one, put1, _ = check_put(pkg, lib, mem, oracle, batch, chunks, row_bytes, mixed, params, 256, 0, False, what=(nchunks, "mixed"))
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        many_passes, put2, _ = check_put(pkg, lib, mem, oracle, batch, chunks, row_bytes, mixed, params, 256, 0, False, what=(nchunks, "16 KiB passes"))
    finally:
        lib.blosc_amd_getitem_pass_bytes(0)
    assert put1.offsets() == put2.offsets() and put1.results() == put2.results() and np.array_equal(one, many_passes), "the passes changed the container"


def test_carried_over_chunks_around_the_tile_ends_of_assemble(pkg, lib, mem, oracle):
    """MEMCPYED chunks of 16 383, 16 384, 16 385, 32 768 and 32 769 bytes that no index touches, between chunks that are rewritten, at align 1:
    the 16 KiB tiles of k_put_assemble end in front of, at and behind a chunk's end, and its head / body / tail split meets every size"""
    rng = np.random.default_rng(77)
    sizes = (16383, 16384, 16385, 32768, 32769)
    carried = [orc_compress(oracle, rng.integers(0, 256, c - 16, dtype=np.uint8), 1, 5, 0, "lz4")[1] for c in sizes]
    assert [(header(c)["cbytes"], header(c)["flags"] & 2) for c in carried] == [(c, 2) for c in sizes]
    small = [orc_compress(oracle, plain(n, seed=60 + n), 1, 5, 0, "lz4", blocksize=512)[1] for n in (1001, 3, 2048)]
    chunks = [small[0], carried[0], carried[1], small[1], carried[2], carried[3], small[2], carried[4]]
    rows = chunk_rows(chunks, 1)
    first = np.concatenate([[0], np.cumsum(rows)])
    index = np.concatenate([np.arange(first[k], first[k + 1])[::3] for k in (0, 3, 6)]).astype(np.int64)
    params = [pkg.cparams(1, 5, 0, b"lz4", 512) for _ in chunks]
    for src in (TakeSource(mem, chunks=chunks), TakeSource(mem, *(None,) + pack_container(chunks, align=1))):
        _, put, _ = check_put(pkg, lib, mem, oracle, src, chunks, 1, index, params, 1, 0, True, what="tile ends")
        assert put.rewritten() == [1, 0, 0, 1, 0, 0, 1, 0] and put.results()[1:3] + put.results()[4:6] + put.results()[7:] == list(sizes)


def test_census_failures(pkg, lib, mem, oracle):
    """take's three census failures, a clevel of 10, a Snappy compcode, a dest that overlaps the source: a negative answer, the code at its place
    in chunk_rows_out, nothing else written"""
    setting = ("lz4", 17, 1)
    good = orc_compress(oracle, plain(N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    odd = orc_compress(oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    ok = lambda chunks: table(pkg, chunks, setting)
    for chunks, want, what in (([good, odd, good], [rows, -1, rows], "no multiple"), ([good, good, version], [rows, rows, -9], "version")):
        check_census_failure(pkg, lib, mem, TakeSource(mem, chunks=chunks), chunks, 16, ok(chunks), want, what=what)
    chunks = [version, odd]
    check_census_failure(pkg, lib, mem, TakeSource(mem, *(None,) + pack_container(chunks)), chunks, 16, ok(chunks), [-9, -1], what="both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_census_failure(pkg, lib, mem, TakeSource(mem, container=np.concatenate(parts), offsets=offs), [good] * 3, 16, ok([good] * 3), [rows, -1, rows],
                         what="a slot eight bytes short")
    chunks = [good, good, good]
    for k, row, code in ((2, pkg.cparams(17, 10, 1, b"lz4"), -10), (0, pkg.cparams(17, 5, 1, b"snappy"), -5)):
        params = ok(chunks); params[k] = row
        want = [rows] * 3; want[k] = code
        check_census_failure(pkg, lib, mem, TakeSource(mem, chunks=chunks), chunks, 16, params, want, what=("params", k, code))
    # dest inside the source container, and on top of one src[i] chunk: the source stays what it was
    cont, off = pack_container(chunks)
    room, base = mem.put(np.concatenate([cont, np.full(3 * (N + 16) + 64, 0xA5, np.uint8)]))
    idx, new = mem.put(np.array([0, 1, 2], np.int64).view(np.uint8)), mem.put(np.zeros(48, np.uint8))
    for packed in (True, False):
        put = pkg.RowPut(16, lib=lib)
        dest = base + (cont.size - 8 if packed else off[2] + 20)
        if packed: rc = put.packed(base, cont.size, off, idx[1], 3, new[1], ok(chunks), dest, 3 * (N + 16), 1, None)
        else: rc = put.batch([base + o for o in off[:3]], idx[1], 3, new[1], ok(chunks), dest, 3 * (N + 16), 1, None)
        after = mem.get(room)
        assert rc < 0 and np.array_equal(after[:cont.size], cont) and np.all(after[cont.size:] == 0xA5) and put.offsets() == [0] * 4, ("overlap", packed, rc)


def test_one_pipeline_per_call(pkg, lib, mem, oracle):
    """100 000 random indices over 8 LZ4 chunks: one launch each of the mark kernel, k_decode_streams, k_put_claim, k_put_scatter, k_encode_streams
    and k_put_assemble, whatever the number of rows"""
    setting = ("lz4", 8, 1)
    chunks = [orc_compress(oracle, plain(8 * N, seed=20 + k), 8, 5, 1, "lz4", blocksize=BLOCKSIZE)[1] for k in range(8)]
    params = table(pkg, chunks, setting)
    row_bytes = 8
    index = np.random.default_rng(9).integers(0, 8 * 8 * N // row_bytes, 100000).astype(np.int64)
    src = TakeSource(mem, chunks=chunks)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        _, put, _ = check_put(pkg, lib, mem, oracle, src, chunks, row_bytes, index, params, 256, 0, True, what="one pipeline")
        names = ("k_take_mark", "k_decode_streams", "k_put_claim", "k_put_scatter", "k_encode_streams", "k_put_assemble", "k_take_gather")
        launches = {k: pkg.profile_get(k)[1] for k in names}
        assert launches == dict(zip(names, (1, 1, 1, 1, 1, 1, 0))), launches
        assert put.rewritten() == [1] * 8
    finally:
        lib.blosc_gpu_profile(0)


def test_tensors_put_rows(pkg, lib):
    """tensors.put_rows against Tensor.index_copy_ with distinct indices and against a sequential loop with repeated ones, read back through both
    take_rows and unpack_tensors"""
    import torch
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_put", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    tensors = importlib.util.module_from_spec(spec); spec.loader.exec_module(tensors)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(5)
    table_ = torch.cumsum(torch.randn(6000 * 17, device=dev, generator=g) * 1e-3, 0).reshape(6000, 17)
    steps = torch.arange(4096, dtype=torch.int64, device=dev) * 7 - 1000
    for t, per_chunk, nchunks in ((table_, 1000, 6), (steps, None, 1)):
        cont, off, meta = tensors.pack_rows(lib, t, rows_per_chunk=per_chunk, cname=b"lz4", shuffle=1)
        before = cont.clone()
        everything = torch.arange(t.shape[0], dtype=torch.int64, device=dev)
        # distinct indices: index_copy_
        index = torch.randperm(t.shape[0], device=dev, generator=g)[:700]
        new = (torch.randn((700,) + tuple(t.shape[1:]), device=dev, generator=g) * 100).to(t.dtype)
        want = t.clone().index_copy_(0, index, new)
        cont2, off2 = tensors.put_rows(lib, cont, off, meta, index, new, cname=b"lz4", shuffle=1)
        assert len(off2) == nchunks + 1 and int(cont2.numel()) == off2[-1] and torch.equal(cont, before)
        assert torch.equal(tensors.take_rows(lib, cont2, off2, meta, everything), want)
        assert torch.equal(torch.cat(tensors.unpack_tensors(lib, cont2, off2, meta)), want)
        # repeated indices: a sequential loop, the last occurrence wins
        index = torch.randint(0, 50, (300,), dtype=torch.int64, device=dev, generator=g) * (t.shape[0] // 50)
        new = (torch.randn((300,) + tuple(t.shape[1:]), device=dev, generator=g) * 100).to(t.dtype)
        want = t.clone()
        for k, r in enumerate(index.tolist()):
            want[r] = new[k]
        cont3, off3 = tensors.put_rows(lib, cont, off, meta, index, new, cname=b"lz4", shuffle=1)
        assert torch.equal(tensors.take_rows(lib, cont3, off3, meta, everything), want)
        assert torch.equal(torch.cat(tensors.unpack_tensors(lib, cont3, off3, meta)), want)
        # no index: the same table in a container of its own; an index outside the table raises
        cont4, off4 = tensors.put_rows(lib, cont, off, meta, index[:0], new[:0])
        assert off4 == list(off) and torch.equal(cont4, cont[:off4[-1]])
        index[17] = t.shape[0]
        with pytest.raises(RuntimeError, match="1 of 300 rows failed"):
            tensors.put_rows(lib, cont, off, meta, index, new)
