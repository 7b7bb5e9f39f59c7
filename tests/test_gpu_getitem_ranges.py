"""blosc_gpu_getitem_batch / blosc_gpu_getitem_packed on the device (include/blosc_gpu_getitem.h): many item ranges of many chunks in one
call; blosc_getitem / blosc_gpu_getitem, one range of one chunk through the same pipeline, with host and device memory on either side.  Expected results and bytes come from the oracle's orc_getitem on the same chunk, range by range (tests/getitem_ranges_checks.py)."""
import numpy as np
import pytest

from getitem_ranges_checks import (BIG, BLOCKSIZE, SENTINEL, SHUFFLES, SMALL, TYPESIZES, NumpyMem, TorchMem, check_batch, check_damage, check_single,
                                   chunk_ranges, damaged_single_chunks, expected, pick_damage, plain, prefix, single_grid_chunks)
from helpers import header, orc_compress, ref_compress

pytestmark = pytest.mark.gpu
CODECS = ["lz4", "blosclz", "zstd", "zlib"]


def lib_chunks(pkg, mem, datas, T, shuffle, cname, blocksize):
    """blosc_gpu_compress_batch of `datas` with one setting"""
    src = [mem.put(d) for d in datas]
    dst = [mem.filled(d.size + 16, 0) for d in datas]
    b = pkg.DeviceBatch([p for _, p in src], [d.size for d in datas], [p for _, p in dst], [d.size + 16 for d in datas])
    assert b.compress(T, 5, shuffle, cname.encode(), blocksize) == 0
    cb = b.results()
    assert all(c > 0 for c in cb), cb
    return [mem.get(h)[:c].copy() for (h, _), c in zip(dst, cb)]


@pytest.fixture(scope="module")
def mem(pkg):
    return TorchMem()


@pytest.fixture(scope="module")
def chunks(pkg, mem, oracle, ref):
    """typesizes 1, 2, 4, 8, 17 x shuffle 0 / 1 / 2 x the four codecs at 40 KiB + 24 bytes with blocksize 8192, written by the oracle (LZ4, BloscLZ),
    by the reference where it is built and by this library; the same at 5 x 64 KiB + 24 for the shuffled settings (a split block is widened to
    64 KiB, so only this size gives the split typesizes several blocks); a MEMCPYED chunk of random bytes, one of 100 bytes, one of nbytes 0"""
    small, big = plain(SMALL), plain(BIG)
    out = []
    for T in TYPESIZES:
        for shuffle in SHUFFLES:
            for cname in CODECS:
                if cname in ("lz4", "blosclz"):
                    out.append(orc_compress(oracle, small, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1])
                if ref is not None:
                    out.append(ref_compress(ref, small, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1])
                datas = [small, big] if shuffle == 1 else [small]
                out += lib_chunks(pkg, mem, datas, T, shuffle, cname, BLOCKSIZE)
                if shuffle == 1 and ref is not None and T in (4, 8):
                    out.append(ref_compress(ref, big, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1])
    rng = np.random.default_rng(3)
    out.append(orc_compress(oracle, rng.integers(0, 256, 9000, dtype=np.uint8), 4, 5, 1, "lz4")[1])
    out.append(orc_compress(oracle, plain(100), 4, 5, 1, "lz4")[1])
    out.append(orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1])
    assert header(out[-3])["flags"] & 2 and header(out[-1])["nbytes"] == 0
    nblocks = [-(-header(c)["nbytes"] // header(c)["blocksize"]) for c in out[:-3]]
    assert sum(n == 6 for n in nblocks) >= 40 and all(c is not None for c in out)
    return out


def all_ranges(chunks):
    return [(ci, s, k) for ci, c in enumerate(chunks) for s, k in chunk_ranges(c)] + [(len(chunks), 0, 1)]


def test_one_batch_over_every_chunk(pkg, lib, mem, oracle, chunks):
    got = check_batch(pkg, lib, mem, oracle, chunks, all_ranges(chunks))
    assert sum(g > 0 for g in got) > 8 * len(chunks) and got[-1] == -1


def test_passes_depend_on_bytes_and_give_the_same(pkg, lib, mem, oracle, chunks):
    """a pass bound of 64 KiB: the call runs as many launches as its decoded bytes ask for - and no more - and answers the same"""
    sub = chunks[::7] + chunks[-3:]
    ranges = all_ranges(sub)[::-1]
    spans = [-(-header(c)["nbytes"] // header(c)["blocksize"]) * header(c)["blocksize"] for c in sub if not header(c)["flags"] & 2 and header(c)["nbytes"]]
    lib.blosc_amd_getitem_pass_bytes(64 << 10)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        check_batch(pkg, lib, mem, oracle, sub, ranges, "64 KiB passes")
        launches = pkg.profile_get("k_getitem_gather")[1]
        assert 2 <= launches <= len(spans), (launches, len(spans))      # by bytes: never more than one per chunk, whatever the ~12 ranges per chunk
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_a_damaged_block_fails_the_ranges_that_touch_it(pkg, lib, mem, oracle, cname):
    for T, shuffle, n in ((17, 1, SMALL), (8, 1, BIG)):
        chunk = orc_compress(oracle, plain(n), T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        found, rngs = pick_damage(oracle, chunk)
        for kind, bad in found:
            ranges = [(0, s, k) for s, k in rngs] + [(1, s, k) for s, k in rngs]      # chunk 1: the intact copy, same blocks in the same call
            got = check_batch(pkg, lib, mem, oracle, [bad, chunk], ranges, (cname, T, kind))
            assert got[0] < 0 and got[1] == 7 * T and got[2] < 0 and got[3:] == [7 * T] * 3, (kind, got)


def test_packed(pkg, lib, mem, oracle):
    rng = np.random.default_rng(4)
    hosts = [plain(SMALL), rng.integers(0, 256, 9000, dtype=np.uint8), plain(100), plain(0), plain(BIG, seed=5)]
    n = len(hosts)
    src = [mem.put(h) for h in hosts]
    for cname, shuffle, T in ((b"lz4", 1, 17), (b"lz4", 1, 8), (b"blosclz", 2, 4), (b"zstd", 1, 4), (b"zlib", 0, 1)):
        pb = pkg.PackedBatch(n)
        cap = pb.bound([h.size for h in hosts], 256)
        cont, cptr = mem.filled(cap, 0)
        assert pb.compress([p for _, p in src], [h.size for h in hosts], cptr, cap, T, 5, shuffle, cname, BLOCKSIZE, 256) == 0
        off, cb = pb.offsets(), pb.results()
        assert all(c > 0 for c in cb) and all(o % 256 == 0 for o in off)
        image = mem.get(cont)
        chunks = [image[off[i]:off[i] + cb[i]].copy() for i in range(n)]
        ranges = [(ci, s, k) for ci, c in enumerate(chunks) for s, k in chunk_ranges(c)] + [(n, 0, 1)]
        want = expected(oracle, chunks, ranges)
        res, offs = [r for r, _ in want], prefix([r for r, _ in want])
        b = pkg.ItemRanges(ranges)
        assert b.packed(cptr, cap, off, None, 0) == 0                                # the size query
        assert b.results() == res and b.offsets() == offs, cname
        total = offs[-1]
        out, optr = mem.filled(total + 64, SENTINEL)
        assert b.packed(cptr, cap, off, optr, total) == 0                            # a dest of exactly that size
        assert b.results() == res and b.offsets() == offs, cname
        exp = np.concatenate([d for r, d in want if r > 0])
        got = mem.get(out)
        assert np.array_equal(got[:total], exp) and np.all(got[total:] == SENTINEL), cname
        last = max(k for k, r in enumerate(res) if r > 0)                            # one byte short
        out, optr = mem.filled(total + 64, SENTINEL)
        assert b.packed(cptr, cap, off, optr, total - 1) == 0
        assert b.results() == res[:last] + [-1] + res[last + 1:], cname
        got = mem.get(out)
        assert np.array_equal(got[:offs[last]], exp[:offs[last]]) and np.all(got[offs[last]:] == SENTINEL), cname
    # an offset table built by hand, the slot of chunk 1 eight bytes short of its cbytes: every range of that chunk answers -1
    chunks = [orc_compress(oracle, plain(SMALL), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1] for _ in range(3)]
    offs, parts = [0], []
    for k, c in enumerate(chunks):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    cont, cptr = mem.put(np.concatenate(parts))
    ranges = [(ci, s, k) for ci in range(3) for s, k in chunk_ranges(chunks[ci])[:7]]
    want = expected(oracle, chunks, ranges)
    res = [-1 if ci == 1 else r for (ci, _, _), (r, _) in zip(ranges, want)]
    total = prefix(res)[-1]
    b = pkg.ItemRanges(ranges)
    out, optr = mem.filled(total + 64, SENTINEL)
    assert b.packed(cptr, offs[-1], offs, optr, total) == 0
    assert b.results() == res and b.offsets() == prefix(res)
    got = mem.get(out)
    assert np.array_equal(got[:total], np.concatenate([d for (ci, _, _), (r, d) in zip(ranges, want) if ci != 1 and r > 0])) and np.all(got[total:] == SENTINEL)
    assert b.packed(cptr, offs[-1] - 1, offs, None, 0) < 0                           # tables that are unusable as a whole
    assert b.packed(cptr, offs[-1], [0, 5, 4, offs[-1]], None, 0) < 0


def test_one_pipeline_per_call(pkg, lib, mem, oracle):
    """1000 single-item ranges over 8 LZ4 chunks: one launch of the decode kernel and one of the gather kernel"""
    rng = np.random.default_rng(8)
    chunks = [orc_compress(oracle, plain(BIG, seed=20 + k), 8, 5, 1, "lz4")[1] for k in range(8)]
    ni = BIG // 8
    ranges = [(int(rng.integers(0, 8)), int(rng.integers(0, ni)), 1) for _ in range(1000)]
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        check_batch(pkg, lib, mem, oracle, chunks, ranges)
        assert pkg.profile_get("k_decode_streams")[1] == 1 and pkg.profile_get("k_getitem_gather")[1] == 1
    finally:
        lib.blosc_gpu_profile(0)


# ---- the single calls: one range of one chunk through the same pipeline ----
# blosc_getitem finds out by itself where each pointer lies: all four combinations of host and device memory; blosc_gpu_getitem: device memory
SINGLE = [("blosc_getitem", "host", "host"), ("blosc_getitem", "host", "device"), ("blosc_getitem", "device", "host"),
          ("blosc_getitem", "device", "device"), ("blosc_gpu_getitem", "device", "device")]
SINGLE_IDS = [f"{e}-{a}-to-{b}" for e, a, b in SINGLE]


def single_call(lib, mem, case):
    entry, src, dst = case
    call = lib.blosc_getitem if entry == "blosc_getitem" else (lambda p, s, k, d: lib.blosc_gpu_getitem(p, s, k, d, None))
    return call, (mem if src == "device" else NumpyMem()), (mem if dst == "device" else NumpyMem())


@pytest.fixture(scope="module")
def single_chunks(pkg, mem, oracle, ref):
    return single_grid_chunks(oracle, ref, lambda d, T, shuffle, cname, bs: lib_chunks(pkg, mem, [d], T, shuffle, cname, bs)[0])


@pytest.fixture(scope="module")
def damaged(pkg, mem, oracle, ref):
    out = damaged_single_chunks(oracle, ref, lambda d, T, shuffle, cname, bs: lib_chunks(pkg, mem, [d], T, shuffle, cname, bs)[0])
    assert len({n.split(",")[0] for n, _, _ in out}) == 4
    return out


@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_single_call_grid(lib, mem, oracle, ref, single_chunks, case):
    call, src_mem, dst_mem = single_call(lib, mem, case)
    for cname, chunk in single_chunks:
        got = check_single(call, src_mem, dst_mem, oracle, ref, chunk, chunk_ranges(chunk), (case, cname))
        assert got[-2] == -1                                       # start = -1


@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_single_call_in_passes(lib, mem, oracle, ref, single_chunks, case):
    """a pass bound of 16 KiB: a single chunk beyond the bound still decodes, as a pass of its own"""
    call, src_mem, dst_mem = single_call(lib, mem, case)
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        for cname, chunk in single_chunks:
            check_single(call, src_mem, dst_mem, oracle, ref, chunk, chunk_ranges(chunk), (case, cname, "16 KiB passes"))
    finally:
        lib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("case", SINGLE, ids=SINGLE_IDS)
def test_single_call_on_damaged_blocks(lib, mem, oracle, ref, damaged, case):
    call, src_mem, dst_mem = single_call(lib, mem, case)
    check_damage(call, src_mem, dst_mem, oracle, ref, damaged, case)
