"""What tests/test_gpu_getitem_ranges.py (device) and tests/test_emu_getitem_ranges.py (wavefront emulator) both assert about the calls of
include/blosc_gpu_getitem.h (check_batch) and about the single calls blosc_getitem / blosc_gpu_getitem that the same pipeline serves (check_single).  Expected results and bytes come from the oracle's orc_getitem on the same chunk, range by range, never from
the library under test.  `mem` is how a test reaches "device" memory: mem.put(array) -> (keep-alive handle, address), mem.get(handle) ->
host array, mem.filled(n, value) -> (handle, address)."""
import numpy as np

from helpers import header, orc_compress, ptr, ref_compress

SENTINEL = 0xA5
SMALL = 40 * 1024 + 24          # with blocksize 8192: five blocks and a leftover where the block is not split (typesize 17) - a split block
BIG = 5 * 65536 + 24            # is widened to 64 KiB (blosc.c:1037-1048), so the split settings get their five blocks and a leftover here
BLOCKSIZE = 8192
TYPESIZES = [1, 2, 4, 8, 17]
SHUFFLES = [0, 1, 2]


def plain(n, seed=11):
    """bytes every setting compresses (a period of 331 bytes with a little noise), so that no chunk of the grid ends up MEMCPYED"""
    rng = np.random.default_rng(seed)
    d = np.resize(rng.integers(0, 256, 331, dtype=np.uint8), n).copy()
    if n:
        d[rng.integers(0, n, n // 97)] ^= 1
    return d


class NumpyMem:
    """the emulator's "device" memory is the host's"""
    def put(self, a):
        a = np.ascontiguousarray(a).copy() if a.size else np.zeros(1, np.uint8)
        return a, a.ctypes.data

    def filled(self, n, value):
        a = np.full(max(n, 1), value, np.uint8)
        return a, a.ctypes.data

    def get(self, h):
        return h


class TorchMem:
    def __init__(self):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")

    def put(self, a):
        t = self.torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.dev) if a.size else self.torch.zeros(1, dtype=self.torch.uint8, device=self.dev)
        return t, t.data_ptr()

    def filled(self, n, value):
        t = self.torch.full((max(n, 1),), value, dtype=self.torch.uint8, device=self.dev)
        return t, t.data_ptr()

    def get(self, h):
        return h.cpu().numpy()


def chunk_ranges(chunk):
    """the ranges of case 1 for one chunk, as (start, nitems): whatever the chunk's shape, the oracle says what each of them gives"""
    h = header(chunk)
    T, nbytes, bs = max(h["typesize"], 1), h["nbytes"], max(h["blocksize"], 1)
    ni, bi = nbytes // T, max(bs // T, 1)
    nblocks = -(-nbytes // bs)
    b1 = bi if nblocks > 1 else 0                       # first item of block 1 where there is one
    last_full = (nblocks - 2) * bi if nblocks > 1 else 0
    cl = lambda s, k: (max(min(s, ni), 0), max(min(k, ni - max(min(s, ni), 0)), 0))
    return [
        (0, ni), (0, min(1, ni)), (max(ni - 1, 0), min(1, ni)), (ni // 2, 0),      # whole, first item, last item, empty
        cl(b1 + 3, 5),                                    # inside one block
        cl(max(b1 - 2, 0), 5),                            # across a block boundary
        cl(last_full + 3, ni),                            # ends in the leftover block
        cl(10, 20), cl(20, 20), cl(10, 20),               # two that overlap and share a block, an exact duplicate
        (-1, 1), (max(ni - 1, 0), 2),                     # start = -1; one past the end
    ]


def expected(oracle, chunks, ranges):
    """[(result, bytes)] of the oracle for (chunk index, start, nitems) triples; a chunk index outside the table answers -1"""
    out = []
    for ci, s, k in ranges:
        if not 0 <= ci < len(chunks):
            out.append((-1, None)); continue
        T = max(header(chunks[ci])["typesize"], 1)
        buf = np.full(max(k, 0) * T + 16, SENTINEL, np.uint8)
        r = oracle.orc_getitem(ptr(chunks[ci]), s, k, ptr(buf))
        # (a range that fails in a later block has its earlier blocks' bytes in the oracle's buffer, as in blosc_getitem's; the batched calls write nothing for it)
        assert r < 0 or np.all(buf[r:] == SENTINEL), "the oracle wrote more than it returned"
        out.append((r, buf[:max(r, 0)].copy()))
    return out


def slot_widths(chunks, ranges):
    return [max(k, 0) * max(header(chunks[ci])["typesize"], 1) if 0 <= ci < len(chunks) else max(k, 0) * 8 for ci, s, k in ranges]


def odd_slots(widths):
    """every slice's place inside one buffer: at odd addresses of every residue modulo 16, a gap between neighbours"""
    at, off = [], 1
    for r, w in enumerate(widths):
        off += 2 * (r % 8)
        at.append(off)
        off += w + 1
        off += off % 2 == 0
    return at, off + 64


def check_batch(pkgmod, lib, mem, oracle, chunks, ranges, what="", stream=None, keep=None):
    """one blosc_gpu_getitem_batch over `ranges` = (chunk, start, nitems) triples: every result and every byte the oracle's; destinations at odd
    offsets inside one buffer of sentinels; every byte outside the slices and every byte of a failed range's slot still the sentinel.
    stream: the caller's stream (default the NULL stream); keep: a dict that receives the results and the whole buffer as the call left them"""
    want = expected(oracle, chunks, ranges)
    at, total = odd_slots(slot_widths(chunks, ranges))
    assert all(a % 2 == 1 for a in at)
    dev = [mem.put(c) for c in chunks]
    out, base = mem.filled(total, SENTINEL)
    b = pkgmod.ItemRanges(ranges, lib=lib)
    assert b.batch([p for _, p in dev], [base + a for a in at], stream=stream) == 0, what
    got = b.results()
    if keep is not None:
        keep.update(results=np.array(got, np.int64), bytes=mem.get(out)[:total].copy())
    exp = np.full(total, SENTINEL, np.uint8)
    for a, (r, data) in zip(at, want):
        if r > 0: exp[a:a + r] = data
    res_want = [r for r, _ in want]
    assert got == res_want, (what, [(k, ranges[k], g, w) for k, (g, w) in enumerate(zip(got, res_want)) if g != w][:8])
    buf = mem.get(out)[:total]
    if not np.array_equal(buf, exp):
        bad = int(np.flatnonzero(buf != exp)[0])
        k = max(j for j, a in enumerate(at) if a <= bad) if bad >= at[0] else -1
        raise AssertionError((what, "byte", bad, "range", k, ranges[k] if k >= 0 else None, "slot at", at[k] if k >= 0 else None, int((buf != exp).sum())))
    return got


def expected_single(oracle, ref, chunk, start, nitems):
    """(result, bytes) of one blosc_getitem: the reference's where it is built, the oracle's otherwise.  The chunk lies in front of 256 zero
    bytes: a damaged bstarts entry sends the reader behind the chunk"""
    T = max(header(chunk)["typesize"], 1)
    padded = np.concatenate([np.asarray(chunk, np.uint8), np.zeros(256, np.uint8)])
    buf = np.full(max(nitems, 0) * T + 16, SENTINEL, np.uint8)
    fn = ref.blosc_getitem if ref is not None else oracle.orc_getitem
    r = fn(ptr(padded), start, nitems, ptr(buf))
    assert r < 0 or np.all(buf[r:] == SENTINEL), "the checker wrote more than it returned"
    return r, buf[:max(r, 0)].copy()


def check_single(call, src_mem, dst_mem, oracle, ref, chunk, ranges, what=""):
    """One `call(src address, start, nitems, dest address)` - blosc_getitem or blosc_gpu_getitem - per (start, nitems) of `ranges` on one
    chunk held in src_mem: every result and every byte those of expected_single.  Every destination sits at offset 1 of a buffer of sentinels
    in dst_mem, and every byte outside [1, 1 + max(result, 0)) is still the sentinel afterwards: a call that fails writes nothing."""
    T = max(header(chunk)["typesize"], 1)
    keep, src = src_mem.put(chunk)
    got = []
    for s, k in ranges:
        r, data = expected_single(oracle, ref, chunk, s, k)
        total = 1 + max(k, 0) * T + 33
        out, base = dst_mem.filled(total, SENTINEL)
        res = call(src, s, k, base + 1)
        buf = dst_mem.get(out)[:total]
        print(what, (s, k), "->", res, "want", r)
        assert res == r, (what, (s, k), res, r)
        exp = np.full(total, SENTINEL, np.uint8)
        exp[1:1 + max(r, 0)] = data
        assert np.array_equal(buf, exp), (what, (s, k), "byte", int(np.flatnonzero(buf != exp)[0]), int((buf != exp).sum()))
        got.append(res)
    del keep
    return got


def single_grid_chunks(oracle, ref, lib_compress):
    """the chunks of the single-call grid as (name, chunk): Zstd and zlib written by the reference where it is built and by the library under
    test (lib_compress(data, typesize, shuffle, cname, blocksize)) otherwise, LZ4 and BloscLZ by the oracle; the three specials"""
    small = plain(SMALL)
    out = []
    for T, shuffle, cname in ((17, 1, "lz4"), (17, 2, "blosclz"), (4, 2, "zstd"), (8, 1, "zlib"), (17, 0, "zstd")):
        if cname in ("lz4", "blosclz"): c = orc_compress(oracle, small, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        elif ref is not None: c = ref_compress(ref, small, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
        else: c = lib_compress(small, T, shuffle, cname, BLOCKSIZE)
        out.append((f"{cname} T{T} shuffle {shuffle}", c))
    out.append(("memcpyed", orc_compress(oracle, np.random.default_rng(3).integers(0, 256, 9000, dtype=np.uint8), 4, 5, 1, "lz4")[1]))
    out.append(("100 bytes", orc_compress(oracle, plain(100), 4, 5, 1, "lz4")[1]))
    out.append(("empty", orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1]))
    assert header(out[-3][1])["flags"] & 2 and header(out[-1][1])["nbytes"] == 0
    assert all(-(-header(c)["nbytes"] // header(c)["blocksize"]) >= 5 for _, c in out[:5] if header(c)["typesize"] == 17)
    return out


def damaged_single_chunks(oracle, ref, lib_compress):
    """(name, damaged chunk, its three ranges) for pick_damage on a SMALL typesize-17 shuffle-1 chunk of each of the four codecs"""
    out = []
    for cname in ("lz4", "blosclz", "zstd", "zlib"):
        if cname in ("lz4", "blosclz"): c = orc_compress(oracle, plain(SMALL), 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
        elif ref is not None: c = ref_compress(ref, plain(SMALL), 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
        else: c = lib_compress(plain(SMALL), 17, 1, cname, BLOCKSIZE)
        found, rngs = pick_damage(oracle, c)
        out += [(f"{cname}, {kind}", bad, rngs) for kind, bad in found]
    return out


def check_damage(call, src_mem, dst_mem, oracle, ref, damaged, what=""):
    """the range inside the damaged block and the one crossing into it answer the checker's negative code and write nothing, the range in the
    block before it answers its bytes"""
    for name, bad, rngs in damaged:
        got = check_single(call, src_mem, dst_mem, oracle, ref, bad, rngs, (what, name))
        assert got[0] < 0 and got[1] == 7 * 17 and got[2] < 0, (what, name, got)


def pick_damage(oracle, chunk):
    """A damaged copy of a chunk of several blocks, and two ranges: one inside the damaged block (the oracle answers a negative code) and one
    inside the block before it (the oracle answers its bytes).  The damage is chosen on the CPU so that the oracle alone gives that split:
    the block's bstarts entry sent behind the chunk, or its first stream's size word made negative.  Returns (damaged, [(start, nitems)] * 3,
    the third range crossing from the good block into the damaged one)."""
    h = header(chunk)
    T, bs = h["typesize"], h["blocksize"]
    nblocks = -(-h["nbytes"] // bs)
    assert nblocks >= 3 and not h["flags"] & 2, h
    bi = bs // T
    blk = 2
    rng_bad, rng_good, rng_both = (blk * bi + 5, 7), ((blk - 1) * bi + 5, 7), (blk * bi - 3, 7)
    found = []
    for kind in ("bstarts", "size word"):
        t = chunk.copy()
        if kind == "bstarts":
            t[16 + 4 * blk:20 + 4 * blk] = np.array([h["cbytes"] + 100], "<i4").view(np.uint8)
        else:
            at = int(chunk[16 + 4 * blk:20 + 4 * blk].view("<i4")[0])
            t[at:at + 4] = np.array([-5], "<i4").view(np.uint8)
        buf = np.zeros(8 * T + 16, np.uint8)
        r_bad = oracle.orc_getitem(ptr(t), rng_bad[0], rng_bad[1], ptr(buf))
        r_good = oracle.orc_getitem(ptr(t), rng_good[0], rng_good[1], ptr(buf))
        if r_bad < 0 and r_good == rng_good[1] * T:
            found.append((kind, t))
    assert found, "no damage gives the split with the oracle alone"
    return found, [rng_bad, rng_good, rng_both]


def prefix(results):
    off = [0]
    for r in results:
        off.append(off[-1] + max(r, 0))
    return off
