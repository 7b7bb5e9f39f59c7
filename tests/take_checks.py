"""What tests/test_gpu_take.py (device) and tests/test_emu_take.py (wavefront emulator) both assert about the calls of include/blosc_gpu_take.h,
and the cases they run.  Expected bytes never come from the library under test: the plaintext of every chunk is the oracle's orc_decompress,
the expected row k is a numpy slice of the concatenated plaintexts, and a damaged block's code is the oracle's orc_getitem on one item at
the block's start.  `mem` is getitem_ranges_checks' NumpyMem / TorchMem: how a test reaches "device" memory."""
import numpy as np

from getitem_ranges_checks import plain
from helpers import header, orc_compress, orc_decompress, ptr

SENTINEL = 0xA5
STATUS_SENTINEL = np.int32(-1515870811)      # 0xA5A5A5A5
# 40 800 = 2^5 * 3 * 5^2 * 17: every row size below divides it.  With blocksize 8192 that is five blocks (at typesize 17 blocks are 8177
# bytes); the split typesizes, whose blocks are widened to 64 KiB, take 8 N: again five blocks
N = 40800
BLOCKSIZE = 8192
# 4080: large, a multiple of 16, divides neither block size - rows cross boundaries; 20 400: a row over three or four blocks
ROW_SIZES = [1, 2, 4, 8, 12, 16, 17, 24, 32, 48, 96, 4080, 20400]
ALL_OFFSETS = (1, 12, 17, 4080)                  # row sizes that run at every offset 0 ... 15 of dest from a 16-byte boundary; the rest at 0 and 5
MEMCPYED_BYTES = 8160
OUT_OF_BOUNDS = [-1, None, 2 ** 40, -2 ** 63, 2 ** 63 - 1]      # None: nrows


def offsets_for(row_bytes):
    return range(16) if row_bytes in ALL_OFFSETS else (0, 5)


def batch_chunks(oracle, write, row_bytes, scale=1):
    """The chunks of one call, each a multiple of row_bytes long: N * scale bytes, a chunk of nbytes 0 in the middle, N * scale / 2 where
    row_bytes divides it, a MEMCPYED chunk of random bytes (not for 20 400).  write(k, data) -> chunk k of the compressible ones"""
    n = N * scale
    out = [write(0, plain(n)), orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1]]
    if (n // 2) % row_bytes == 0:
        out.append(write(1, plain(n // 2, seed=12)))
    if MEMCPYED_BYTES % row_bytes == 0:
        out.append(orc_compress(oracle, np.random.default_rng(3).integers(0, 256, MEMCPYED_BYTES, dtype=np.uint8), 4, 5, 1, "lz4")[1])
        assert header(out[-1])["flags"] & 2
    assert header(out[1])["nbytes"] == 0 and all(header(c)["nbytes"] % row_bytes == 0 for c in out)
    return out


MANY_SHAPES = [0, 48, 144, 480, 1536]            # nbytes of chunk k of many_chunks: k % 5 picks; multiples of 48, so rows of 4, 12 and 48 bytes divide them
MANY_EMPTY = (range(100, 103), range(700, 704), range(1022, 1025))      # stretches of chunks without rows; the last one lies across chunk 1024
MANY_COUNTS = (1024, 1025, 1300)                 # k_take.hip's TK_LDS_CHUNKS = 1024: the last batch that bisects the LDS copy, the first and a later one that bisect global memory


def many_chunks(oracle, write, row_bytes, nchunks, made=None):
    """More chunks than the kernels' LDS table of row_first holds, small ones: chunk k has MANY_SHAPES[k % 5] bytes - none; 48 and 144, which
    the oracle stores MEMCPYED; 480 in one block, by write(k, data); 1536 in four blocks of 510.  The first chunk, the last two and the
    stretches of MANY_EMPTY have no rows.  Chunk k is the same in every batch that holds it with rows (made: a dict that keeps them between
    calls), so the batch of 1025 is the batch of 1024 and one chunk more"""
    made = {} if made is None else made
    empty = orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1]
    out = []
    for k in range(nchunks):
        n = MANY_SHAPES[k % 5]
        if n == 0 or k >= nchunks - 2 or any(k in s for s in MANY_EMPTY):
            out.append(empty)
            continue
        if k not in made:
            rng = np.random.default_rng(1000 + k)
            data = np.resize(rng.integers(0, 256, 96, dtype=np.uint8), n).copy()      # a period of 96 bytes with a little noise: every block compresses
            data[rng.integers(0, n, n // 97 + 1)] ^= 1
            if n == 480: c = write(k, data)
            elif n == 1536: c = orc_compress(oracle, data, 17, 5, 1, "lz4", blocksize=512)[1]      # (typesize 17 is not split: the block size stands)
            else: c = orc_compress(oracle, data, 4, 5, 1, "lz4")[1]
            h = header(c)
            assert h["nbytes"] == n and (n > 144 or h["flags"] & 2), (k, h)
            assert n != 480 or h["blocksize"] >= n, (k, h)
            assert n != 1536 or (not h["flags"] & 2 and -(-n // h["blocksize"]) >= 3), (k, h)
            made[k] = c
        out.append(made[k])
    rows = [header(c)["nbytes"] for c in out]
    assert all(n % row_bytes == 0 for n in rows) and rows[0] == 0 and rows[-1] == 0 and rows[-2] == 0
    runs = "".join("e" if n == 0 else "." for n in rows).split(".")
    assert sum(1 for r in runs if len(r) >= 3) >= 2, "two stretches of three or more chunks without rows"
    return out


def plaintext(oracle, chunks):
    """the rows of a call: the oracle's plaintext of every chunk, end to end"""
    parts = []
    for c in chunks:
        n = header(c)["nbytes"]
        r, out = orc_decompress(oracle, c, n)
        assert r == n, "the oracle cannot read a chunk of the batch"
        parts.append(np.asarray(out[:n], np.uint8))
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


def chunk_rows(chunks, row_bytes):
    return [header(c)["nbytes"] // row_bytes for c in chunks]


def index_sets(chunks, row_bytes, seed=5):
    """name -> int64 indices: every row in order and reversed, 3000 random rows with repeats, the first and last row of every chunk, the rows
    ending at, starting at and crossing every block boundary of every chunk, out-of-bounds values among good ones, and no index at all"""
    rows = chunk_rows(chunks, row_bytes)
    first = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    nrows = int(first[-1])
    rng = np.random.default_rng(seed)
    sets = {"in order": np.arange(nrows, dtype=np.int64), "reversed": np.arange(nrows, dtype=np.int64)[::-1].copy(),
            "random": rng.integers(0, nrows, 3000).astype(np.int64)}
    edges = []
    for k, c in enumerate(chunks):
        h = header(c)
        if not rows[k]:
            continue
        edges += [int(first[k]), int(first[k + 1]) - 1]
        if h["flags"] & 2:
            continue
        for b in range(h["blocksize"], h["nbytes"], h["blocksize"]):      # the row that holds byte b - 1, the one that holds byte b, their neighbours
            edges += [int(first[k]) + r for r in {(b - 1) // row_bytes - 1, (b - 1) // row_bytes, b // row_bytes, b // row_bytes + 1} if 0 <= r < rows[k]]
    sets["edges"] = np.array(edges, np.int64)
    good = rng.integers(0, nrows, 3 * len(OUT_OF_BOUNDS)).astype(np.int64)
    mixed = []
    for k, bad in enumerate(OUT_OF_BOUNDS):
        mixed += [int(good[3 * k]), nrows if bad is None else bad, int(good[3 * k + 1]), int(good[3 * k + 2])]
    sets["out of bounds"] = np.array(mixed, np.int64)
    sets["none"] = np.zeros(0, np.int64)
    return sets


def damaged_rows(oracle, chunks, row_bytes, which, bad_chunk, blk):
    """per row of the call 0, or the code of block `blk` of chunk `which` - replaced by its damaged copy bad_chunk - for the rows that touch it:
    what the oracle's orc_getitem answers for one item at the start of that block"""
    h = header(bad_chunk)
    bs, T = h["blocksize"], h["typesize"]
    buf = np.zeros(T + 16, np.uint8)
    code = oracle.orc_getitem(ptr(bad_chunk), blk * (bs // T), 1, ptr(buf))
    assert code < 0, "the oracle reads the damaged block"
    rows = chunk_rows(chunks, row_bytes)
    base = sum(rows[:which]) * row_bytes
    lo, hi = base + blk * bs, base + min((blk + 1) * bs, h["nbytes"])
    codes = np.zeros(sum(rows), np.int32)
    codes[lo // row_bytes:(hi - 1) // row_bytes + 1] = code
    return codes, code


def expected(rows_plain, row_bytes, index, row_code=None):
    """(status [nidx], dest bytes [nidx, row_bytes] with the sentinel where nothing is written)"""
    nrows = rows_plain.size // row_bytes
    idx = np.asarray(index, np.int64)
    ok = (idx >= 0) & (idx < nrows)
    status = np.where(ok, row_bytes, -1).astype(np.int32)
    if row_code is not None and ok.any():
        c = row_code[idx[ok]]
        status[ok] = np.where(c < 0, c, row_bytes)
    dest = np.full((idx.size, row_bytes), SENTINEL, np.uint8)
    good = status > 0
    dest[good] = rows_plain[:nrows * row_bytes].reshape(nrows, row_bytes)[idx[good]]
    return status, dest


class TakeSource:
    """the chunks of a call in "device" memory: src pointers ("batch"), or one container with its offset table ("packed")"""
    def __init__(self, mem, chunks=None, container=None, offsets=None):
        self.mem = mem
        if chunks is not None:
            self.keep = [mem.put(np.asarray(c, np.uint8)) for c in chunks]
            self.ptrs = [p for _, p in self.keep]
        else:
            self.keep = mem.put(np.asarray(container, np.uint8))
            self.container, self.size, self.offsets = self.keep[1], int(container.size), [int(o) for o in offsets]
        self.packed = chunks is None

    def call(self, take, index_ptr, nidx, dest, status, stream=None):
        if self.packed:
            return take.packed(self.container, self.size, self.offsets, index_ptr, nidx, dest, status, stream=stream)
        return take.batch(self.ptrs, index_ptr, nidx, dest, status, stream=stream)


def pack_container(chunks, align=256):
    """chunks end to end at multiples of `align`: (container, offsets [n + 1])"""
    off, parts = [0], []
    for c in chunks:
        pad = (-c.size) % align
        parts += [np.asarray(c, np.uint8), np.zeros(pad, np.uint8)]
        off.append(off[-1] + c.size + pad)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), off


GUARD = 48


def run_take(pkgmod, lib, mem, source, row_bytes, index, offset=0, with_status=True, stream=None):
    """One call (stream: the caller's stream, default the NULL stream).  dest lies `offset` bytes behind a 16-byte boundary inside a buffer of sentinels, the status table between sentinel words.
    Returns (answer, dest bytes [nidx, row_bytes], status [nidx] or None, chunk_rows, failed); the sentinels around both are asserted here"""
    idx = np.ascontiguousarray(np.asarray(index, np.int64))
    nidx = int(idx.size)
    keep_i, index_ptr = mem.put(idx.view(np.uint8))
    assert index_ptr % 8 == 0
    total = nidx * row_bytes
    out, base = mem.filled(total + 2 * GUARD, SENTINEL)
    at = (-base) % 16 + 16 + offset
    st_h, st_base = (mem.filled(4 * (nidx + 8), SENTINEL) if with_status else (None, 0))
    take = pkgmod.RowTake(row_bytes, lib=lib)
    rc = source.call(take, index_ptr if nidx else None, nidx, (base + at) if nidx else None, (st_base + 16) if with_status else None, stream)
    buf = mem.get(out)[:total + 2 * GUARD]
    assert np.all(buf[:at] == SENTINEL) and np.all(buf[at + total:] == SENTINEL), "bytes outside dest were written"
    status = None
    if with_status:
        words = np.ascontiguousarray(mem.get(st_h)[:4 * (nidx + 8)]).view(np.int32)
        assert np.all(words[:4] == STATUS_SENTINEL) and np.all(words[4 + nidx:] == STATUS_SENTINEL), "words outside status were written"
        status = words[4:4 + nidx].copy()
    del keep_i
    return rc, buf[at:at + total].reshape(nidx, row_bytes).copy(), status, take.chunk_rows(), take.failed()


def check_take(pkgmod, lib, mem, source, chunks, rows_plain, row_bytes, index, offset=0, with_status=True, row_code=None, what="", stream=None, keep=None):
    """the bytes, the status table, failed_out and chunk_rows_out of one call; rows with a negative status still hold the sentinel.
    keep: a dict that receives what the call gave (dest, status, chunk_rows, failed), for callers that compare two calls"""
    want_status, want = expected(rows_plain, row_bytes, index, row_code)
    rc, got, status, rows, failed = run_take(pkgmod, lib, mem, source, row_bytes, index, offset, with_status, stream)
    if keep is not None:
        keep.update(dest=got, status=status, chunk_rows=np.array(rows, np.int64), failed=np.array([failed], np.int64))
    what = (what, "row_bytes", row_bytes, "offset", offset, "status" if with_status else "no status")
    assert rc == 0, (what, rc)
    assert rows == chunk_rows(chunks, row_bytes), (what, rows)
    if with_status:
        bad = np.flatnonzero(status != want_status)
        assert bad.size == 0, (what, "status", [(int(k), int(index[k]), int(status[k]), int(want_status[k])) for k in bad[:8]])
    assert failed == int((want_status < 0).sum()), (what, "failed", failed, int((want_status < 0).sum()))
    if not np.array_equal(got, want):
        k = int(np.flatnonzero((got != want).any(axis=1))[0])
        raise AssertionError((what, "row", k, "index", int(index[k]), "first byte", int(np.flatnonzero(got[k] != want[k])[0]), int((got != want).sum())))
    return want_status


def check_census_failure(pkgmod, lib, mem, source, row_bytes, want_rows, what=""):
    """a call with an unusable chunk: -1, the chunks' rows and codes in chunk_rows_out, dest and status untouched"""
    index = np.array([0, 1, 2], np.int64)
    rc, got, status, rows, failed = run_take(pkgmod, lib, mem, source, row_bytes, index)
    assert rc == -1 and rows == want_rows, (what, rc, rows, want_rows)
    assert np.all(got == SENTINEL) and np.all(status == STATUS_SENTINEL) and failed == 0, (what, "something was written")
    rc, _, _, rows, _ = run_take(pkgmod, lib, mem, source, row_bytes, np.zeros(0, np.int64))
    assert rc == -1 and rows == want_rows, (what, "census alone", rc, rows)
