"""What tests/test_gpu_put.py (device) and tests/test_emu_put.py (wavefront emulator) both assert about the calls of include/blosc_gpu_put.h,
and the cases they run.  Expected bytes never come from the library under test: the plaintext of every source chunk is the oracle's
orc_decompress, the rows are applied to it by a numpy loop in index order (the last occurrence wins), and the plaintext of every chunk of the
new container is again the oracle's orc_decompress.  `mem` is getitem_ranges_checks' NumpyMem / TorchMem: how a test reaches "device" memory."""
import numpy as np

from helpers import header, orc_decompress
from take_checks import OUT_OF_BOUNDS, SENTINEL, STATUS_SENTINEL, TakeSource, chunk_rows, index_sets  # noqa: F401

GUARD = 64
ALIGNS = (1, 16, 256)


def put_index_sets(chunks, row_bytes, seed=5):
    """take's index sets and three more: one row a thousand times (every occurrence contends for one owner word), the rows of one chunk only
    (the others come through untouched), and - already among take's - none at all"""
    sets = index_sets(chunks, row_bytes, seed)
    rows = chunk_rows(chunks, row_bytes)
    first = np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)
    rng = np.random.default_rng(seed + 1)
    sets["one row a thousand times"] = np.full(1000, int(first[-1]) // 3, np.int64)
    last = max(k for k, r in enumerate(rows) if r)
    sets["one chunk only"] = rng.integers(int(first[last]), int(first[last + 1]), 200).astype(np.int64)
    assert sets["none"].size == 0
    return sets


def new_rows(nidx, row_bytes, seed=7):
    """the rows of a call, [nidx, row_bytes]: bytes that tell every k from every other, so a mix of two occurrences cannot pass"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 4, (nidx, row_bytes), dtype=np.uint8)      # (compressible)
    tag = np.arange(nidx, dtype=np.uint32)
    for b in range(min(row_bytes, 4)):
        rows[:, b] = (tag >> (8 * b)) & 0xff if row_bytes >= 2 else (tag * 37 + 11) & 0xff
    return rows


def oracle_plains(oracle, chunks):
    """the oracle's plaintext of every chunk, or None where it cannot read the chunk"""
    out = []
    for c in chunks:
        n = header(c)["nbytes"]
        r, buf = orc_decompress(oracle, c, n)
        out.append(np.asarray(buf[:n], np.uint8).copy() if r == n else None)
    return out


def expected(oracle, chunks, row_bytes, index, rows):
    """(plaintexts after the put - None: the chunk is carried over -, rewritten [n], status [nidx]) by a numpy loop in index order"""
    plains = oracle_plains(oracle, chunks)
    counts = chunk_rows(chunks, row_bytes)
    first = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    nrows = int(first[-1])
    rewritten = [0] * len(chunks)
    status = np.full(len(index), -1, np.int32)
    idx = np.asarray(index, np.int64)
    valid = np.flatnonzero((idx >= 0) & (idx < nrows))
    owner = np.searchsorted(first, idx[valid], side="right") - 1      # (of chunks without rows, which share their successor's first row, the successor)
    for c in np.unique(owner).tolist():
        ks = valid[owner == c]                                        # the indices of chunk c, in index order
        if plains[c] is None:
            rewritten[c] = -1
            continue
        rewritten[c] = 1
        status[ks] = row_bytes
        table = plains[c].reshape(counts[c], row_bytes)
        if ks.size <= 4096:
            for k in ks.tolist():                                     # index order: a later occurrence overwrites an earlier one
                table[int(idx[k] - first[c])] = rows[k]
        else:                                                         # the same loop, its last assignment per row found first
            rows_of, pos = np.unique((idx[ks] - first[c])[::-1], return_index=True)
            table[rows_of] = np.asarray(rows)[ks[ks.size - 1 - pos]]
    return [p if w == 1 else None for p, w in zip(plains, rewritten)], rewritten, status


def bound(chunks, align):
    return sum(-(-(header(c)["nbytes"] + 16) // align) * align for c in chunks)


def run_put(pkgmod, lib, mem, source, chunks, row_bytes, index, rows, params, align=1, offset=0, with_status=True, destsize=None, stream=None):
    """One call (stream: the caller's stream, default the NULL stream).  `rows` lies `offset` bytes behind a 16-byte boundary, dest (destsize bytes, default the bound) inside a buffer of sentinels,
    the status table between sentinel words.  Returns (answer, dest bytes, status or None, the RowPut); the sentinels around dest and status
    and the bytes of the source are asserted here"""
    idx = np.ascontiguousarray(np.asarray(index, np.int64))
    nidx = int(idx.size)
    keep_i, index_ptr = mem.put(idx.view(np.uint8))
    held = np.zeros(nidx * row_bytes + 48, np.uint8)
    held[16 + offset:16 + offset + nidx * row_bytes] = np.asarray(rows, np.uint8).reshape(-1)
    keep_r, rows_base = mem.put(held)
    assert index_ptr % 8 == 0 and rows_base % 16 == 0
    cap = bound(chunks, align) if destsize is None else destsize
    out, base = mem.filled(cap + 2 * GUARD + 256, SENTINEL)
    at = (-base) % 256 + GUARD      # (no alignment of dest is promised to the call: 64 bytes behind a 256-byte boundary)
    st_h, st_base = (mem.filled(4 * (nidx + 8), SENTINEL) if with_status else (None, 0))
    before = [mem.get(h).copy() for h, _ in source.keep] if not source.packed else mem.get(source.keep[0]).copy()
    put = pkgmod.RowPut(row_bytes, lib=lib)
    args = (index_ptr if nidx else None, nidx, (rows_base + 16 + offset) if nidx else None, params, base + at, cap, align, (st_base + 16) if with_status else None)
    rc = put.packed(source.container, source.size, source.offsets, *args, stream=stream) if source.packed else put.batch(source.ptrs, *args, stream=stream)
    buf = mem.get(out)
    assert np.all(buf[:at] == SENTINEL) and np.all(buf[at + cap:] == SENTINEL), "bytes outside dest were written"
    status = None
    if with_status:
        words = np.ascontiguousarray(mem.get(st_h)[:4 * (nidx + 8)]).view(np.int32)
        assert np.all(words[:4] == STATUS_SENTINEL) and np.all(words[4 + nidx:] == STATUS_SENTINEL), "words outside status were written"
        status = words[4:4 + nidx].copy()
    after = [mem.get(h) for h, _ in source.keep] if not source.packed else mem.get(source.keep[0])
    assert all(np.array_equal(a, b) for a, b in zip(after, before)) if not source.packed else np.array_equal(after, before), "the source was written"
    del keep_i, keep_r
    return rc, buf[at:at + cap].copy(), status, put


def check_put(pkgmod, lib, mem, oracle, source, chunks, row_bytes, index, params, align=1, offset=0, with_status=True, destsize=None, seed=7, what="",
              stream=None, keep=None):
    """everything include/blosc_gpu_put.h says about one call that passes the census.  Returns (dest bytes, the RowPut, the expected plaintexts).
    keep: a dict that receives what the call gave (dest, status and the host tables), for callers that compare two calls"""
    rows = new_rows(len(index), row_bytes, seed)
    want_plain, want_rew, want_status = expected(oracle, chunks, row_bytes, index, rows)
    rc, dest, status, put = run_put(pkgmod, lib, mem, source, chunks, row_bytes, index, rows, params, align, offset, with_status, destsize, stream)
    if keep is not None:
        keep.update(dest=dest, status=status, offsets=np.array(put.offsets(), np.int64), cbytes=np.array(put.results(), np.int64),
                    rewritten=np.array(put.rewritten(), np.int64), chunk_rows=np.array(put.chunk_rows(), np.int64), failed=np.array([put.failed()], np.int64))
    what = (what, "row_bytes", row_bytes, "offset", offset, "align", align, "status" if with_status else "no status")
    cap = dest.size
    assert rc == 0, (what, rc)
    assert put.chunk_rows() == chunk_rows(chunks, row_bytes), (what, put.chunk_rows())
    assert put.rewritten() == want_rew, (what, "rewritten", put.rewritten(), want_rew)
    if with_status:
        bad = np.flatnonzero(status != want_status)
        assert bad.size == 0, (what, "status", [(int(k), int(index[k]), int(status[k]), int(want_status[k])) for k in bad[:8]])
    assert put.failed() == int((want_status < 0).sum()), (what, "failed", put.failed(), int((want_status < 0).sum()))
    off, cb = put.offsets(), put.results()
    assert off[0] == 0 and len(off) == len(chunks) + 1
    at = 0
    for i, c in enumerate(chunks):
        assert off[i] == at, (what, "offsets", i, off)
        if want_rew[i] == 1:      # its size is the library's to choose; the header must say it
            size = cb[i] if cb[i] else None
        else:
            size = header(c)["cbytes"]
        if at + (size if size is not None else 0) <= cap and size is not None:
            got = dest[at:at + size]
            assert cb[i] == size, (what, "cbytes_out", i, cb[i], size)
            if want_rew[i] == 1:
                h = header(got)
                assert h["cbytes"] == size and h["nbytes"] == want_plain[i].size and size <= want_plain[i].size + 16, (what, "header", i, h)
                r, back = orc_decompress(oracle, got, h["nbytes"])
                assert r == h["nbytes"], (what, "the oracle cannot read chunk", i, r)
                if not np.array_equal(np.asarray(back[:r], np.uint8), want_plain[i]):
                    d = np.flatnonzero(np.asarray(back[:r], np.uint8) != want_plain[i])
                    raise AssertionError((what, "chunk", i, "differs in", int(d.size), "bytes, first at", int(d[0]), "row", int(d[0]) // row_bytes))
            else:
                assert np.array_equal(got, np.asarray(c[:size], np.uint8)), (what, "carried-over chunk", i, "differs")
            nxt = -(-(at + size) // align) * align
            assert np.all(dest[at + size:min(nxt, cap)] == 0), (what, "padding behind chunk", i)
            at = nxt
        else:      # the chunk ends behind destsize: nothing of it is written, the table still says where the next one would begin
            assert cb[i] == 0, (what, "cbytes_out behind the cut", i, cb[i])
            assert size is None or np.all(dest[min(at, cap):] == SENTINEL), (what, "bytes behind the cut were written", i)
            if size is None:
                return dest, put, want_plain      # (a rewritten chunk's size is unknown to the test: the rest of the table cannot be checked)
            at = -(-(at + size) // align) * align
    assert off[len(chunks)] == at, (what, "offsets", off, at)
    assert np.all(dest[min(at, cap):] == SENTINEL), (what, "bytes behind the last chunk were written")
    return dest, put, want_plain


def check_census_failure(pkgmod, lib, mem, source, chunks, row_bytes, params, want_rows, align=1, dest_over=None, what=""):
    """a call that fails the census: a negative answer, the chunks' rows and codes in chunk_rows_out, and dest, offsets_out, cbytes_out, status and
    failed_out untouched"""
    index = np.array([0, 1, 2], np.int64)
    rows = new_rows(3, row_bytes)
    rc, dest, status, put = run_put(pkgmod, lib, mem, source, chunks, row_bytes, index, rows, params, align)
    assert rc < 0 and (want_rows is None or put.chunk_rows() == want_rows), (what, rc, put.chunk_rows(), want_rows)
    assert np.all(dest == SENTINEL) and np.all(status == STATUS_SENTINEL) and put.failed() == 0, (what, "something was written")
    assert put.offsets() == [0] * (len(chunks) + 1) and put.results() == [0] * len(chunks) and put.rewritten() == [0] * len(chunks), (what, "a host table was written")
