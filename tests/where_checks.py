"""What tests/test_gpu_where.py (device) and tests/test_emu_where.py (wavefront emulator) both assert about the calls of
include/blosc_gpu_where.h, and the cases they run.  Expected answers never come from the library under test: the plaintext of every chunk is
the oracle's orc_decompress, the expected table is numpy.nonzero of the numpy comparison on the field view of that plaintext (bfloat16 as
(uint16 << 16).view(float32)), and a damaged chunk's code is the oracle's orc_decompress answer.  `mem` is getitem_ranges_checks' NumpyMem /
TorchMem: how a test reaches "device" memory.

The tables are made here: bytes every codec compresses, the field of every row overwritten with a pattern from a small value set, so that
every constant of the set has matches and the densities are known.  Two kinds of table go through whole value spaces instead: table16 holds
every 16-bit pattern once, asked about the constants at which a format changes regime (constants16), and the 4- and 8-byte kinds are drawn
from neighbour_set - the patterns around 2^31, 2^32 and 2^63, the regime changes of binary32 and binary64, halves of 8-byte values."""
import ctypes as C
import operator

import numpy as np

from getitem_ranges_checks import plain
from helpers import header, orc_compress, orc_decompress
from take_checks import MEMCPYED_BYTES, N, TakeSource, chunk_rows, pack_container, plaintext  # noqa: F401  (re-exported to the test files)

UINT, INT, FLOAT, BFLOAT16 = range(4)
OPS = [operator.eq, operator.ne, operator.lt, operator.le, operator.gt, operator.ge]      # BLOSC_GPU_WHERE_EQ ... _GE
KINDS = [(UINT, 1), (UINT, 2), (UINT, 4), (UINT, 8), (INT, 1), (INT, 2), (INT, 4), (INT, 8), (FLOAT, 2), (FLOAT, 4), (FLOAT, 8), (BFLOAT16, 2)]
SENTINEL = 0xA5
WORD_SENTINEL = np.int64(-0x5A5A5A5A5A5A5A5B)      # 0xA5A5A5A5A5A5A5A5
INT_SENTINEL, SIZE_SENTINEL = -7777, 777777
GUARD = 8                                          # sentinel words in front of and behind index_out
# (row_bytes, offset, kind, bytes): a plain column; an unaligned field; an odd row size; the field in a row's last bytes; rows that cross block
# boundaries; a row over three or four blocks with the field at its end
LAYOUTS = [(4, 0, FLOAT, 4), (12, 5, UINT, 4), (17, 9, INT, 8), (96, 88, FLOAT, 8), (4080, 1021, BFLOAT16, 2), (20400, 20392, UINT, 8)]


def kind_name(kind, nbytes):
    return f"{('uint', 'int', 'float', 'bfloat')[kind]}{8 * nbytes}"


def value_set(kind, nbytes):
    """the bit patterns (unsigned, nbytes wide) the fields and the constants are drawn from.  Integers: min, -1 or max, 0, 1, a mid value;
    floating point: two NaNs, +0, -0, +inf, -inf, the smallest subnormal, +1.5, -1.5"""
    bits = 8 * nbytes
    top = (1 << bits) - 1
    if kind == UINT:
        return [0, top, 1, 0x35 * (top // 0xff)]
    if kind == INT:
        return [1 << (bits - 1), top, 0, 1, (0x35 * (top // 0xff)) >> 1]
    # +inf, a quiet NaN, +1.5
    exp, quiet, sig = {(FLOAT, 2): (0x7c00, 0x7e00, 0x3e00), (BFLOAT16, 2): (0x7f80, 0x7fc0, 0x3fc0), (FLOAT, 4): (0x7f800000, 0x7fc00000, 0x3fc00000),
                       (FLOAT, 8): (0x7ff0 << 48, 0x7ff8 << 48, 0x3ff8 << 48)}[(kind, nbytes)]
    sign = 1 << (bits - 1)
    return [quiet, sign | exp | 1, 0, sign, exp, sign | exp, 1, sig, sign | sig]


MANTISSA = {(FLOAT, 2): 10, (BFLOAT16, 2): 7, (FLOAT, 4): 23, (FLOAT, 8): 52}      # the mantissa bits of the floating-point formats


def regime(kind, nbytes):
    """the magnitudes at which a floating-point format changes regime, by name: zero, the smallest and the largest subnormal, the smallest
    normal, 1.0, the largest finite value, infinity, the first pattern above it (a NaN) and a quiet NaN"""
    mant, bits = MANTISSA[(kind, nbytes)], 8 * nbytes
    inf = ((1 << (bits - 1 - mant)) - 1) << mant
    return {"zero": 0, "min_sub": 1, "max_sub": (1 << mant) - 1, "min_normal": 1 << mant, "one": ((1 << (bits - 2 - mant)) - 1) << mant,
            "max_finite": inf - 1, "inf": inf, "first_nan": inf + 1, "quiet_nan": inf | (1 << (mant - 1))}


def regime_set(kind, nbytes):
    """every magnitude of regime() with both signs, and one quiet NaN: 17 patterns"""
    r, sign = regime(kind, nbytes), 1 << (8 * nbytes - 1)
    mags = [r[k] for k in ("zero", "min_sub", "max_sub", "min_normal", "one", "max_finite", "inf", "first_nan")]
    return [s | m for m in mags for s in (0, sign)] + [r["quiet_nan"]]


CARRIES16 = [0, 1, 0x00ff, 0x0100, 0x7fff, 0x8000, 0x8001, 0xfffe, 0xffff]      # the byte carry of a two-byte load, and the sign change
KINDS16 = [(UINT, 2), (INT, 2), (FLOAT, 2), (BFLOAT16, 2)]
NEIGHBOUR_KINDS = [(UINT, 4), (UINT, 8), (INT, 4), (INT, 8), (FLOAT, 4), (FLOAT, 8)]
# binary64: two patterns that differ only in the low word - in the order a signed low word would reverse - and two that differ only in the high word
LOW_PAIR = [(0x400921fb << 32) | 0x00000001, (0x400921fb << 32) | 0xfffffffe]
HIGH_PAIR = [(0x3ff00000 << 32) | 0x80000000, (0x3ff00001 << 32) | 0x80000000]


def constants16(kind):
    """the constants the table of every 16-bit pattern is asked about"""
    return CARRIES16 if kind in (UINT, INT) else regime_set(kind, 2)


def thin_constants16(kind):
    """the emulator's four, each on a regime change"""
    if kind in (UINT, INT): return [0x00ff, 0x0100, 0x7fff, 0x8000]
    r = regime(kind, 2)
    return [r["max_sub"], 0x8000 | r["min_normal"], r["inf"], 0x8000 | r["first_nan"]]


def neighbour_set(kind, nbytes):
    """the patterns of the 4- and 8-byte kinds next to which an order can go wrong.  Integers: 0, 1 and the neighbours of 2^31, 2^32 and 2^63 -
    where a sign bit, a half of a composed load or the key's bit 63 changes; floating point: regime_set, and for binary64 LOW_PAIR and HIGH_PAIR"""
    if kind in (UINT, INT):
        small = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]
        return small if nbytes == 4 else small + [2 ** 32, 2 ** 32 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 1]
    return regime_set(kind, nbytes) + (LOW_PAIR + HIGH_PAIR if nbytes == 8 else [])


def thin_neighbour_picks(kind, nbytes):
    """the emulator's (op, constant) pairs on a neighbour set, as many as thin_picks has: the integers across 2^31 (and 2^32, 2^63), the
    floating-point formats across subnormal / normal and finite / infinity / NaN (binary64: inside the two pairs)"""
    if kind in (UINT, INT):
        return [(2, 2 ** 31), (5, 2 ** 32 - 1)] + ([(4, 2 ** 63 - 1), (3, 2 ** 32)] if nbytes == 8 else [])
    r, sign = regime(kind, nbytes), 1 << (8 * nbytes - 1)
    if nbytes == 8:
        return [(2, LOW_PAIR[1]), (4, HIGH_PAIR[0]), (5, sign | r["max_sub"]), (3, r["max_finite"])]
    return [(2, r["min_normal"]), (5, sign | r["max_sub"]), (4, r["max_finite"]), (1, r["first_nan"])]


def comparable(patterns, kind, nbytes):
    """unsigned patterns -> the numpy array the comparison runs on"""
    u = np.ascontiguousarray(patterns, dtype=f"<u{nbytes}")
    if kind == UINT: return u
    if kind == INT: return u.view(f"<i{nbytes}")
    if kind == FLOAT: return u.view(f"<f{nbytes}")
    return (u.astype(np.uint32) << 16).view(np.float32)


def field_of(rows_plain, row_bytes, offset, kind, nbytes):
    nrows = rows_plain.size // row_bytes
    raw = np.ascontiguousarray(rows_plain[:nrows * row_bytes].reshape(nrows, row_bytes)[:, offset:offset + nbytes])
    return comparable(raw.view(f"<u{nbytes}").ravel(), kind, nbytes)


def expected(rows_plain, row_bytes, offset, kind, nbytes, op, constant, dead=()):
    """numpy's table: the rows whose field `op` the constant (a pattern), without the rows [lo, hi) of `dead` - chunks that do not decode"""
    with np.errstate(invalid="ignore"):
        hit = OPS[op](field_of(rows_plain, row_bytes, offset, kind, nbytes), comparable([constant], kind, nbytes)[0])
    for lo, hi in dead:
        hit[lo:hi] = False
    return np.nonzero(hit)[0].astype(np.int64)


def make_table(nrows, row_bytes, offset, nbytes, patterns, seed=21, noise=False):
    """nrows rows: bytes every codec compresses - short rows repeat every seven rows, long ones are getitem_ranges_checks.plain's, both with a
    little noise - or (noise) random ones, for a chunk that has to come out MEMCPYED; the field of row r is overwritten by patterns[r] (an
    unsigned array; None: the row keeps its bytes)"""
    rng = np.random.default_rng(seed)
    n = nrows * row_bytes
    if noise: base = rng.integers(0, 256, n, dtype=np.uint8)
    elif row_bytes > 96: base = plain(n, seed=seed)
    else:
        base = np.resize(rng.integers(0, 256, 7 * row_bytes, dtype=np.uint8), n).copy()
        if n: base[rng.integers(0, n, n // 97)] ^= 1
    tab = base.reshape(nrows, row_bytes)
    if patterns is not None:
        tab[:, offset:offset + nbytes] = np.ascontiguousarray(patterns, dtype=f"<u{nbytes}").view(np.uint8).reshape(nrows, nbytes)
    return tab.reshape(-1)


def drawn(values, nrows, seed=4):
    """a pattern per row from `values`: a sequence of period 997 with one row in forty drawn anew - every value has rows, and the codecs have matches"""
    rng = np.random.default_rng(seed)
    v = np.array(values, dtype=np.uint64)
    pick = np.resize(rng.integers(0, v.size, 997), nrows)
    anew = rng.integers(0, nrows, max(nrows // 40, 1))
    pick[anew] = rng.integers(0, v.size, anew.size)
    return v[pick]


def total_rows(row_bytes, scale=1):
    """the rows of where_chunks' call"""
    n = N * scale
    return (n + (n // 2 if (n // 2) % row_bytes == 0 else 0) + (MEMCPYED_BYTES if MEMCPYED_BYTES % row_bytes == 0 else 0)) // row_bytes


def where_chunks(oracle, write, row_bytes, offset, nbytes, patterns_for, scale=1, memcpyed_step=4):
    """The chunks of one call - take_checks.batch_chunks' shape with a table of our own in it: N * scale bytes, a chunk of nbytes 0 in the
    middle, N * scale / 2 where row_bytes divides it, a MEMCPYED chunk of random rows with the field set in one row of memcpyed_step (not for
    20 400).  patterns_for(first_row, nrows) -> the unsigned patterns of these rows; write(k, data) -> chunk k of the compressible ones"""
    n = N * scale
    sizes = [n, 0] + ([n // 2] if (n // 2) % row_bytes == 0 else [])
    out, first = [], 0
    for k, size in enumerate(sizes):
        rows = size // row_bytes
        out.append(write(k, make_table(rows, row_bytes, offset, nbytes, patterns_for(first, rows), seed=21 + k)) if size
                   else orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += rows
    if MEMCPYED_BYTES % row_bytes == 0:
        rows = MEMCPYED_BYTES // row_bytes
        data = make_table(rows, row_bytes, offset, nbytes, None, seed=3, noise=True).reshape(rows, row_bytes)
        pat = np.ascontiguousarray(patterns_for(first, rows), dtype=f"<u{nbytes}").view(np.uint8).reshape(rows, nbytes)
        data[::memcpyed_step, offset:offset + nbytes] = pat[::memcpyed_step]
        out.append(orc_compress(oracle, data.reshape(-1), 4, 5, 1, "lz4")[1])
        assert header(out[-1])["flags"] & 2
    assert header(out[1])["nbytes"] == 0 and all(header(c)["nbytes"] % row_bytes == 0 for c in out)
    return out


def predicate(pkgmod, kind, nbytes, op, constant, offset):
    return pkgmod.predicate(kind, nbytes, op, int(constant).to_bytes(nbytes, "little"), offset=offset)


class Outputs:
    """the host outputs of one call, filled with sentinels"""
    def __init__(self, nchunks):
        self.n = nchunks
        self.total, self.unread = C.c_size_t(SIZE_SENTINEL), C.c_size_t(SIZE_SENTINEL)
        self.matches = (C.c_int * max(nchunks, 1))(*[INT_SENTINEL] * max(nchunks, 1))
        self.rows = (C.c_int * max(nchunks, 1))(*[INT_SENTINEL] * max(nchunks, 1))

    def untouched(self, rows_too=False):
        return (self.total.value == SIZE_SENTINEL and self.unread.value == SIZE_SENTINEL and all(m == INT_SENTINEL for m in self.matches)
                and (not rows_too or all(r == INT_SENTINEL for r in self.rows)))


def raw_call(lib, source, row_bytes, pred, index_ptr, capacity, out, stream=None):
    """blosc_gpu_where_batch or _packed, as `source` (a take_checks.TakeSource) says"""
    if source.packed:
        return lib.blosc_gpu_where_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, C.byref(pred), index_ptr,
                                          capacity, C.byref(out.total), out.matches, out.rows, C.byref(out.unread), stream)
    return lib.blosc_gpu_where_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, C.byref(pred), index_ptr, capacity, C.byref(out.total),
                                     out.matches, out.rows, C.byref(out.unread), stream)


def nchunks_of(source):
    return len(source.offsets) - 1 if source.packed else len(source.ptrs)


def run_where(lib, mem, source, row_bytes, pred, capacity, null_table=False, stream=None):
    """One call.  index_out lies between GUARD sentinel words inside a buffer of sentinels (null_table: NULL, for capacity 0).
    Returns (answer, all `capacity` words of the table, Outputs); the words around the table are asserted here"""
    out = Outputs(nchunks_of(source))
    buf, base = mem.filled(8 * (capacity + 2 * GUARD), SENTINEL)
    assert base % 8 == 0
    rc = raw_call(lib, source, row_bytes, pred, None if null_table else base + 8 * GUARD, capacity, out, stream)
    words = np.ascontiguousarray(mem.get(buf)[:8 * (capacity + 2 * GUARD)]).view(np.int64)
    assert np.all(words[:GUARD] == WORD_SENTINEL) and np.all(words[GUARD + capacity:] == WORD_SENTINEL), "words outside index_out were written"
    return rc, words[GUARD:GUARD + capacity].copy(), out


def check_where(lib, mem, source, chunks, rows_plain, row_bytes, pred_args, pkgmod, capacity=None, dead=(), codes=None, stream=None, what="", keep=None):
    """one call against numpy: the answer 0, the prefix of the table exact and ascending, every word from min(total, capacity) on untouched, the
    total, the per-chunk counts (codes: {chunk: the decoder's answer} for the chunks of `dead`), the rows and the unread rows.
    capacity None: the total + 5.  Returns numpy's table.  keep: a dict that receives what the call gave (the whole table, the total, the
    per-chunk counts, the rows, unread), for callers that compare two calls"""
    offset, kind, nbytes, op, constant = pred_args
    want = expected(rows_plain, row_bytes, offset, kind, nbytes, op, constant, dead)
    cap = want.size + 5 if capacity is None else capacity
    rc, table, out = run_where(lib, mem, source, row_bytes, predicate(pkgmod, kind, nbytes, op, constant, offset), cap, null_table=(capacity == 0),
                               stream=stream)
    if keep is not None:
        keep.update(table=table, total=np.array([out.total.value, out.unread.value], np.uint64), matches=np.array(list(out.matches)[:out.n], np.int64),
                    chunk_rows=np.array(list(out.rows)[:out.n], np.int64))
    what = (what, "row_bytes", row_bytes, "offset", offset, kind_name(kind, nbytes), OPS[op].__name__, hex(constant), "capacity", cap)
    assert rc == 0, (what, rc)
    rows = chunk_rows(chunks, row_bytes)
    assert list(out.rows)[:out.n] == rows, (what, list(out.rows))
    assert out.total.value == want.size, (what, "total", out.total.value, want.size)
    first = np.concatenate([[0], np.cumsum(rows)])
    per_chunk = [int(((want >= first[k]) & (want < first[k + 1])).sum()) for k in range(len(rows))]
    for k, code in (codes or {}).items():
        per_chunk[k] = code
    assert list(out.matches)[:out.n] == per_chunk, (what, "chunk matches", list(out.matches), per_chunk)
    assert out.unread.value == sum(hi - lo for lo, hi in dead), (what, "unread", out.unread.value)
    m = min(want.size, cap)
    if not np.array_equal(table[:m], want[:m]):
        k = int(np.flatnonzero(table[:m] != want[:m])[0])
        raise AssertionError((what, "entry", k, int(table[k]), int(want[k]), int((table[:m] != want[:m]).sum())))
    assert np.all(table[m:] == WORD_SENTINEL), (what, "words behind min(total, capacity) were written")
    assert m < 2 or np.all(np.diff(table[:m]) > 0), (what, "not ascending")
    return want


def check_failure(lib, mem, source, row_bytes, pred, want_rows, what=""):
    """a call that is refused: a negative answer; index_out, total, chunk matches and unread keep their sentinels; chunk_rows_out holds want_rows
    (None: it is untouched as well)"""
    rc, table, out = run_where(lib, mem, source, row_bytes, pred, 16)
    assert rc < 0, (what, rc)
    assert np.all(table == WORD_SENTINEL) and out.untouched(rows_too=want_rows is None), (what, "something was written")
    if want_rows is not None:
        assert list(out.rows)[:out.n] == want_rows, (what, list(out.rows), want_rows)
    rc, _, out = run_where(lib, mem, source, row_bytes, pred, 0, null_table=True)
    assert rc < 0 and out.untouched(rows_too=want_rows is None), (what, "the count alone", rc)


def density_patterns(name, nrows, firsts, hit, miss):
    """the field of every row for one density case, `hit` where the row is to match (EQ hit) and `miss` elsewhere"""
    p = np.full(nrows, miss, np.uint64)
    if name == "none": pass
    elif name == "every": p[:] = hit
    elif name == "one in sixteen": p[np.random.default_rng(8).random(nrows) < 1 / 16] = hit
    elif name == "row 0": p[0] = hit
    elif name == "last row": p[nrows - 1] = hit
    elif name == "chunk edges":
        for f in firsts[1:-1]:
            p[[r for r in (f - 1, f) if 0 <= r < nrows]] = hit
    else: raise ValueError(name)
    return p


DENSITIES = ["none", "every", "one in sixteen", "row 0", "last row", "chunk edges"]


def decoder_code(oracle, bad):
    """what blosc_decompress answers for a damaged chunk: the oracle's orc_decompress"""
    code, _ = orc_decompress(oracle, bad, header(bad)["nbytes"])
    assert code < 0, "the oracle reads the damaged chunk"
    return code


# ---- the cases: env has pkg (the loader module), lib, mem, oracle and writer(cname, T, shuffle, turn) -> write(k, data) ----
class Env:
    def __init__(self, pkg, lib, mem, oracle, writer):
        self.pkg, self.lib, self.mem, self.oracle, self.writer = pkg, lib, mem, oracle, writer
        pkg.declare_where(lib)


def table_call(env, setting, layout, patterns, turn=0, memcpyed_step=4):
    """(chunks, their plaintext by the oracle) of one call whose rows carry `patterns` in the layout's field"""
    cname, T, shuffle, scale = setting
    row_bytes, offset, _, nbytes = layout
    assert patterns.size == total_rows(row_bytes, scale)
    chunks = where_chunks(env.oracle, env.writer(cname, T, shuffle, turn), row_bytes, offset, nbytes, lambda f, n: patterns[f:f + n], scale, memcpyed_step)
    assert not header(chunks[0])["flags"] & 2, "the table's first chunk came out MEMCPYED"
    return chunks, plaintext(env.oracle, chunks)


def both_sources(env, chunks):
    return TakeSource(env.mem, chunks=chunks), TakeSource(env.mem, *(None,) + pack_container(chunks))


def case_kind(env, kind, nbytes, setting, picks, turn=0):
    """case 1: a field of this kind and width at offset 3 of rows of 17 bytes, drawn from its value set; picks: the (op, constant) pairs to run"""
    layout = (17, 3, kind, nbytes)
    values = value_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, layout, drawn(values, total_rows(17, setting[3])), turn)
    src = TakeSource(env.mem, chunks=chunks)
    for op, constant in picks(values):
        want = check_where(env.lib, env.mem, src, chunks, rows_plain, 17, (3, kind, nbytes, op, constant), env.pkg, what=setting)
        if kind in (FLOAT, BFLOAT16) and constant in values[:2]:      # a NaN constant: nothing, or with NE every row
            assert want.size == (rows_plain.size // 17 if op == 1 else 0)


def case_neighbours(env, kind, nbytes, setting, picks=None, turn=0):
    """case 1 on the kind's neighbour set: the table drawn from it, every op against every constant of it (picks: the (op, constant) pairs
    of a thinner run)"""
    values = neighbour_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, (17, 3, kind, nbytes), drawn(values, total_rows(17, setting[3]), seed=6), turn)
    src = TakeSource(env.mem, chunks=chunks)
    for op, constant in (all_picks(values) if picks is None else picks):
        assert constant in values
        check_where(env.lib, env.mem, src, chunks, rows_plain, 17, (3, kind, nbytes, op, constant), env.pkg, what=("neighbours", setting))


ROWS16 = [30001, 20003, 15532]      # the 65 536 rows of table16 in three chunks, none a multiple of a tile's 1 024 rows
LAYOUTS16 = [(2, 0), (5, 3)]        # (row_bytes, offset): the field is the row; the field at an odd address in every row


def table16(env, row_layout, turn=0):
    """(chunks, their plaintext) of a table whose two-byte field takes each of the 65 536 patterns exactly once, in a seeded permutation"""
    row_bytes, offset = row_layout
    patterns = np.random.default_rng(16).permutation(1 << 16).astype(np.uint64)
    write = env.writer("lz4" if row_bytes == 2 else "blosclz", row_bytes, 1, turn)
    assert sum(ROWS16) == 1 << 16 and all(r % 1024 for r in ROWS16)
    chunks = [write(k, make_table(rows, row_bytes, offset, 2, patterns[sum(ROWS16[:k]):sum(ROWS16[:k + 1])], seed=90 + k)) for k, rows in enumerate(ROWS16)]
    rows_plain = plaintext(env.oracle, chunks)
    assert np.array_equal(np.sort(field_of(rows_plain, row_bytes, offset, UINT, 2)), np.arange(1 << 16)), "not every pattern once"
    return chunks, rows_plain


def case_patterns16(env, kind, row_layout, constants, ops=range(6), packed_ops=(0, 2, 4), turn=0):
    """every 16-bit pattern as a row against each constant: the ops through blosc_gpu_where_batch, packed_ops through _packed as well"""
    row_bytes, offset = row_layout
    chunks, rows_plain = table16(env, row_layout, turn)
    batch, packed = both_sources(env, chunks)
    for constant in constants:
        for op in ops:
            args = (offset, kind, 2, op, constant)
            a = check_where(env.lib, env.mem, batch, chunks, rows_plain, row_bytes, args, env.pkg, what="every pattern, batch")
            if op == 0:      # EQ: the pattern itself - both zeros of a floating-point format, no row for a NaN
                is_float = kind in (FLOAT, BFLOAT16)
                mag = constant & 0x7fff
                assert a.size == (1 if not is_float else 0 if mag > regime(kind, 2)["inf"] else 2 if mag == 0 else 1), (kind_name(kind, 2), hex(constant), a.size)
            if op in packed_ops:
                b = check_where(env.lib, env.mem, packed, chunks, rows_plain, row_bytes, args, env.pkg, what="every pattern, packed")
                assert np.array_equal(a, b)


def all_picks(values):
    return [(op, c) for op in range(6) for c in values]


def thin_picks(values):
    """the emulator's: two ops on the integers; on the floating-point sets EQ against -0, NE and LE against a NaN, GE against the
    subnormal - the other ops run on the row layouts"""
    if len(values) > 5:
        return [(0, values[3]), (1, values[0]), (3, values[1]), (5, values[6])]
    return [(2, values[2]), (4, values[0])]


def case_layout(env, layout, setting, turn=0, stream=None, ops=range(6), packed_ops=(0, 2, 4)):
    """cases 2 and 9: the ops on one row layout (packed_ops: through both entry points, which give the same)"""
    row_bytes, offset, kind, nbytes = layout
    values = value_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, layout, drawn(values, total_rows(row_bytes, setting[3])), turn)
    batch, packed = both_sources(env, chunks)
    for op in ops:
        args = (offset, kind, nbytes, op, values[(op + 3) % len(values)])
        a = check_where(env.lib, env.mem, batch, chunks, rows_plain, row_bytes, args, env.pkg, stream=stream, what=("batch", setting))
        if op in packed_ops:
            b = check_where(env.lib, env.mem, packed, chunks, rows_plain, row_bytes, args, env.pkg, stream=stream, what=("packed", setting))
            assert np.array_equal(a, b)


def case_density(env, name, setting, turn=0):
    """case 3: EQ on a 32-bit field at offset 5 of rows of 12 bytes that holds `hit` in the rows of the case and `miss` elsewhere"""
    layout, hit, miss = (12, 5, UINT, 4), 0xDEADBEEF, 0x01020304
    nrows = total_rows(12, setting[3])
    n = N * setting[3]
    firsts = np.cumsum([0, n // 12, 0, n // 2 // 12, MEMCPYED_BYTES // 12])
    assert firsts[-1] == nrows
    chunks, rows_plain = table_call(env, setting, layout, density_patterns(name, nrows, firsts, hit, miss), turn, memcpyed_step=1)
    src = TakeSource(env.mem, chunks=chunks)
    want = check_where(env.lib, env.mem, src, chunks, rows_plain, 12, (5, UINT, 4, 0, hit), env.pkg, what=name)
    count = {"none": 0, "every": nrows, "row 0": 1, "last row": 1, "chunk edges": 2 * 2}.get(name)      # (the boundary at the empty chunk is one boundary)
    assert count is None or want.size == count, (name, want.size)
    assert name != "one in sixteen" or abs(want.size - nrows / 16) < nrows / 64
    if name in ("one in sixteen", "chunk edges"):
        check_where(env.lib, env.mem, src, chunks, rows_plain, 12, (5, UINT, 4, 1, hit), env.pkg, what=(name, "complement"))


def case_many_tiles(env, thin=False):
    """case 4: 320 000 rows of one byte in four chunks - hundreds of tiles whatever the tile size, chunk ends inside tiles"""
    sizes = [120001, 0, 119999, 80000]
    pats = drawn(value_set(UINT, 1), sum(sizes), seed=9)
    write = env.writer("lz4", 4, 1, 0)
    chunks, first = [], 0
    for k, size in enumerate(sizes):
        chunks.append(write(0, make_table(size, 1, 0, 1, pats[first:first + size])) if size else orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += size
    rows_plain = plaintext(env.oracle, chunks)
    src = TakeSource(env.mem, chunks=chunks)
    want = check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 0, 1), env.pkg, what="many tiles")
    assert sum(sizes) // 5 < want.size < sum(sizes) // 3
    if not thin:
        check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 5, 0x35), env.pkg, capacity=100000, what="many tiles, cut")


TILE_ROWS, SCAN_THREADS = 1024, 1024      # k_where.hip's WH_TILE and WH_SCAN_THREADS: thread i of k_where_scan owns `per` tiles from i * per
# rows per chunk, one byte each: 1024 tiles (per = 1, every scan thread busy); 1025 (per = 2: thread 512 owns one tile, 513 ... 1023 none);
# 1465 + 586 tiles in one pass (per = 3: the chunk boundary lies inside thread 488's stretch)
WIDE = {"1024 tiles": [1024 * 1024], "1025 tiles": [1024 * 1024 + 1], "two chunks": [1500000, 600001]}


def tiles_of_pass(rows):
    """(the pass's tile number of every row, the number of tiles): tiles of 1024 rows that never straddle a chunk"""
    per_chunk = [-(-r // TILE_ROWS) for r in rows]
    first = np.concatenate([[0], np.cumsum(per_chunk)])
    return np.concatenate([first[k] + np.arange(r) // TILE_ROWS for k, r in enumerate(rows)]), int(first[-1])


def wide_patterns(rows, hit, miss):
    """density_patterns' one row in sixteen, then whole tiles without a match: with per = 3 the middle tile of every scan thread's stretch, so
    that the tiles either side of every boundary between two threads hold matches; with per <= 2 every tile lies at such a boundary, and one
    tile in eight is emptied.  The first and the last tile keep their matches, in the first and the last row.  Returns (patterns, the matches
    of every tile)"""
    nrows = sum(rows)
    tile, ntiles = tiles_of_pass(rows)
    per = -(-ntiles // SCAN_THREADS)
    p = density_patterns("one in sixteen", nrows, None, hit, miss)
    none = (tile % 3 == 1) if per == 3 else (tile % 8 == 5)
    p[none & (tile != 0) & (tile != ntiles - 1)] = miss
    p[0] = p[nrows - 1] = hit
    counts = np.bincount(tile, weights=(p == hit), minlength=ntiles).astype(np.int64)
    assert counts[0] and counts[-1] and (counts == 0).any()
    if per == 3:
        assert np.all(counts[np.arange(ntiles) % 3 != 1] > 0), "a tile next to a boundary between two scan threads holds no match"
    return p, counts


def case_wide_pass(env, name, thin=False):
    """more than 1024 tiles in one pass: a thread of k_where_scan owns two or three tiles, and the threads behind the last tile own none.
    EQ on one-byte rows; the table with room for every match, and cut inside a tile that a high-numbered thread owns"""
    rows = WIDE[name]
    p, counts = wide_patterns(rows, 1, 0)
    ntiles = counts.size
    assert -(-ntiles // SCAN_THREADS) == {"1024 tiles": 1, "1025 tiles": 2, "two chunks": 3}[name]
    write = env.writer("lz4", 4, 1, 0)
    chunks, first = [], 0
    for k, n in enumerate(rows):
        chunks.append(write(k, make_table(n, 1, 0, 1, p[first:first + n])))
        first += n
    rows_plain = plaintext(env.oracle, chunks)
    src = TakeSource(env.mem, chunks=chunks)
    want = check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 0, 1), env.pkg, what=("wide pass", name))
    assert want.size == counts.sum()
    if thin: return
    t = max(t for t in range(ntiles - 1) if counts[t] >= 2)      # the last full tile with matches: the highest thread that owns tiles owns it
    cut = int(counts[:t].sum() + counts[t] // 2)
    assert t >= ntiles - 4 and counts[:t].sum() < cut < counts[:t + 1].sum()
    check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 0, 1), env.pkg, capacity=cut, what=("wide pass, cut", name))


def case_many_chunks(env, chunks, pass_bytes=(0, 16 << 10), thin=False):
    """take_checks.many_chunks as one-byte rows: more than 1024 tiles with another chunk for nearly every tile, under the default pass bound
    and under 16 KiB - dozens of passes, the running total carried on the device across all of them"""
    rows = chunk_rows(chunks, 1)
    assert sum(-(-r // TILE_ROWS) for r in rows) > SCAN_THREADS and len(chunks) > 1024
    rows_plain = plaintext(env.oracle, chunks)
    constant = int(np.bincount(rows_plain, minlength=256).argmax())
    src = TakeSource(env.mem, chunks=chunks)
    for bound in pass_bytes:
        env.lib.blosc_amd_getitem_pass_bytes(bound)
        try:
            assert rows_plain.size > 30 * bound
            want = check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 0, constant), env.pkg, what=("many chunks", bound))
            if not thin:
                check_where(env.lib, env.mem, src, chunks, rows_plain, 1, (0, UINT, 1, 1, constant), env.pkg, capacity=rows_plain.size // 2, what=("many chunks, cut", bound))
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)
        assert 100 < want.size < rows_plain.size // 2


def case_capacity(env, setting, turn=0):
    """case 5: capacity 0 with a NULL table, total - 1, total, total + 7 - the prefix exact, the rest untouched, the counts the same in all four"""
    layout = (12, 5, INT, 4)
    values = value_set(INT, 4)
    chunks, rows_plain = table_call(env, setting, layout, drawn(values, total_rows(12, setting[3])), turn)
    total = expected(rows_plain, 12, 5, INT, 4, 3, values[3]).size
    assert total > 8
    for n, src in enumerate(both_sources(env, chunks)):
        for cap in (0, total - 1, total, total + 7)[:4 if n == 0 else 2]:
            check_where(env.lib, env.mem, src, chunks, rows_plain, 12, (5, INT, 4, 3, values[3]), env.pkg, capacity=cap, what="capacity")


def case_passes(env, setting, layout, turn=0):
    """case 6: under a pass bound of 16 KiB every chunk is a pass of its own; the table and the counts are those of the default bound"""
    row_bytes, offset, kind, nbytes = layout
    values = value_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, layout, drawn(values, total_rows(row_bytes, setting[3])), turn)
    args = (offset, kind, nbytes, 4, values[2])
    for src in both_sources(env, chunks):
        one = check_where(env.lib, env.mem, src, chunks, rows_plain, row_bytes, args, env.pkg, what="default bound")
        env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            many = check_where(env.lib, env.mem, src, chunks, rows_plain, row_bytes, args, env.pkg, what="16 KiB passes")
            check_where(env.lib, env.mem, src, chunks, rows_plain, row_bytes, args, env.pkg, capacity=one.size // 2, what="16 KiB passes, cut")
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)
        assert np.array_equal(one, many) and one.size > 0


def case_damage(env, chunk_of, what="", thin=False):
    """case 7: a chunk that does not decode between two that do.  chunk_of(data) -> a typesize-17 chunk of several blocks"""
    from getitem_ranges_checks import pick_damage
    layout = (17, 3, INT, 4)
    values = value_set(INT, 4)
    rows = N // 17
    good = [chunk_of(make_table(rows, 17, 3, 4, drawn(values, rows, seed=30 + k), seed=40 + k)) for k in range(3)]
    rows_plain = plaintext(env.oracle, good)
    found, _ = pick_damage(env.oracle, good[1])
    for kind, bad in found[:1 if thin else None]:
        chunks = [good[0], bad, good[2]]
        code = decoder_code(env.oracle, bad)
        for src in both_sources(env, chunks):
            for op, constant in ((1, values[2]), (0, values[4]))[:1 if src.packed else 2]:
                want = check_where(env.lib, env.mem, src, chunks, rows_plain, 17, (3, INT, 4, op, constant), env.pkg, dead=[(rows, 2 * rows)], codes={1: code},
                                   what=(what, kind))
                assert (want < rows).any() and (want >= 2 * rows).any() and not ((want >= rows) & (want < 2 * rows)).any()


def case_refused(env):
    """case 8: take's three census failures with the code at its place in chunk_rows_out, and an index_out that overlaps the source"""
    good = orc_compress(env.oracle, plain(N), 17, 5, 1, "lz4", blocksize=8192)[1]
    odd = orc_compress(env.oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=8192)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    pred = predicate(env.pkg, UINT, 4, 1, 0, 4)
    mem = env.mem
    check_failure(env.lib, mem, TakeSource(mem, chunks=[good, odd, good]), 16, pred, [rows, -1, rows], "no multiple")
    check_failure(env.lib, mem, TakeSource(mem, chunks=[good, good, version]), 16, pred, [rows, rows, -9], "version")
    check_failure(env.lib, mem, TakeSource(mem, *(None,) + pack_container([version, odd])), 16, pred, [-9, -1], "both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_failure(env.lib, mem, TakeSource(mem, container=np.concatenate(parts), offsets=offs), 16, pred, [rows, -1, rows], "a slot eight bytes short")
    # index_out inside the second chunk; inside the container, in the padding between two chunks
    for src in (TakeSource(mem, chunks=[good, good]), TakeSource(mem, *(None,) + pack_container([good, good], align=4096))):
        before = np.array(mem.get(src.keep[0] if src.packed else src.keep[1][0]), copy=True)
        base = src.container + src.offsets[1] - 64 if src.packed else src.ptrs[1] + 64
        base += (-base) % 8
        for cap in (4, 1):
            out = Outputs(2)
            rc = raw_call(env.lib, src, 16, pred, base, cap, out)
            assert rc < 0 and out.untouched(rows_too=True), ("overlap", src.packed, rc, list(out.rows))
        assert np.array_equal(before, mem.get(src.keep[0] if src.packed else src.keep[1][0])), "the source was written"
