"""What tests/test_gpu_zones.py (device) and tests/test_emu_zones.py (wavefront emulator) both assert about the calls of
include/blosc_gpu_zones.h, the cases they run, and numpy's statement of the prune rule (tests/test_zone_rule_cpu.py holds the library's
against it).

The yardsticks.  blosc_gpu_aggregate_fields_*: every field's total, chunk entries and status against blosc_gpu_aggregate_clauses_* for that
field alone, as bytes; the first and the last field of every call also through clauses_checks.check_aggregate, which holds the clause call
against numpy and aggregate_checks.tree_sum.  The zoned calls: clauses_checks.check_where / check_aggregate - numpy on the oracle's plaintext
- and the bytes they return; chunk_pruned_out against the rule as numpy states it on the plaintext of every chunk."""
import ctypes as C

import numpy as np

import aggregate_checks as A
import clauses_checks as K
import where_checks as W
from clauses_checks import EQ, GE, GT, LE, LT, NE
from helpers import header, orc_compress
from take_checks import BLOCKSIZE, TakeSource, chunk_rows, pack_container, plaintext
from where_checks import BFLOAT16, FLOAT, INT, UINT

SENTINEL = 0xA5


# ---- the rule in numpy ----
def values_of(patterns, kind, nbytes):
    return W.comparable(np.array(patterns, dtype=np.uint64).astype(f"<u{nbytes}"), kind, nbytes)


def is_nan(patterns, kind, nbytes):
    v = values_of(patterns, kind, nbytes)
    return np.isnan(v) if kind in (FLOAT, BFLOAT16) else np.zeros(len(patterns), bool)


def passes(patterns, kind, nbytes, op, constant):
    """numpy's comparison of every value of the chunk with the constant"""
    with np.errstate(invalid="ignore"):
        return np.asarray(W.OPS[op](values_of(patterns, kind, nbytes), values_of([constant], kind, nbytes)[0]))


def table_says(patterns, kind, nbytes, op, constant):
    """the header's table: can the term be true in a chunk of these values (at least one)?"""
    nan = is_nan(patterns, kind, nbytes)
    if is_nan([constant], kind, nbytes)[0] or nan.all():
        return op == NE
    v = values_of(patterns, kind, nbytes)[~nan]
    k, lo, hi = values_of([constant], kind, nbytes)[0], v.min(), v.max()
    return bool({LT: lo < k, LE: lo <= k, GT: hi > k, GE: hi >= k, EQ: lo <= k <= hi, NE: not (lo == k and hi == k and not nan.any())}[op])


def entry_of(pkgmod, patterns, kind, nbytes, first_row=0):
    """the blosc_gpu_aggregate of an unfiltered aggregate over a chunk of these values (the sum plays no part in the rule)"""
    nan = is_nan(patterns, kind, nbytes)
    v = values_of(patterns, kind, nbytes)
    a = pkgmod.Aggregate()
    a.rows = a.count = len(patterns)
    a.nans = int(nan.sum())
    a.min_row = a.max_row = -1
    at = np.flatnonzero(~nan)
    if at.size:
        lo, hi = int(at[np.argmax(v[at] == v[at].min())]), int(at[np.argmax(v[at] == v[at].max())])
        a.min_row, a.max_row = first_row + lo, first_row + hi
        a.min[:nbytes] = list(int(patterns[lo]).to_bytes(nbytes, "little"))
        a.max[:nbytes] = list(int(patterns[hi]).to_bytes(nbytes, "little"))
    return a


def excluded_chunks(rows_plain, row_bytes, rows, terms, zoned):
    """the rule on the plaintext: 1 for every chunk that holds rows and in which some clause has no term that can be true.  terms:
    clauses_checks' tuples; zoned: the (offset, kind, nbytes) that have a zone"""
    first = np.concatenate([[0], np.cumsum(rows)])
    out = []
    for k, n in enumerate(rows):
        part = rows_plain[int(first[k]) * row_bytes:int(first[k + 1]) * row_bytes]
        gone = False
        for clause in {t[5] for t in terms}:
            can = False
            for offset, kind, nbytes, op, constant, c in terms:
                if c != clause: continue
                if (offset, kind, nbytes) not in zoned: can = True
                elif n: can |= table_says(W.field_of(part, row_bytes, offset, UINT, nbytes).astype(np.uint64), kind, nbytes, op, constant)
            gone |= not can
        out.append(int(bool(n) and gone))
    return out


class Env(K.Env):
    def __init__(self, pkg, lib, mem, oracle, writer):
        super().__init__(pkg, lib, mem, oracle, writer)
        pkg.declare_zones(lib)


# ---- the fields call ----
class FieldsOut:
    """the host outputs of one fields call, filled with sentinels"""
    def __init__(self, pkgmod, nchunks, nfields):
        self.n, self.nf = nchunks, nfields
        self.totals = (pkgmod.Aggregate * nfields)()
        self.chunks = (pkgmod.Aggregate * max(nchunks * nfields, 1))()
        C.memset(self.totals, SENTINEL, C.sizeof(self.totals))
        C.memset(self.chunks, SENTINEL, C.sizeof(self.chunks))
        self.status = (C.c_int * max(nchunks, 1))(*[A.INT_SENTINEL] * max(nchunks, 1))
        self.rows = (C.c_int * max(nchunks, 1))(*[A.INT_SENTINEL] * max(nchunks, 1))
        self.unread = C.c_size_t(A.SIZE_SENTINEL)

    def of_field(self, f):
        """what clauses_checks.check_aggregate returns for a call on field f alone"""
        return (bytes(self.totals[f]) + b"".join(bytes(self.chunks[k * self.nf + f]) for k in range(self.n)) + bytes(self.status)[:4 * self.n])


def fields_table(pkgmod, fields):
    return (pkgmod.Field * len(fields))(*[pkgmod.field(kind, nbytes, offset=offset) for offset, kind, nbytes in fields])


def raw_fields(lib, source, row_bytes, ftab, nf, table, n, out, stream=None):
    if source.packed:
        return lib.blosc_gpu_aggregate_fields_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, ftab, nf,
                                                     table, n, out.totals, out.chunks, out.status, out.rows, C.byref(out.unread), stream)
    return lib.blosc_gpu_aggregate_fields_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, ftab, nf, table, n, out.totals, out.chunks,
                                                out.status, out.rows, C.byref(out.unread), stream)


def single_call(env, source, row_bytes, field_args, terms, stream=None):
    """blosc_gpu_aggregate_clauses_* for one field: the bytes check_aggregate returns, and (rows, unread)"""
    offset, kind, nbytes = field_args
    out = A.Outputs(env.pkg, A.nchunks_of(source))
    table, n = K.terms_table(env.pkg, terms)
    rc = K.raw_aggregate(env.lib, source, row_bytes, env.pkg.field(kind, nbytes, offset=offset), table, n, out, stream)
    assert rc == 0, ("the clause call", field_args, rc)
    return bytes(out.total) + bytes(out.chunks)[:64 * out.n] + bytes(out.status)[:4 * out.n], (list(out.rows)[:out.n], out.unread.value)


def check_fields(env, source, chunks, rows_plain, row_bytes, fields, terms, dead=None, stream=None, grounded=(0, -1), what=""):
    """one fields call: every field's bytes against the clause call for that field alone; the fields numbered in `grounded` against numpy as
    well (clauses_checks.check_aggregate).  Returns all the bytes the call wrote"""
    n = A.nchunks_of(source)
    out = FieldsOut(env.pkg, n, len(fields))
    table, nterms = K.terms_table(env.pkg, terms)
    rc = raw_fields(env.lib, source, row_bytes, fields_table(env.pkg, fields), len(fields), table, nterms, out, stream)
    what = (what, "row_bytes", row_bytes, "nfields", len(fields), "nterms", len(terms), "packed" if source.packed else "batch")
    assert rc == 0, (what, rc)
    grounded = {g % len(fields) for g in grounded}
    seen = {}
    for f, fld in enumerate(fields):
        if f in grounded:
            want = K.check_aggregate(env, source, chunks, rows_plain, row_bytes, fld, terms, dead=dead, stream=stream, what=(what, "field", f))
            other = (chunk_rows(chunks, row_bytes), sum(chunk_rows(chunks, row_bytes)[k] for k in (dead or {})))
        elif fld in seen:
            want, other = seen[fld]
        else:
            want, other = single_call(env, source, row_bytes, fld, terms, stream)
        seen[fld] = (want, other)
        got = out.of_field(f)
        if got != want:
            k = next(i for i in range(len(got)) if got[i] != want[i])
            raise AssertionError((what, "field", f, fld, "differs from the clause call at byte", k, "entry", (k - 64) // 64 if k >= 64 else "total"))
        assert (list(out.rows)[:n], out.unread.value) == other, (what, "rows / unread", list(out.rows), out.unread.value, other)
    return bytes(out.totals) + bytes(out.chunks)[:64 * n * len(fields)] + bytes(out.status)[:4 * n] + bytes(out.rows)[:4 * n]


def nfields_of(layout, n):
    """n fields out of a layout, cycled: repeats as soon as n exceeds it"""
    return [layout[i % len(layout)] for i in range(n)]


# rows of 20 bytes (clauses_checks.SHAPE_LAYOUT) in chunks of EDGE_ROWS rows and a MEMCPYED chunk
def table20(env, turn=0, rows=None):
    rows = K.EDGE_ROWS if rows is None else rows
    fields_for = K.drawn_fields(K.SHAPE_LAYOUT, K.ORDER, K.total_of(K.SHAPE_ROW, rows, True), seed=7)
    return K.table_call(env, K.SHAPE_ROW, rows, fields_for, setting=("lz4", 4, 1), turn=turn, memcpyed=True)


TERM_LISTS = {"no terms": [], "one term": K.PLAIN_TERMS[:1], "16 terms": K.SHAPES["16 terms, 4 x 4"]}


def case_shape_fields(env, table, counts=(1, 2, 15, 16), lists=("no terms", "one term", "16 terms"), sources=(0, 1)):
    """1, 2, 15 and 16 fields out of the five of SHAPE_LAYOUT (above five they repeat) with 0, 1 and 16 terms, batch and packed; the call of
    16 fields and the call of 1 agree on field 0"""
    chunks, rows_plain = table
    both = K.both_sources(env, chunks)
    for name in lists:
        terms = TERM_LISTS[name]
        if terms:
            mask = K.mask_of(rows_plain, K.SHAPE_ROW, terms)
            assert mask.any() and not mask.all(), name
        for s in sources:
            first = {}
            for nf in counts:
                got = check_fields(env, both[s], chunks, rows_plain, K.SHAPE_ROW, nfields_of(K.SHAPE_LAYOUT, nf), terms, what=("shape", name))
                first[nf] = got[:64]
            assert len(set(first.values())) == 1, ("field 0's total depends on the number of fields", name)


# rows of 96 bytes: the twelve kinds of where_checks.KINDS packed from byte 1 on (46 bytes, most of them unaligned), then four more fields:
# eight bytes across the first ones, the binary32 again (a repeated field), a binary32 of its own and two bytes at the row's end
def wide_layout():
    layout, at = [], 1
    for kind, nbytes in W.KINDS:
        layout.append((at, kind, nbytes))
        at += nbytes
    assert at == 47 and len(layout) == 12
    return layout


WIDE_ROW = 96
WIDE_KINDS = wide_layout()
WIDE_FIELDS = WIDE_KINDS + [(3, UINT, 8), WIDE_KINDS[9], (90, FLOAT, 4), (94, INT, 2)]
assert len(WIDE_FIELDS) == 16 and {(k, b) for _, k, b in WIDE_FIELDS} == set(W.KINDS)


def wide_terms(n):
    """n terms over the twelve kinds, four clauses of n / 4: every constant out of the field's value_set"""
    terms = []
    for i in range(n):
        offset, kind, nbytes = WIDE_KINDS[(5 * i) % 12]
        values = W.value_set(kind, nbytes)
        terms.append((offset, kind, nbytes, (NE, GE, LE, NE)[i % 4], values[(2, 7)[kind in (FLOAT, BFLOAT16)]], i % 4 if n > 1 else 0))
    return terms


def table96(env, rows, turn=0):
    sets = [W.value_set(kind, nbytes) for _, kind, nbytes in WIDE_KINDS] + [K.F32_SET, K.I16_SET]
    layout = WIDE_KINDS + [(90, FLOAT, 4), (94, INT, 2)]
    fields_for = K.drawn_fields(layout, sets, K.total_of(WIDE_ROW, rows), seed=13)      # (no MEMCPYED chunk: with fifty bytes of every row drawn from small sets the codecs win)
    return K.table_call(env, WIDE_ROW, rows, fields_for, setting=("blosclz" if turn % 2 else "lz4", 8, 1), turn=turn)


def case_wide_fields(env, table, lists=(0, 1, 16), sources=(0, 1)):
    """16 fields of every kind and width, overlapping and repeated, with 0, 1 and 16 terms"""
    chunks, rows_plain = table
    both = K.both_sources(env, chunks)
    for n in lists:
        terms = wide_terms(n)
        if terms:
            mask = K.mask_of(rows_plain, WIDE_ROW, terms)
            assert mask.any() and not mask.all(), n
        for s in sources:
            check_fields(env, both[s], chunks, rows_plain, WIDE_ROW, WIDE_FIELDS, terms, grounded=(9, 12) if s else (0, 10), what=("wide", n))


def case_fields_damage(env, chunk_of, what=""):
    """a chunk that does not decode between two that do: its status, its zeroed entries for every field, its rows in unread"""
    from getitem_ranges_checks import pick_damage
    rows = W.N // 17
    values = W.value_set(INT, 4)
    good = [chunk_of(K.make_rows(rows, 17, [(3, 4, W.drawn(values, rows, seed=30 + k)), (9, 1, W.drawn(K.U8_SET, rows, seed=50 + k))], seed=40 + k)) for k in range(3)]
    rows_plain = plaintext(env.oracle, good)
    found, _ = pick_damage(env.oracle, good[1])
    name, bad = found[0]
    chunks = [good[0], bad, good[2]]
    code = W.decoder_code(env.oracle, bad)
    terms = [(3, INT, 4, NE, values[2], 0), (9, UINT, 1, GE, 2, 1)]
    fields = [(3, INT, 4), (9, UINT, 1), (3, INT, 4), (11, UINT, 2)]
    for src in K.both_sources(env, chunks):
        got = check_fields(env, src, chunks, rows_plain, 17, fields, terms, dead={1: code}, what=(what, name))
        entries = got[64 * 4:64 * 4 + 64 * 12]
        assert entries[64 * 4:64 * 8] == (bytes(24) + b"\xff" * 16 + bytes(24)) * 4, "a dead chunk's entries are not those of nothing"


def case_fields_passes(env, table, sources=(0, 1)):
    """under a pass bound of 16 KiB - chunks in several passes - and under the default: the same bytes"""
    chunks, rows_plain = table
    terms = TERM_LISTS["one term"]
    fields = nfields_of(K.SHAPE_LAYOUT, 7)
    assert sum(header(c)["nbytes"] for c in chunks) > 16 << 10      # more than one pass
    for src in [K.both_sources(env, chunks)[s] for s in sources]:
        one = check_fields(env, src, chunks, rows_plain, K.SHAPE_ROW, fields, terms, what="default bound")
        env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            assert check_fields(env, src, chunks, rows_plain, K.SHAPE_ROW, fields, terms, what="16 KiB passes") == one, "the pass bound changes the answer"
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)


ROUND_ROWS = [1025, 0, 700, 2049]
ROUND_ROW, ROUND_LAYOUT = 17, [(3, FLOAT, 4), (8, FLOAT, 8)]


def case_fields_rounding(env, turn=0, rows=None):
    """aggregate_checks.rounding_values in a binary32 and a binary64 field of one row: sums that round in nearly every addition, so that the
    order of the additions shows.  check_aggregate holds both fields against tree_sum bit for bit; the fields call gives the same bytes,
    unfiltered and under GT 0 on the other field"""
    rows = ROUND_ROWS if rows is None else rows
    n = sum(rows)
    x32, x64 = A.rounding_values(4, n), A.rounding_values(8, n)[::-1]
    pats = [A.patterns_of(x32, FLOAT, 4), A.patterns_of(x64, FLOAT, 8)]
    fields_for = lambda first, m: [(off, nb, p[first:first + m]) for (off, _, nb), p in zip(ROUND_LAYOUT, pats)]
    chunks, rows_plain = K.table_call(env, ROUND_ROW, rows, fields_for, setting=("lz4", 4, 1), turn=turn)
    for src in K.both_sources(env, chunks):
        for terms in ([], [(8, FLOAT, 8, GT, 0, 0)], [(3, FLOAT, 4, LT, 0, 3)]):
            check_fields(env, src, chunks, rows_plain, ROUND_ROW, ROUND_LAYOUT + ROUND_LAYOUT[:1], terms, grounded=(0, 1), what="rounding")


def case_fields_tall(env, turn=0):
    """one chunk of 256 x 1024 + 1 rows: lane 0 of k_aggregate_chunks_fields folds a second tile.  Rows of 8 bytes read as binary64 (the sum
    that rounds: aggregate_checks.tall_patterns), as int64 and as the uint32 of their upper half"""
    rows = [A.TALL_ROWS[1]]
    chunks, rows_plain = A.tall_call(env, A.tall_patterns(rows, [A.TALL_SEEDS[1]]), rows, turn)
    src = TakeSource(env.mem, chunks=chunks)
    for terms in ([], [(0, FLOAT, 8, GT, 0, 0)]):
        check_fields(env, src, chunks, rows_plain, 8, [(0, FLOAT, 8), (0, INT, 8), (4, UINT, 4)], terms, grounded=(0,), what="tall")


def case_fields_stream(env, table, stream):
    chunks, rows_plain = table
    fields = nfields_of(K.SHAPE_LAYOUT, 5)
    for src in K.both_sources(env, chunks):
        assert (check_fields(env, src, chunks, rows_plain, K.SHAPE_ROW, fields, K.PLAIN_TERMS, stream=stream, what="side stream")
                == check_fields(env, src, chunks, rows_plain, K.SHAPE_ROW, fields, K.PLAIN_TERMS, what="NULL stream"))


# ---- the zoned calls ----
# rows of 16 bytes: an int32 that ascends with the row number, a binary32 of noise with NaNs, a uint16 key at byte 9 (no zone), and a
# uint32 that is noise but for one chunk in which it is constant
Z_ROW = 16
Z_STAMP, Z_NOISE, Z_KEY, Z_FLAG = (0, INT, 4), (4, FLOAT, 4), (9, UINT, 2), (12, UINT, 4)
Z_ZONED = [Z_STAMP, Z_NOISE, Z_FLAG]
Z_ROWS = [700, 1025, 300, 0, 64, 1500, 63]
Z_CONSTANT_CHUNK, Z_CONSTANT = 2, 7
Z_TALL = 5      # the chunk of several blocks, which pick_damage can damage


def stamp(r):
    """the ascending column: row r holds 3 r - 1000"""
    return 3 * r - 1000


def zoned_table(env, turn=0, rows=None):
    rows = Z_ROWS if rows is None else rows
    n = sum(rows)
    first = np.concatenate([[0], np.cumsum(rows)])
    r = np.arange(n)
    flag = W.drawn(K.U32_SET, n, seed=17)
    flag[first[Z_CONSTANT_CHUNK]:first[Z_CONSTANT_CHUNK + 1]] = Z_CONSTANT
    pats = [(stamp(r) % 2 ** 32).astype(np.uint64), W.drawn(K.F32_SET, n, seed=5), W.drawn(K.U8_SET, n, seed=6), flag]
    layout = [Z_STAMP, Z_NOISE, Z_KEY, Z_FLAG]
    fields_for = lambda f, m: [(off, nb, p[f:f + m]) for (off, _, nb), p in zip(layout, pats)]
    chunks, rows_plain = K.table_call(env, Z_ROW, rows, fields_for, setting=("lz4", 4, 1), turn=turn)
    return chunks, rows_plain


def build_map(env, source, chunks, rows_plain, zoned=None):
    """the zone map of the zoned fields by the fields call (no terms): (the Field table, the entries as the call wrote them)"""
    zoned = Z_ZONED if zoned is None else zoned
    n = A.nchunks_of(source)
    out = FieldsOut(env.pkg, n, len(zoned))
    ftab = fields_table(env.pkg, zoned)
    assert raw_fields(env.lib, source, Z_ROW, ftab, len(zoned), None, 0, out) == 0
    assert list(out.rows)[:n] == chunk_rows(chunks, Z_ROW) and out.unread.value == 0
    rows = chunk_rows(chunks, Z_ROW)
    first = np.concatenate([[0], np.cumsum(rows)])
    for k in range(n):      # ... and it says what numpy says of every chunk
        for f, (offset, kind, nbytes) in enumerate(zoned):
            pats = W.field_of(rows_plain[int(first[k]) * Z_ROW:int(first[k + 1]) * Z_ROW], Z_ROW, offset, UINT, nbytes).astype(np.uint64)
            want = A.entry(entry_of(env.pkg, pats, kind, nbytes, int(first[k]))) if rows[k] else A.NOTHING
            assert A.entry(out.chunks[k * len(zoned) + f])[:7] == want[:7], ("the map", k, f)
    return ftab, out.chunks


def at_row(r, op, clause):
    return Z_STAMP + (op, stamp(r) % 2 ** 32, clause)


def zoned_lists(rows=None):
    """family -> [(name, terms, prunes some but not all)]"""
    rows = Z_ROWS if rows is None else rows
    first = np.concatenate([[0], np.cumsum(rows)])
    nan = 0x7fc00000
    f = [int(x) for x in first]
    return {
        "a range inside one chunk": [("chunk 1", [at_row(f[1] + 10, GE, 0), at_row(f[1] + 500, LT, 1)], True),
                                     ("the last chunk", [at_row(f[6] + 1, GT, 0), at_row(f[7] - 1, LE, 3)], True)],
        "a range across a chunk edge": [("chunks 1 and 2", [at_row(f[2] - 20, GE, 0), at_row(f[2] + 20, LT, 1)], True),
                                        ("across the empty chunk", [at_row(f[3] - 5, GE, 4), at_row(f[4] + 5, LE, 9)], True)],
        "nothing": [("below every row", [at_row(-1, LT, 0)], False), ("an empty range", [at_row(f[2], GE, 0), at_row(f[2], LT, 1)], False)],
        "everything": [("from the first row", [at_row(0, GE, 0)], False)],
        "a key set": [("three rows of three chunks", [at_row(5, EQ, 2), at_row(f[2] + 1, EQ, 2), at_row(f[6], EQ, 2)], True),
                      ("a key between two rows", [Z_STAMP + (EQ, (stamp(f[1] + 3) + 1) % 2 ** 32, 0)], True)],
        "a column without a zone": [("the key alone", [Z_KEY + (EQ, 3, 0)], False),
                                    ("the key and a range", [Z_KEY + (EQ, 3, 0), at_row(f[5] + 100, GE, 1)], True)],
        "a NaN constant": [("EQ a NaN", [Z_NOISE + (EQ, nan, 0)], False), ("NE a NaN", [Z_NOISE + (NE, nan, 0)], False),
                           ("a NaN inside an OR clause", [Z_NOISE + (GT, nan, 0), at_row(f[4] + 3, LT, 0)], True)],
        "NE on a constant chunk": [("the flag", [Z_FLAG + (NE, Z_CONSTANT, 0)], True), ("the flag equal", [Z_FLAG + (EQ, Z_CONSTANT, 1), at_row(f[1], GE, 0)], True)],
    }


class ZonedOut:
    def __init__(self, n):
        self.pruned = (C.c_uint8 * max(n, 1))(*[SENTINEL] * max(n, 1))


def raw_where_zoned(lib, source, row_bytes, table, n, ftab, nz, zones, index_ptr, capacity, out, pruned, stream=None):
    if source.packed:
        return lib.blosc_gpu_where_zoned_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, table, n, ftab, nz,
                                                zones, index_ptr, capacity, C.byref(out.total), out.matches, out.rows, C.byref(out.unread), pruned, stream)
    return lib.blosc_gpu_where_zoned_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, table, n, ftab, nz, zones, index_ptr, capacity,
                                           C.byref(out.total), out.matches, out.rows, C.byref(out.unread), pruned, stream)


def run_where_zoned(env, source, terms, ftab, nz, zones, capacity, stream=None):
    """(answer, the table's bytes, the host outputs, chunk_pruned_out); the sentinel words around index_out are asserted"""
    out = W.Outputs(W.nchunks_of(source))
    pruned = ZonedOut(out.n).pruned
    buf, base = env.mem.filled(8 * (capacity + 2 * W.GUARD), W.SENTINEL)
    table, n = K.terms_table(env.pkg, terms)
    rc = raw_where_zoned(env.lib, source, Z_ROW, table, n, ftab, nz, zones, base + 8 * W.GUARD if capacity else None, capacity, out, pruned, stream)
    words = np.ascontiguousarray(env.mem.get(buf)[:8 * (capacity + 2 * W.GUARD)]).view(np.int64)
    assert np.all(words[:W.GUARD] == W.WORD_SENTINEL) and np.all(words[W.GUARD + capacity:] == W.WORD_SENTINEL), "words outside index_out were written"
    return rc, words[W.GUARD:W.GUARD + capacity].tobytes(), out, list(pruned)[:out.n]


def raw_aggregate_zoned(lib, source, row_bytes, fld, table, n, ftab, nz, zones, out, pruned, stream=None):
    if source.packed:
        return lib.blosc_gpu_aggregate_zoned_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, C.byref(fld),
                                                    table, n, ftab, nz, zones, C.byref(out.total), out.chunks, out.status, out.rows, C.byref(out.unread), pruned,
                                                    stream)
    return lib.blosc_gpu_aggregate_zoned_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, C.byref(fld), table, n, ftab, nz, zones,
                                               C.byref(out.total), out.chunks, out.status, out.rows, C.byref(out.unread), pruned, stream)


def run_aggregate_zoned(env, source, field_args, terms, ftab, nz, zones, stream=None):
    """(answer, the bytes check_aggregate returns, (rows, unread), chunk_pruned_out)"""
    offset, kind, nbytes = field_args
    out = A.Outputs(env.pkg, A.nchunks_of(source))
    pruned = ZonedOut(out.n).pruned
    table, n = K.terms_table(env.pkg, terms)
    rc = raw_aggregate_zoned(env.lib, source, Z_ROW, env.pkg.field(kind, nbytes, offset=offset), table, n, ftab, nz, zones, out, pruned, stream)
    return (rc, bytes(out.total) + bytes(out.chunks)[:64 * out.n] + bytes(out.status)[:4 * out.n], (list(out.rows)[:out.n], out.unread.value),
            list(pruned)[:out.n])


def check_zoned(env, source, chunks, rows_plain, terms, zone_map, zoned=None, capacity=None, aggregated=Z_NOISE, what=""):
    """the zoned where and the zoned aggregate of one list against the clause calls (held against numpy by clauses_checks) byte for byte, and
    chunk_pruned_out against the rule in numpy.  Returns the pruned flags"""
    zoned = Z_ZONED if zoned is None else zoned
    ftab, zones = zone_map
    rows = chunk_rows(chunks, Z_ROW)
    want_pruned = excluded_chunks(rows_plain, Z_ROW, rows, terms, zoned)
    table, outs = K.check_where(env, source, chunks, rows_plain, Z_ROW, terms, capacity=capacity, what=(what, "the clause call"))
    cap = outs[0] + 5 if capacity is None else capacity
    rc, got_table, out, pruned = run_where_zoned(env, source, terms, ftab, len(zoned), zones, cap)
    assert rc == 0, (what, rc)
    assert pruned == want_pruned, (what, "chunk_pruned_out", pruned, want_pruned)
    assert got_table == table and K.outputs_of(out) == outs, (what, "the zoned where differs from the clause call", K.outputs_of(out), outs)
    want = K.check_aggregate(env, source, chunks, rows_plain, Z_ROW, aggregated, terms, what=(what, "the clause call"))
    rc, got, other, pruned = run_aggregate_zoned(env, source, aggregated, terms, ftab, len(zoned), zones)
    assert rc == 0 and pruned == want_pruned, (what, "aggregate", rc, pruned, want_pruned)
    assert got == want and other == (rows, 0), (what, "the zoned aggregate differs from the clause call")
    return pruned


def case_zoned_family(env, table, family, sources=(0, 1)):
    chunks, rows_plain = table
    both = K.both_sources(env, chunks)
    holding = sum(1 for r in chunk_rows(chunks, Z_ROW) if r)
    partly = 0
    for n, (name, terms, some) in enumerate(zoned_lists()[family]):
        for s in sources:
            src = both[s]
            pruned = check_zoned(env, src, chunks, rows_plain, terms, build_map(env, both[(s + n) % 2], chunks, rows_plain), what=(family, name))
            assert (0 < sum(pruned) < holding) == some, (family, name, pruned)
            partly += some
    assert partly or family in ("nothing", "everything"), (family, "no list of the family prunes some chunks and not all")


def case_zoned_nothing_and_everything(env, table):
    """an all-pruned call answers 0 with total 0 and decodes nothing; a list that excludes nothing prunes nothing"""
    chunks, rows_plain = table
    src = TakeSource(env.mem, chunks=chunks)
    zone_map = build_map(env, src, chunks, rows_plain)
    rows = chunk_rows(chunks, Z_ROW)
    name, terms, _ = zoned_lists()["nothing"][0]
    assert check_zoned(env, src, chunks, rows_plain, terms, zone_map, what=name) == [int(r > 0) for r in rows]
    name, terms, _ = zoned_lists()["everything"][0]
    assert check_zoned(env, src, chunks, rows_plain, terms, zone_map, what=name) == [0] * len(rows)
    # no zone fields at all: the clause call
    assert check_zoned(env, src, chunks, rows_plain, zoned_lists()["nothing"][0][1], (None, None), zoned=[], what="nzfields 0") == [0] * len(rows)


def case_zoned_garbage(env, table):
    """the proof that a pruned chunk is not read: the excluded chunk of several blocks is damaged.  The zoned calls answer as before, with no
    unread row; the clause call reports the decoder's code for it"""
    from getitem_ranges_checks import pick_damage
    chunks, rows_plain = table
    rows = chunk_rows(chunks, Z_ROW)
    first = [int(x) for x in np.concatenate([[0], np.cumsum(rows)])]
    whole = orc_compress(env.oracle, rows_plain[first[Z_TALL] * Z_ROW:first[Z_TALL + 1] * Z_ROW], 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]      # (case_damage's typesize: blocks of 8 KiB)
    found, _ = pick_damage(env.oracle, whole)
    name, bad = found[0]
    code = W.decoder_code(env.oracle, bad)
    damaged = list(chunks)
    damaged[Z_TALL] = bad
    terms = [at_row(first[1] + 10, GE, 0), at_row(first[2] + 20, LT, 1)]      # chunks 1 and 2
    for good_src, bad_src in zip(K.both_sources(env, chunks), K.both_sources(env, damaged)):
        zone_map = build_map(env, good_src, chunks, rows_plain)
        pruned = check_zoned(env, good_src, chunks, rows_plain, terms, zone_map, what="before the damage")
        assert pruned[Z_TALL] == 1 and pruned[1] == 0
        ftab, zones = zone_map
        total = int(K.mask_of(rows_plain, Z_ROW, terms).sum())
        before = run_where_zoned(env, good_src, terms, ftab, len(Z_ZONED), zones, total + 5)
        after = run_where_zoned(env, bad_src, terms, ftab, len(Z_ZONED), zones, total + 5)
        assert after[0] == 0 and after[1] == before[1] and K.outputs_of(after[2]) == K.outputs_of(before[2]) and after[3] == before[3], "the damaged chunk was read"
        assert after[2].unread.value == 0 and after[2].total.value == total > 0
        before = run_aggregate_zoned(env, good_src, Z_NOISE, terms, ftab, len(Z_ZONED), zones)
        after = run_aggregate_zoned(env, bad_src, Z_NOISE, terms, ftab, len(Z_ZONED), zones)
        assert after == before and after[2][1] == 0, "the damaged chunk was read by the aggregate"
        # ... while the clause call decodes it and says so
        rc, _, out = K.run_where(env, bad_src, Z_ROW, terms, total + 5)
        assert rc == 0 and out.matches[Z_TALL] == code and out.unread.value == rows[Z_TALL], (list(out.matches), code)
        # a list that does not exclude it: the zoned call reads it too
        rc, _, out, pruned = run_where_zoned(env, bad_src, [at_row(first[Z_TALL] + 1, GE, 0)], ftab, len(Z_ZONED), zones, 0)
        assert rc == 0 and pruned[Z_TALL] == 0 and out.matches[Z_TALL] == code and out.unread.value == rows[Z_TALL]


def case_zoned_stale_rows(env, table):
    """a map with one entry's rows off by one is refused before anything is decoded, with nothing but chunk_rows_out written"""
    chunks, rows_plain = table
    rows = chunk_rows(chunks, Z_ROW)
    terms = [at_row(5, GE, 0)]
    for src in K.both_sources(env, chunks):
        ftab, zones = build_map(env, src, chunks, rows_plain)
        for k, f, delta in ((1, 0, 1), (len(rows) - 1, 2, -1), (3, 1, 1)):      # (chunk 3 holds no row: its entry says 0, which any census agrees with until it says 1)
            copy = (env.pkg.Aggregate * len(zones))()
            C.memmove(copy, zones, C.sizeof(zones))
            copy[k * len(Z_ZONED) + f].rows += delta
            rc, table_bytes, out, pruned = run_where_zoned(env, src, terms, ftab, len(Z_ZONED), copy, 4)
            assert rc < 0 and list(out.rows)[:out.n] == rows and pruned == [SENTINEL] * len(rows), ("stale rows", k, rc)
            assert out.untouched(), ("stale rows: an output was written", k)
            assert table_bytes == np.full(4, W.WORD_SENTINEL).tobytes()
            agg = A.Outputs(env.pkg, len(rows))
            flags = ZonedOut(len(rows)).pruned
            table, n = K.terms_table(env.pkg, terms)
            rc = raw_aggregate_zoned(env.lib, src, Z_ROW, env.pkg.field(FLOAT, 4, offset=4), table, n, ftab, len(Z_ZONED), copy, agg, flags)
            assert rc < 0 and agg.untouched() and list(agg.rows)[:agg.n] == rows and list(flags)[:len(rows)] == [SENTINEL] * len(rows)


def case_zoned_capacity_and_passes(env, table, sources=(0, 1), caps=(0, 1, -1, None)):
    """capacity below the total, batch and packed; and the 16 KiB pass bound, under which the live chunks are dealt to passes of their own"""
    chunks, rows_plain = table
    first = [int(x) for x in np.concatenate([[0], np.cumsum(chunk_rows(chunks, Z_ROW))])]
    terms = [at_row(first[1] + 10, GE, 0), at_row(first[5] + 20, LT, 1), Z_KEY + (NE, 3, 2)]
    total = int(K.mask_of(rows_plain, Z_ROW, terms).sum())
    assert total > 8
    for src in [K.both_sources(env, chunks)[s] for s in sources]:
        zone_map = build_map(env, src, chunks, rows_plain)
        flags = [check_zoned(env, src, chunks, rows_plain, terms, zone_map, capacity=cap, what=("capacity", cap))
                 for cap in [total + c if c else total if c is None else 0 for c in caps]]
        assert all(f == flags[0] for f in flags) and 0 < sum(flags[0]) < len(chunks) - 1
        env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            assert check_zoned(env, src, chunks, rows_plain, terms, zone_map, what="16 KiB passes") == flags[0]
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)
