"""What tests/test_gpu_clauses.py (device) and tests/test_emu_clauses.py (wavefront emulator) both assert about the calls of
include/blosc_gpu_clauses.h, and the cases they run.  The yardstick is numpy on the plaintext, as in where_checks.expected: the plaintext of
every chunk is the oracle's, every term is evaluated by the numpy comparison on its field view, the terms of a clause are combined with `|`,
the clauses with `&`, and the rows of chunks that do not decode are knocked out.  Everything is compared exactly: the index table, the
counts, all 64 bytes of an aggregate - its floating-point sum bit for bit against aggregate_checks.tree_sum over the rows numpy lets through.

A term is (offset, kind, nbytes, op, constant pattern, clause).  Except in the cases named "none" / "every", assert_not_vacuous() holds
numpy's own answer to this before the library is called: the list matches some rows and not all, so does every single term, the list's table
differs from every single term's, and a list of several clauses with an OR in it differs from the all-AND and the all-OR reading of its terms."""
import ctypes as C

import numpy as np

import aggregate_checks as A
import where_checks as W
from getitem_ranges_checks import plain
from helpers import header, orc_compress
from take_checks import BLOCKSIZE, MEMCPYED_BYTES, TakeSource, chunk_rows, pack_container, plaintext
from where_checks import BFLOAT16, FLOAT, INT, UINT, GUARD, SENTINEL, WORD_SENTINEL

EQ, NE, LT, LE, GT, GE = range(6)


# ---- numpy's answer ----
def term_hits(rows_plain, row_bytes, terms):
    """one boolean array per term"""
    out = []
    with np.errstate(invalid="ignore"):
        for offset, kind, nbytes, op, constant, _ in terms:
            out.append(np.asarray(W.OPS[op](W.field_of(rows_plain, row_bytes, offset, kind, nbytes), W.comparable([constant], kind, nbytes)[0])))
    return out


def combine(hits, clauses):
    """the terms of a clause with |, the clauses with &; no term: every row"""
    mask = None
    for c in sorted(set(clauses)):
        one = None
        for h, k in zip(hits, clauses):
            if k == c: one = h.copy() if one is None else one | h
        mask = one if mask is None else mask & one
    return mask


def mask_of(rows_plain, row_bytes, terms, dead=()):
    nrows = rows_plain.size // row_bytes
    mask = combine(term_hits(rows_plain, row_bytes, terms), [t[5] for t in terms]) if terms else np.ones(nrows, bool)
    for lo, hi in dead:
        mask[lo:hi] = False
    return mask


def assert_not_vacuous(rows_plain, row_bytes, terms, exempt=()):
    """the condition of the module's docstring on numpy's answer.  exempt: indices of terms that are stated to match no row (a NaN constant)"""
    hits = term_hits(rows_plain, row_bytes, terms)
    clauses = [t[5] for t in terms]
    both = combine(hits, clauses)
    assert both.any() and not both.all(), ("the list matches none or all", int(both.sum()), both.size)
    for k, h in enumerate(hits):
        if k in exempt:
            assert not h.any(), ("a term stated to match nothing matches", k)
            continue
        assert h.any() and not h.all(), ("a term matches none or all", k, terms[k], int(h.sum()))
        assert len(terms) == 1 or not np.array_equal(h, both), ("the list gives a single term's table", k, terms[k])
    if 1 < len(set(clauses)) < len(terms):      # mixed: neither reading alone
        every, any_of = combine(hits, list(range(len(terms)))), combine(hits, [0] * len(terms))
        assert not np.array_equal(both, every) and not np.array_equal(both, any_of), "a mixed list reads as all-AND or all-OR"
    return both


# ---- tables: rows with several fields ----
def make_rows(nrows, row_bytes, fields, seed=21, noise=False, step=1):
    """where_checks.make_table with several fields: fields = [(offset, nbytes, patterns)], written into one row in `step`"""
    tab = W.make_table(nrows, row_bytes, 0, 1, None, seed=seed, noise=noise).reshape(nrows, row_bytes)
    for offset, nbytes, patterns in fields:
        raw = np.ascontiguousarray(patterns, dtype=f"<u{nbytes}").view(np.uint8).reshape(nrows, nbytes)
        tab[::step, offset:offset + nbytes] = raw[::step]
    return tab.reshape(-1)


def empty_chunk(env):
    return orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1]


def memcpyed_chunk(env, row_bytes, fields_for, first):
    """a chunk of random rows that the oracle stores MEMCPYED, the fields set in one row of four"""
    rows = MEMCPYED_BYTES // row_bytes
    data = make_rows(rows, row_bytes, fields_for(first, rows), seed=3, noise=True, step=4)
    chunk = orc_compress(env.oracle, data, 4, 5, 1, "lz4")[1]
    assert header(chunk)["flags"] & 2
    return chunk


def table_call(env, row_bytes, rows, fields_for, setting=("lz4", 4, 1), turn=0, memcpyed=False):
    """(chunks, their plaintext) of one call: chunk k holds rows[k] rows (0: a chunk of nbytes 0); fields_for(first_row, nrows) -> the fields
    of these rows as make_rows takes them; memcpyed: one more chunk, stored MEMCPYED"""
    cname, T, shuffle = setting
    write = env.writer(cname, T, shuffle, turn)
    chunks, first = [], 0
    for k, n in enumerate(rows):
        chunks.append(write(k, make_rows(n, row_bytes, fields_for(first, n), seed=21 + k)) if n else empty_chunk(env))
        first += n
    if memcpyed:
        chunks.append(memcpyed_chunk(env, row_bytes, fields_for, first))
    assert chunk_rows(chunks, row_bytes)[:len(rows)] == list(rows)
    return chunks, plaintext(env.oracle, chunks)


def drawn_fields(layout, sets, nrows_total, seed=4):
    """fields_for of a table whose field i = layout[i] = (offset, kind, nbytes) is drawn from sets[i], every field with a seed of its own"""
    pats = [W.drawn(s, nrows_total, seed=seed + 11 * i) for i, s in enumerate(sets)]
    return lambda first, n: [(off, nb, p[first:first + n]) for (off, _, nb), p in zip(layout, pats)]


def total_of(row_bytes, rows, memcpyed=False):
    return sum(rows) + (MEMCPYED_BYTES // row_bytes if memcpyed else 0)


def both_sources(env, chunks):
    return TakeSource(env.mem, chunks=chunks), TakeSource(env.mem, *(None,) + pack_container(chunks))


# ---- one call ----
def terms_table(pkgmod, terms):
    rows = [pkgmod.term(W.predicate(pkgmod, kind, nbytes, op, constant, offset), clause) for offset, kind, nbytes, op, constant, clause in terms]
    return ((pkgmod.Term * len(rows))(*rows) if rows else None), len(rows)


def raw_where(lib, source, row_bytes, table, n, index_ptr, capacity, out, stream=None):
    if source.packed:
        return lib.blosc_gpu_where_clauses_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, table, n,
                                                  index_ptr, capacity, C.byref(out.total), out.matches, out.rows, C.byref(out.unread), stream)
    return lib.blosc_gpu_where_clauses_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, table, n, index_ptr, capacity,
                                             C.byref(out.total), out.matches, out.rows, C.byref(out.unread), stream)


def run_where(env, source, row_bytes, terms, capacity, null_table=False, stream=None):
    """where_checks.run_where for a term list: index_out between GUARD sentinel words, which are asserted here.  Returns (answer, the `capacity`
    words of the table, Outputs)"""
    out = W.Outputs(W.nchunks_of(source))
    buf, base = env.mem.filled(8 * (capacity + 2 * GUARD), SENTINEL)
    assert base % 8 == 0
    table, n = terms_table(env.pkg, terms)
    rc = raw_where(env.lib, source, row_bytes, table, n, None if null_table else base + 8 * GUARD, capacity, out, stream)
    words = np.ascontiguousarray(env.mem.get(buf)[:8 * (capacity + 2 * GUARD)]).view(np.int64)
    assert np.all(words[:GUARD] == WORD_SENTINEL) and np.all(words[GUARD + capacity:] == WORD_SENTINEL), "words outside index_out were written"
    return rc, words[GUARD:GUARD + capacity].copy(), out


def outputs_of(out):
    return (out.total.value, out.unread.value, list(out.matches)[:out.n], list(out.rows)[:out.n])


def check_where(env, source, chunks, rows_plain, row_bytes, terms, capacity=None, dead=(), codes=None, stream=None, what=""):
    """one call against numpy, as where_checks.check_where holds it.  capacity None: the total + 5.  Returns (the whole table as written, the
    host outputs) for callers that compare two calls"""
    want = np.nonzero(mask_of(rows_plain, row_bytes, terms, dead))[0].astype(np.int64)
    cap = want.size + 5 if capacity is None else capacity
    rc, table, out = run_where(env, source, row_bytes, terms, cap, null_table=(capacity == 0), stream=stream)
    what = (what, "row_bytes", row_bytes, "terms", terms, "capacity", cap)
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
    assert np.all(table[m:] == WORD_SENTINEL), (what, "words from min(total, capacity) on were written")
    return table.tobytes(), outputs_of(out)


def raw_aggregate(lib, source, row_bytes, fld, table, n, out, stream=None):
    if source.packed:
        return lib.blosc_gpu_aggregate_clauses_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes,
                                                      C.byref(fld), table, n, C.byref(out.total), out.chunks, out.status, out.rows, C.byref(out.unread), stream)
    return lib.blosc_gpu_aggregate_clauses_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, C.byref(fld), table, n, C.byref(out.total),
                                                 out.chunks, out.status, out.rows, C.byref(out.unread), stream)


def check_aggregate(env, source, chunks, rows_plain, row_bytes, field_args, terms, dead=None, stream=None, what=""):
    """one call against numpy, as aggregate_checks.check_aggregate holds it with the list's mask in the filter's place: counts, extremes and
    integer sums exact, every chunk's floating-point sum bit for bit against tree_sum, the total the left fold of the chunks bit for bit.
    Returns all the bytes the call wrote, for callers that compare two calls"""
    offset, kind, nbytes = field_args
    out = A.Outputs(env.pkg, A.nchunks_of(source))
    table, n = terms_table(env.pkg, terms)
    rc = raw_aggregate(env.lib, source, row_bytes, env.pkg.field(kind, nbytes, offset=offset), table, n, out, stream)
    what = (what, "row_bytes", row_bytes, "field", field_args, "terms", terms)
    assert rc == 0, (what, rc)
    dead = dead or {}
    rows = chunk_rows(chunks, row_bytes)
    first = np.concatenate([[0], np.cumsum(rows)])
    assert list(out.rows)[:out.n] == rows, (what, list(out.rows))
    assert list(out.status)[:out.n] == [dead.get(k, 0) for k in range(out.n)], (what, "status", list(out.status))
    assert out.unread.value == sum(rows[k] for k in dead), (what, "unread", out.unread.value)
    vals, raw = W.field_of(rows_plain, row_bytes, offset, kind, nbytes), W.field_of(rows_plain, row_bytes, offset, UINT, nbytes)
    mask = mask_of(rows_plain, row_bytes, terms)
    got = [A.entry(out.chunks[k]) for k in range(out.n)]
    live = np.ones(vals.size, bool)
    for k in range(out.n):
        lo, hi = int(first[k]), int(first[k + 1])
        if k in dead or lo == hi:
            assert got[k] == A.NOTHING, (what, "chunk", k, got[k])
            live[lo:hi] = False
            continue
        want = A.expected_of(vals[lo:hi], raw[lo:hi], mask[lo:hi], kind, nbytes, lo)
        assert got[k][:7] == want[:7], (what, "chunk", k, got[k], want)
        if kind in (FLOAT, BFLOAT16):
            with np.errstate(invalid="ignore"):
                x = vals[lo:hi].astype(np.float64)
            A.check_tree(got[k][7], A.tree_sum(np.where(mask[lo:hi] & ~np.isnan(x), x, 0.0)), (what, "chunk", k))
        else:
            assert got[k][7] == want[7], (what, "chunk", k, "sum", got[k][7], want[7])
    total = A.entry(out.total)
    at = np.flatnonzero(live)
    want = A.expected_of(vals[at], raw[at], mask[at], kind, nbytes, 0)
    want = want[:3] + (int(at[want[3]]) if want[3] >= 0 else -1, int(at[want[4]]) if want[4] >= 0 else -1) + want[5:7]
    assert total[:7] == want, (what, "total", total, want)
    assert total == A.fold(got, kind, nbytes), (what, "the total is not the left fold of the chunks", total, A.fold(got, kind, nbytes))
    return bytes(out.total) + bytes(out.chunks)[:64 * out.n] + bytes(out.status)[:4 * out.n]


class Env(W.Env):
    def __init__(self, pkg, lib, mem, oracle, writer):
        super().__init__(pkg, lib, mem, oracle, writer)
        pkg.declare_aggregate(lib)
        pkg.declare_clauses(lib)


# ---- case 1: one term is the existing call, byte for byte ----
def one_term_constant(kind, nbytes):
    """a constant of where_checks.value_set under which all six ops match some rows and not all: 1, 0, +1.5"""
    values = W.value_set(kind, nbytes)
    return values[2] if kind in (UINT, INT) else values[7]


ONE_ROWS = [1500, 0, 700]


def case_one_term(env, kind, nbytes, ops=range(6), packed_ops=range(6), turn=0):
    """a field of this kind and width at offset 3 of rows of 17 bytes: the where table, total and chunk_matches of the list of one term against
    blosc_gpu_where_*, all 64 bytes per chunk and of the total against blosc_gpu_aggregate_* with the term as its filter, and no terms against
    filter NULL - two different kernels each time.  The numpy yardstick is held as well"""
    layout = [(3, kind, nbytes)]
    fields_for = drawn_fields(layout, [W.value_set(kind, nbytes)], total_of(17, ONE_ROWS, True))
    chunks, rows_plain = table_call(env, 17, ONE_ROWS, fields_for, setting=("blosclz" if turn % 2 else "lz4", 17, turn % 3), turn=turn, memcpyed=True)
    constant = one_term_constant(kind, nbytes)
    sources = both_sources(env, chunks)
    fld = env.pkg.field(kind, nbytes, offset=3)
    for op in ops:
        term = (3, kind, nbytes, op, constant, 5)
        assert_not_vacuous(rows_plain, 17, [term])
        pred = W.predicate(env.pkg, kind, nbytes, op, constant, 3)
        for src in sources[:2 if op in packed_ops else 1]:
            what = ("one term", W.kind_name(kind, nbytes), W.OPS[op].__name__, "packed" if src.packed else "batch")
            table, outs = check_where(env, src, chunks, rows_plain, 17, [term], what=what)
            cap = outs[0] + 5
            rc, old_table, old = W.run_where(env.lib, env.mem, src, 17, pred, cap)
            assert rc == 0 and old_table.tobytes() == table and outputs_of(old) == outs, (what, "differs from blosc_gpu_where_*")
            got = check_aggregate(env, src, chunks, rows_plain, 17, (3, kind, nbytes), [term], what=what)
            ref = A.Outputs(env.pkg, len(chunks))
            assert A.raw_call(env.lib, src, 17, fld, pred, ref) == 0
            assert got == bytes(ref.total) + bytes(ref.chunks)[:64 * ref.n] + bytes(ref.status)[:4 * ref.n], (what, "differs from blosc_gpu_aggregate_*")
    for src in sources:
        got = check_aggregate(env, src, chunks, rows_plain, 17, (3, kind, nbytes), [], what=("no terms", W.kind_name(kind, nbytes)))
        ref = A.Outputs(env.pkg, len(chunks))
        assert A.raw_call(env.lib, src, 17, fld, None, ref) == 0
        assert got == bytes(ref.total) + bytes(ref.chunks)[:64 * ref.n] + bytes(ref.status)[:4 * ref.n], ("no terms differ from filter NULL", src.packed)


# ---- case 2: term counts and clause shapes ----
# rows of 20 bytes, five fields of five kinds, two of them unaligned; every field drawn from eight values, ORDER[i] ascending (the NaN last)
SHAPE_LAYOUT = [(0, UINT, 1), (1, INT, 2), (3, UINT, 4), (8, FLOAT, 4), (12, INT, 8)]
SHAPE_ROW = 20
SHAPE_ROWS = [1025, 0, 700]


def _f32(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


ORDER = [list(range(8)),
         [v % 2 ** 16 for v in range(-4, 4)],
         [v * 0x01010101 for v in range(8)],
         [_f32(x) for x in (-2.0, -1.0, -0.0, 0.5, 1.0, 2.0, 3.0)] + [0x7fc00000],
         [(v << 33) % 2 ** 64 for v in range(-4, 4)]]
# a term by the share of rows it is to match: the (op, index into ORDER[field]) it may be, taken in turns
CLASSES = {"low": [(EQ, k) for k in range(7)], "high": [(NE, k) for k in range(7)],
           "quarter": [(LT, 2), (GT, 4), (LE, 1), (GE, 5)], "half": [(GE, 3), (LT, 3), (GT, 2), (LE, 3)]}


def shape_terms(clauses, classes):
    """term i tests field i % 5 and belongs to clauses[i]; classes[i] names its share"""
    terms = []
    for i, (clause, cls) in enumerate(zip(clauses, classes)):
        f = i % len(SHAPE_LAYOUT)
        op, at = CLASSES[cls][(i // len(SHAPE_LAYOUT) + f) % len(CLASSES[cls])]
        offset, kind, nbytes = SHAPE_LAYOUT[f]
        terms.append((offset, kind, nbytes, op, ORDER[f][at], clause))
    return terms


SHAPES = {}
for _n in (2, 3, 8, 16):
    SHAPES[f"{_n} terms, each its own clause"] = shape_terms(list(range(_n)), ["high"] * _n)
    SHAPES[f"{_n} terms, one clause"] = shape_terms([3] * _n, ["low"] * _n)
SHAPES["3 terms, 2 + 1"] = shape_terms([0, 1, 0], ["quarter", "half", "quarter"])
SHAPES["8 terms, clauses 0, 7 and 15 interleaved"] = shape_terms([0, 7, 15, 0, 7, 15, 0, 7], ["quarter"] * 8)
SHAPES["16 terms, 4 x 4"] = shape_terms([i % 4 for i in range(16)], ["quarter"] * 16)
SHAPES["16 terms, 15 + 1"] = shape_terms([9] * 7 + [2] + [9] * 8, ["low"] * 7 + ["half"] + ["low"] * 8)
THIN_SHAPES = ["3 terms, 2 + 1", "8 terms, clauses 0, 7 and 15 interleaved", "16 terms, each its own clause", "16 terms, 15 + 1"]


def variants(terms, seed):
    """the same list permuted, with its clause numbers renamed, and with one term doubled - but for a list of 16, which has no room for it"""
    rng = np.random.default_rng(seed)
    permuted = [terms[i] for i in rng.permutation(len(terms))]
    names = dict(zip(sorted({t[5] for t in terms}), rng.permutation(16)))
    renamed = [t[:5] + (int(names[t[5]]),) for t in terms]
    k = int(rng.integers(0, len(terms)))
    doubled = terms[:k + 1] + [terms[k]] + terms[k + 1:]
    if len(doubled) > 16:
        return {"permuted": permuted, "renamed": renamed}
    return {"permuted": permuted, "renamed": renamed, "doubled": doubled}


def shape_table(env, turn=0):
    fields_for = drawn_fields(SHAPE_LAYOUT, ORDER, total_of(SHAPE_ROW, SHAPE_ROWS, True), seed=7)
    return table_call(env, SHAPE_ROW, SHAPE_ROWS, fields_for, setting=("lz4", 4, 1), turn=turn, memcpyed=True)


def case_shape(env, name, table, thin=False):
    """one clause shape against numpy, where and aggregate (the binary32 field); then its variants, which must give the same bytes"""
    chunks, rows_plain = table
    terms = SHAPES[name]
    assert_not_vacuous(rows_plain, SHAPE_ROW, terms)
    src = TakeSource(env.mem, chunks=chunks)
    one = check_where(env, src, chunks, rows_plain, SHAPE_ROW, terms, what=name)
    agg = check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], terms, what=name)
    same = variants(terms, seed=len(name))
    if thin:      # the emulator: all three changes in one list
        both = variants(same["renamed"], seed=1)
        same = {"permuted, renamed, doubled": variants(both.get("doubled", both["permuted"]), seed=2)["permuted"]}
    for how, other in same.items():
        assert mask_of(rows_plain, SHAPE_ROW, other).tolist() == mask_of(rows_plain, SHAPE_ROW, terms).tolist()
        assert check_where(env, src, chunks, rows_plain, SHAPE_ROW, other, what=(name, how)) == one, (name, how, "another table")
        assert check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], other, what=(name, how)) == agg, (name, how, "another aggregate")


# ---- case 3: fields ----
def _bf16(x):
    return _f32(x) >> 16


def _f64(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


F32_SET = [_f32(x) for x in (-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0)] + [0x7fc00000, 0xffc00001]      # two NaNs among them
BF16_SET = [_bf16(x) for x in (-2.0, -1.0, 0.0, 0.5, 1.0, 2.0)] + [0x7fc0, 0xff81]
F64_SET = [_f64(x) for x in (-2.0, -1.0, 0.0, 0.5, 1.0, 2.0)] + [0x7ff8 << 48, (0xfff0 << 48) | 1]
I64_SET = [(v << 33) % 2 ** 64 for v in range(-3, 3)]
U8_SET = list(range(6))
I16_SET = [v % 2 ** 16 for v in (-300, -1, 0, 1, 300, 301)]
U32_SET = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1]

# name -> (row_bytes, [(offset, kind, nbytes)], their value sets, terms, the aggregated fields, terms stated to match nothing)
FIELD_CASES = {
    "a range on rows of 4 bytes": (4, [(0, FLOAT, 4)], [F32_SET],
                                   [(0, FLOAT, 4, GE, _f32(-1.0), 0), (0, FLOAT, 4, LT, _f32(2.0), 1)], [(0, FLOAT, 4)], ()),
    "a range with a hole on rows of 4 bytes": (4, [(0, UINT, 4)], [U32_SET],
                                               [(0, UINT, 4, GE, 1, 0), (0, UINT, 4, LE, 2 ** 31 + 1, 1), (0, UINT, 4, NE, 2 ** 31, 2)], [(0, UINT, 4)], ()),
    "mixed kinds in rows of 17 bytes": (17, [(0, UINT, 1), (2, BFLOAT16, 2), (4, FLOAT, 4), (9, INT, 8)], [U8_SET, BF16_SET, F32_SET, I64_SET],
                                        [(0, UINT, 1, GE, 1, 0), (2, BFLOAT16, 2, LT, _bf16(1.0), 1), (4, FLOAT, 4, EQ, _f32(2.0), 1),
                                         (9, INT, 8, NE, I64_SET[1], 2)], [(4, FLOAT, 4), (15, UINT, 2)], ()),
    "rows of 96 bytes, fields at 0, 5 and 88": (96, [(0, UINT, 1), (5, UINT, 4), (88, FLOAT, 8)], [U8_SET, U32_SET, F64_SET],
                                                [(0, UINT, 1, LE, 3, 0), (5, UINT, 4, GT, 2 ** 31 - 1, 1), (88, FLOAT, 8, GE, _f64(0.5), 1),
                                                 (88, FLOAT, 8, NE, _f64(-2.0), 2)], [(88, FLOAT, 8), (5, UINT, 4)], ()),
    # three sectors of 64 bytes (bytes 8 ... 11, 1000 ... 1001, 4072 ... 4079) and a field across the boundary at byte 64
    "rows of 4080 bytes, three sectors and a straddle": (4080, [(8, FLOAT, 4), (1000, INT, 2), (4072, FLOAT, 8), (62, UINT, 4)], [F32_SET, I16_SET, F64_SET, U32_SET],
                                                         [(8, FLOAT, 4, GT, _f32(-2.0), 0), (1000, INT, 2, LT, 300, 1), (4072, FLOAT, 8, LE, _f64(1.0), 2),
                                                          (62, UINT, 4, GE, 2 ** 31, 2)], [(4072, FLOAT, 8)], ()),
    # the NaN rows of every floating-point field: f < c || f >= c are the rows without a NaN
    "f < c or f >= c": (17, [(0, UINT, 1), (2, BFLOAT16, 2), (4, FLOAT, 4), (9, FLOAT, 8)], [U8_SET, BF16_SET, F32_SET, F64_SET],
                        [(4, FLOAT, 4, LT, _f32(0.5), 0), (4, FLOAT, 4, GE, _f32(0.5), 0), (2, BFLOAT16, 2, LT, _bf16(0.5), 1), (2, BFLOAT16, 2, GE, _bf16(0.5), 1),
                         (9, FLOAT, 8, LT, _f64(0.5), 2), (9, FLOAT, 8, GE, _f64(0.5), 2)], [(4, FLOAT, 4)], ()),
    "f != c and f != d": (17, [(0, UINT, 1), (2, BFLOAT16, 2), (4, FLOAT, 4), (9, FLOAT, 8)], [U8_SET, BF16_SET, F32_SET, F64_SET],
                          [(4, FLOAT, 4, NE, _f32(0.5), 0), (4, FLOAT, 4, NE, _f32(-0.0), 1), (2, BFLOAT16, 2, NE, _bf16(2.0), 2), (9, FLOAT, 8, NE, _f64(-1.0), 3)],
                          [(9, FLOAT, 8)], ()),
    "a NaN constant, which matches none, inside an OR clause": (17, [(0, UINT, 1), (2, BFLOAT16, 2), (4, FLOAT, 4), (9, FLOAT, 8)], [U8_SET, BF16_SET, F32_SET, F64_SET],
                                                                [(4, FLOAT, 4, EQ, 0x7fc00000, 0), (2, BFLOAT16, 2, GT, _bf16(0.5), 0), (9, FLOAT, 8, LE, _f64(1.0), 1)],
                                                                [(2, BFLOAT16, 2)], (0,)),
}
FIELD_ROWS = {4: [1025, 0, 700], 17: [1025, 0, 700], 96: [300, 0, 129], 4080: [25, 0, 12]}


def case_fields(env, name, turn=0):
    row_bytes, layout, sets, terms, aggregated, exempt = FIELD_CASES[name]
    rows = FIELD_ROWS[row_bytes]
    memcpyed = MEMCPYED_BYTES % row_bytes == 0 and row_bytes < 4080
    fields_for = drawn_fields(layout, sets, total_of(row_bytes, rows, memcpyed), seed=5)
    chunks, rows_plain = table_call(env, row_bytes, rows, fields_for, setting=("blosclz", 4, 1) if turn % 2 else ("lz4", 8, 1), turn=turn, memcpyed=memcpyed)
    both = assert_not_vacuous(rows_plain, row_bytes, terms, exempt)
    if name == "f < c or f >= c":      # ... exactly the rows in which no tested field holds a NaN, and some rows do
        nan = np.zeros(both.size, bool)
        for offset, kind, nbytes in layout[1:]:
            nan |= np.isnan(W.field_of(rows_plain, row_bytes, offset, kind, nbytes))
        assert np.array_equal(both, ~nan) and nan.any()
    for offset, kind, nbytes in layout:
        if kind in (FLOAT, BFLOAT16):
            assert np.isnan(W.field_of(rows_plain, row_bytes, offset, kind, nbytes)).any(), "a floating-point field without a NaN row"
    batch, packed = both_sources(env, chunks)
    a = check_where(env, batch, chunks, rows_plain, row_bytes, terms, what=name)
    assert check_where(env, packed, chunks, rows_plain, row_bytes, terms, what=(name, "packed")) == a
    for k, fld in enumerate(aggregated):
        check_aggregate(env, packed if k else batch, chunks, rows_plain, row_bytes, fld, terms, what=(name, "aggregated", fld))


# ---- case 4: tile and chunk edges ----
EDGE_ROWS = [1, 63, 64, 0, 65, 1023, 1024, 1025, 2049]      # rows per chunk, a chunk of nbytes 0 among them; a MEMCPYED chunk follows
EDGE_ROW, EDGE_LAYOUT = 8, [(0, UINT, 4), (4, INT, 4)]
HIT_A, MISS_A, HIT_B, MISS_B = 0xDEADBEEF, 0x01020304, (-5) % 2 ** 32, 7
EDGE_TERMS = [(0, UINT, 4, EQ, HIT_A, 0), (4, INT, 4, LT, 0, 1)]
EDGE_DENSITIES = ["none", "every", "row 0", "last row", "chunk edges"]


def case_edges(env, turn=0):
    """chunks of 1 ... 2049 rows in one call, a chunk of nbytes 0 and a MEMCPYED chunk next to them: a range on one field and a second field"""
    total = total_of(EDGE_ROW, EDGE_ROWS, True)
    fields_for = drawn_fields(EDGE_LAYOUT, [U32_SET, [v % 2 ** 32 for v in (-7, -1, 0, 1, 7)]], total, seed=9)
    chunks, rows_plain = table_call(env, EDGE_ROW, EDGE_ROWS, fields_for, turn=turn, memcpyed=True)
    terms = [(0, UINT, 4, GE, 1, 0), (0, UINT, 4, LT, 2 ** 31 + 1, 1), (4, INT, 4, GE, 0, 2)]
    both = assert_not_vacuous(rows_plain, EDGE_ROW, terms)
    first = np.concatenate([[0], np.cumsum(chunk_rows(chunks, EDGE_ROW))])
    assert all(both[first[k]:first[k + 1]].any() for k in range(len(chunks)) if first[k + 1] - first[k] > 1), "a chunk without a match"
    batch, packed = both_sources(env, chunks)
    a = check_where(env, batch, chunks, rows_plain, EDGE_ROW, terms, what="edges")
    assert check_where(env, packed, chunks, rows_plain, EDGE_ROW, terms, what="edges, packed") == a
    check_aggregate(env, batch, chunks, rows_plain, EDGE_ROW, (4, INT, 4), terms, what="edges")
    check_aggregate(env, packed, chunks, rows_plain, EDGE_ROW, (0, UINT, 4), terms, what="edges, packed")


def case_density(env, name, turn=0):
    """A == hit and B < 0 where the rows of the case hold both; elsewhere A alone in one row of five and B alone in one row of seven, so that
    neither term gives the list's table.  "none": no row holds both; "every": every row does"""
    rows = EDGE_ROWS
    nrows = sum(rows)
    firsts = np.concatenate([[0], np.cumsum(rows)])
    both = W.density_patterns(name, nrows, firsts, 1, 0).astype(bool)
    r = np.arange(nrows)
    a = np.where(both | ((r % 5 == 2) & (name != "every")), HIT_A, MISS_A).astype(np.uint64)
    b = np.where(both | ((r % 7 == 3) & (r % 5 != 2) & (name != "every")), HIT_B, MISS_B).astype(np.uint64)
    chunks, rows_plain = table_call(env, EDGE_ROW, rows, lambda f, n: [(0, 4, a[f:f + n]), (4, 4, b[f:f + n])], turn=turn)
    mask = mask_of(rows_plain, EDGE_ROW, EDGE_TERMS)
    assert np.array_equal(mask, both)
    if name not in ("none", "every"):
        assert_not_vacuous(rows_plain, EDGE_ROW, EDGE_TERMS)
    count = {"none": 0, "every": nrows, "row 0": 1, "last row": 1}.get(name)
    assert count is None or int(mask.sum()) == count
    assert name != "chunk edges" or int(mask.sum()) == 2 * (len([n for n in rows if n]) - 1)
    src = TakeSource(env.mem, chunks=chunks) if turn % 2 else TakeSource(env.mem, *(None,) + pack_container(chunks))
    check_where(env, src, chunks, rows_plain, EDGE_ROW, EDGE_TERMS, what=name)
    check_aggregate(env, src, chunks, rows_plain, EDGE_ROW, (4, INT, 4), EDGE_TERMS, what=name)


def case_damage(env, chunk_of, what=""):
    """where_checks.case_damage's kind: a chunk that does not decode between two that do.  Its rows go to unread, its code into the per-chunk
    output, the other chunks answer as if it were not there.  chunk_of(data) -> a typesize-17 chunk of several blocks"""
    from getitem_ranges_checks import pick_damage
    layout = [(3, INT, 4), (9, UINT, 1)]
    rows = W.N // 17
    values = W.value_set(INT, 4)
    good = [chunk_of(make_rows(rows, 17, [(3, 4, W.drawn(values, rows, seed=30 + k)), (9, 1, W.drawn(U8_SET, rows, seed=50 + k))], seed=40 + k)) for k in range(3)]
    rows_plain = plaintext(env.oracle, good)
    found, _ = pick_damage(env.oracle, good[1])
    name, bad = found[0]
    chunks = [good[0], bad, good[2]]
    code = W.decoder_code(env.oracle, bad)
    terms = [(3, INT, 4, NE, values[2], 0), (9, UINT, 1, GE, 2, 1), (9, UINT, 1, EQ, 0, 1)]
    assert_not_vacuous(rows_plain, 17, terms)
    for src in both_sources(env, chunks):
        check_where(env, src, chunks, rows_plain, 17, terms, dead=[(rows, 2 * rows)], codes={1: code}, what=(what, name))
        check_aggregate(env, src, chunks, rows_plain, 17, (3, INT, 4), terms, dead={1: code}, what=(what, name))


# ---- cases 5 ... 8: capacity, passes, a caller's stream, the overlap rule ----
PLAIN_TERMS = SHAPES["3 terms, 2 + 1"]


def case_capacity(env, table):
    """capacity 0 with a NULL table, 1, total - 1, total, total + 5: the prefix exact, everything from min(total, capacity) on untouched (and
    the sentinel words around the table: run_where), the counts the same in all of them"""
    chunks, rows_plain = table
    total = int(assert_not_vacuous(rows_plain, SHAPE_ROW, PLAIN_TERMS).sum())
    assert total > 8
    for n, src in enumerate(both_sources(env, chunks)):
        outs = [check_where(env, src, chunks, rows_plain, SHAPE_ROW, PLAIN_TERMS, capacity=cap, what="capacity")[1]
                for cap in (0, 1, total - 1, total, total + 5)[:5 if n == 0 else 3]]
        assert all(o == outs[0] for o in outs)


def case_passes(env, table):
    """the same call under a pass bound of 16 KiB - every chunk a pass of its own - and under the default gives the same bytes"""
    chunks, rows_plain = table
    assert_not_vacuous(rows_plain, SHAPE_ROW, PLAIN_TERMS)
    for src in both_sources(env, chunks):
        one = check_where(env, src, chunks, rows_plain, SHAPE_ROW, PLAIN_TERMS, what="default bound")
        agg = check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], PLAIN_TERMS, what="default bound")
        env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            assert check_where(env, src, chunks, rows_plain, SHAPE_ROW, PLAIN_TERMS, what="16 KiB passes") == one
            assert check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], PLAIN_TERMS, what="16 KiB passes") == agg
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)


def case_stream(env, table, stream):
    """a caller's stream and the NULL stream give the same bytes"""
    chunks, rows_plain = table
    for src in both_sources(env, chunks):
        assert (check_where(env, src, chunks, rows_plain, SHAPE_ROW, PLAIN_TERMS, stream=stream, what="side stream")
                == check_where(env, src, chunks, rows_plain, SHAPE_ROW, PLAIN_TERMS, what="NULL stream"))
        assert (check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], PLAIN_TERMS, stream=stream, what="side stream")
                == check_aggregate(env, src, chunks, rows_plain, SHAPE_ROW, SHAPE_LAYOUT[3], PLAIN_TERMS, what="NULL stream"))


def case_overlap(env):
    """index_out inside a source chunk, and inside the container in the padding between two chunks: refused, nothing written"""
    good = orc_compress(env.oracle, plain(W.N), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    table, n = terms_table(env.pkg, [(4, UINT, 4, NE, 0, 0), (0, UINT, 1, GE, 1, 1)])
    mem = env.mem
    for src in (TakeSource(mem, chunks=[good, good]), TakeSource(mem, *(None,) + pack_container([good, good], align=4096))):
        before = np.array(mem.get(src.keep[0] if src.packed else src.keep[1][0]), copy=True)
        base = src.container + src.offsets[1] - 64 if src.packed else src.ptrs[1] + 64
        base += (-base) % 8
        for cap in (4, 1):
            out = W.Outputs(2)
            rc = raw_where(env.lib, src, 16, table, n, base, cap, out)
            assert rc < 0 and out.untouched(rows_too=True), ("overlap", src.packed, rc, list(out.rows))
        assert np.array_equal(before, mem.get(src.keep[0] if src.packed else src.keep[1][0])), "the source was written"
