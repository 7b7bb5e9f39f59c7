"""What tests/test_gpu_aggregate.py (device) and tests/test_emu_aggregate.py (wavefront emulator) both assert about the calls of
include/blosc_gpu_aggregate.h, and the cases they run.  Expected answers never come from the library under test: the plaintext of every chunk
is the oracle's orc_decompress (take_checks.plaintext), the field view is where_checks.field_of, the filter's mask is the numpy comparison of
where_checks.expected, count and nans are numpy's, min and max numpy's over the selected values that are no NaN with the first index that
attains them, integer sums numpy's with dtype uint64 / int64 (which wraps as the contract does), and a floating-point sum is math.fsum: equal
where every partial sum is exact, else within the bound of n - 1 binary64 additions in any order, n u A / (1 - n u) with u = 2^-53 and
A = fsum(|x|), computed in fractions.Fraction.  The tables are where_checks' (make_table, drawn, value_set, where_chunks, table_call, table16,
neighbour_set); the exact-sum windows (WINDOWS) put every finite value of binary16 and bfloat16, and binary32 over all its exponent fields,
through the widening and the additions, with the precondition of an exact sum asserted in integers before each call (assert_exact_window).
On top of that every chunk's floating-point sum, in every case, is held bit for bit against tree_sum: a numpy model of the order of additions
that the header documents, written from its text (check_tree; tests/test_aggregate_tree_model.py is about the model itself)."""
import ctypes as C
import math
import struct
from fractions import Fraction

import numpy as np

from getitem_ranges_checks import plain
from helpers import header, orc_compress
from take_checks import N, TakeSource, chunk_rows, pack_container, plaintext
from test_emu_take import SETTINGS  # noqa: F401  (re-exported to the test files)
from where_checks import (BFLOAT16, FLOAT, INT, INT_SENTINEL, KINDS, KINDS16, LAYOUTS, LAYOUTS16, MANTISSA, NEIGHBOUR_KINDS, OPS, SIZE_SENTINEL,  # noqa: F401
                          UINT, Env, both_sources, comparable, constants16, decoder_code, drawn, field_of, kind_name, make_table, neighbour_set,
                          predicate, regime, table16, table_call, thin_constants16, thin_neighbour_picks, total_rows, value_set, where_chunks)

SENTINEL = 0xA5
EQ, NE, LT, LE, GT, GE = range(6)
U = Fraction(1, 2 ** 53)


# ---- one call ----
class Outputs:
    """the host outputs of one call, filled with sentinels - the two structs included"""
    def __init__(self, pkgmod, nchunks):
        self.n = nchunks
        self.total = pkgmod.Aggregate()
        self.chunks = (pkgmod.Aggregate * max(nchunks, 1))()
        C.memset(C.byref(self.total), SENTINEL, C.sizeof(self.total))
        C.memset(self.chunks, SENTINEL, C.sizeof(self.chunks))
        self.status = (C.c_int * max(nchunks, 1))(*[INT_SENTINEL] * max(nchunks, 1))
        self.rows = (C.c_int * max(nchunks, 1))(*[INT_SENTINEL] * max(nchunks, 1))
        self.unread = C.c_size_t(SIZE_SENTINEL)

    def untouched(self, rows_too=False):
        return (bytes(self.total) == bytes([SENTINEL]) * 64 and bytes(self.chunks) == bytes([SENTINEL]) * C.sizeof(self.chunks)
                and self.unread.value == SIZE_SENTINEL and all(s == INT_SENTINEL for s in self.status)
                and (not rows_too or all(r == INT_SENTINEL for r in self.rows)))


def nchunks_of(source):
    return len(source.offsets) - 1 if source.packed else len(source.ptrs)


def raw_call(lib, source, row_bytes, fld, flt, out, stream=None):
    """blosc_gpu_aggregate_batch or _packed, as `source` (a take_checks.TakeSource) says; flt None: no filter"""
    f = C.byref(flt) if flt is not None else None
    if source.packed:
        return lib.blosc_gpu_aggregate_packed(out.n, source.container, source.size, (C.c_size_t * (out.n + 1))(*source.offsets), row_bytes, C.byref(fld), f,
                                              C.byref(out.total), out.chunks, out.status, out.rows, C.byref(out.unread), stream)
    return lib.blosc_gpu_aggregate_batch(out.n, (C.c_void_p * max(out.n, 1))(*source.ptrs), row_bytes, C.byref(fld), f, C.byref(out.total), out.chunks,
                                         out.status, out.rows, C.byref(out.unread), stream)


def entry(a):
    """the 64 bytes of a blosc_gpu_aggregate as a tuple: rows, count, nans, min_row, max_row, min[8], max[8], the sum's 64 bits"""
    return (int(a.rows), int(a.count), int(a.nans), int(a.min_row), int(a.max_row), bytes(a.min), bytes(a.max), int(a.sum.u))


NOTHING = (0, 0, 0, -1, -1, bytes(8), bytes(8), 0)


def as_f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def fold(entries, kind, nbytes):
    """the left fold of the header: rows, counts and sums added (binary64, or modulo 2^64), the smaller min and the larger max win, the
    earlier chunk on a tie"""
    rows = count = nans = total = 0
    low = high = (-1, bytes(8))
    value = lambda raw: comparable([int.from_bytes(raw[:nbytes], "little")], kind, nbytes)[0]
    for e in entries:
        rows, count, nans = rows + e[0], count + e[1], nans + e[2]
        if kind in (FLOAT, BFLOAT16):
            total = struct.unpack("<Q", struct.pack("<d", as_f64(total) + as_f64(e[7])))[0]
        else:
            total = (total + e[7]) % 2 ** 64
        if e[3] >= 0 and (low[0] < 0 or value(e[5]) < value(low[1])): low = (e[3], e[5])
        if e[4] >= 0 and (high[0] < 0 or value(e[6]) > value(high[1])): high = (e[4], e[6])
    return (rows, count, nans, low[0], high[0], low[1], high[1], total)


# ---- numpy's answer ----
def float_sum(x):
    """what the sum of these binary64 values is to be: ("nan",), ("inf", the infinity), or ("finite", fsum(x), the bound of n - 1 additions)"""
    pos, neg = bool(np.any(x == np.inf)), bool(np.any(x == -np.inf))
    if pos and neg: return ("nan",)
    if pos or neg: return ("inf", math.inf if pos else -math.inf)
    s, a, n = math.fsum(x.tolist()), math.fsum(np.abs(x).tolist()), int(x.size)
    return ("finite", s, n * U * Fraction(a) / (1 - n * U))


def expected_of(vals, raw, mask, kind, nbytes, first_row):
    """numpy's answer for rows whose field is vals (comparable) / raw (unsigned patterns), of which `mask` pass the filter, as entry() has it,
    the sum as what check_sum reads"""
    isnan = np.isnan(vals) if kind in (FLOAT, BFLOAT16) else np.zeros(vals.size, bool)
    sel = mask & ~isnan
    at = np.flatnonzero(sel)
    low = high = (-1, bytes(8))
    if at.size:
        v = vals[at]
        lo, hi = int(at[np.argmax(v == v.min())]), int(at[np.argmax(v == v.max())])      # the first index that attains them
        low = (first_row + lo, int(raw[lo]).to_bytes(nbytes, "little") + bytes(8 - nbytes))
        high = (first_row + hi, int(raw[hi]).to_bytes(nbytes, "little") + bytes(8 - nbytes))
    if kind == UINT: total = int(raw[at].astype(np.uint64).sum(dtype=np.uint64))
    elif kind == INT: total = int(vals[at].astype(np.int64).sum(dtype=np.int64)) % 2 ** 64
    else: total = float_sum(vals[at].astype(np.float64))
    return (int(vals.size), int(mask.sum()), int((mask & isnan).sum()), low[0], high[0], low[1], high[1], total)


TILE_ROWS, LANES, WAVE = 1024, 256, 64      # the header's: tiles of 1024 rows, 256 lanes in four waves of 64


def tree_fold(acc):
    """[m, 256] lane accumulators -> [m]: every wave of 64 lanes folded by the butterfly - l with l ^ 32, ^ 16, ... ^ 1, the lower lane's operand
    in front, which for the lanes that end in lane 0 is v[:d] + v[d:2 d] - then the four waves in their order"""
    v = acc.reshape(-1, LANES // WAVE, WAVE)
    d = WAVE // 2
    while d >= 1:
        v = v[:, :, :d] + v[:, :, d:2 * d]
        d //= 2
    w = v[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def tree_sum(x):
    """The binary64 sum of one chunk in the order that include/blosc_gpu_aggregate.h documents, written from its text: x holds the binary64
    values of the chunk's rows in row order, with +0.0 in the place of every row that fails the filter or holds a NaN.  Tiles of 1024 rows;
    lane l of 256 adds rows l, l + 256, l + 512, l + 768 of its tile; tree_fold; over the tiles lane l adds the partials of tiles l, l + 256,
    ... ascending; tree_fold again.
    The rows behind the chunk's last one and the lanes without a tile are +0.0, and that is exact: an accumulator that starts at +0.0 never
    becomes -0.0 under round-to-nearest (+0 + -0 = +0, x + -x = +0, and no sum of two values that are not both -0 rounds to -0), so
    acc + 0.0 has acc's bits - leaving an addition out and adding +0.0 are the same."""
    x = np.asarray(x, np.float64)
    ntiles = max(-(-x.size // TILE_ROWS), 1)
    rows = np.zeros(ntiles * TILE_ROWS)
    rows[:x.size] = x
    rows = rows.reshape(ntiles, TILE_ROWS // LANES, LANES)
    with np.errstate(invalid="ignore", over="ignore"):      # (+inf and -inf meet as a NaN, an overflow is an infinity: IEEE, as the header has it)
        acc = np.zeros((ntiles, LANES))
        for step in range(TILE_ROWS // LANES):
            acc = acc + rows[:, step, :]
        partial = tree_fold(acc)
        turns = -(-ntiles // LANES)
        tiles = np.zeros(turns * LANES)
        tiles[:ntiles] = partial
        tiles = tiles.reshape(turns, LANES)
        acc = np.zeros((1, LANES))
        for turn in range(turns):
            acc = acc + tiles[turn]
        return float(tree_fold(acc)[0])


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def check_tree(got_bits, model, what):
    """a chunk's sum against tree_sum's: a NaN for a NaN (payload and sign differ between hosts and the device), two zeros with ==, every
    other value bit for bit"""
    got = as_f64(got_bits)
    if math.isnan(model): assert math.isnan(got), (what, "sum", got, "the tree gives a NaN")
    elif model == 0 and got == 0: pass
    else: assert got_bits == f64_bits(model), (what, "sum: not the documented order of additions", got, model, hex(got_bits), hex(f64_bits(model)))


def check_sum(got_bits, want, exact, what):
    if not isinstance(want, tuple):
        assert got_bits == want, (what, "sum", got_bits, want)
        return
    got = as_f64(got_bits)
    if want[0] == "nan": assert math.isnan(got), (what, "sum", got, "a NaN")
    elif want[0] == "inf": assert got == want[1], (what, "sum", got, want[1])
    elif exact: assert got == want[1], (what, "sum", got, want[1])      # (== : the sign of a zero sum is unspecified)
    else: assert math.isfinite(got) and abs(Fraction(got) - Fraction(want[1])) <= want[2], (what, "sum", got, want[1], float(want[2]))


def check_entry(got, want, exact, what):
    assert got[:7] == want[:7], (what, got, want)
    check_sum(got[7], want[7], exact, what)


def filter_mask(rows_plain, row_bytes, filter_args):
    if filter_args is None:
        return np.ones(rows_plain.size // row_bytes, bool)
    offset, kind, nbytes, op, constant = filter_args
    with np.errstate(invalid="ignore"):
        return np.asarray(OPS[op](field_of(rows_plain, row_bytes, offset, kind, nbytes), comparable([constant], kind, nbytes)[0]))


def check_aggregate(env, source, chunks, rows_plain, row_bytes, field_args, filter_args=None, dead=None, stream=None, exact=False, what=""):
    """one call against numpy: the answer 0, chunk_rows_out, chunk_status_out (dead: {chunk: the decoder's answer}), unread, every chunk_out[i]
    and total_out; and total_out is the left fold of chunk_out bit for bit.  Returns (entry of the total, entries of the chunks)"""
    offset, kind, nbytes = field_args
    out = Outputs(env.pkg, nchunks_of(source))
    fld = env.pkg.field(kind, nbytes, offset=offset)
    flt = predicate(env.pkg, filter_args[1], filter_args[2], filter_args[3], filter_args[4], filter_args[0]) if filter_args is not None else None
    rc = raw_call(env.lib, source, row_bytes, fld, flt, out, stream)
    what = (what, "row_bytes", row_bytes, "field", offset, kind_name(kind, nbytes), "filter", filter_args)
    assert rc == 0, (what, rc)
    dead = dead or {}
    rows = chunk_rows(chunks, row_bytes)
    first = np.concatenate([[0], np.cumsum(rows)])
    assert list(out.rows)[:out.n] == rows, (what, list(out.rows))
    assert list(out.status)[:out.n] == [dead.get(k, 0) for k in range(out.n)], (what, "status", list(out.status))
    assert out.unread.value == sum(rows[k] for k in dead), (what, "unread", out.unread.value)
    vals, raw = field_of(rows_plain, row_bytes, offset, kind, nbytes), field_of(rows_plain, row_bytes, offset, UINT, nbytes)
    mask = filter_mask(rows_plain, row_bytes, filter_args)
    got = [entry(out.chunks[k]) for k in range(out.n)]
    live = np.ones(vals.size, bool)
    for k in range(out.n):
        lo, hi = int(first[k]), int(first[k + 1])
        if k in dead or lo == hi:
            assert got[k] == NOTHING, (what, "chunk", k, got[k])
            live[lo:hi] = False
            continue
        check_entry(got[k], expected_of(vals[lo:hi], raw[lo:hi], mask[lo:hi], kind, nbytes, lo), exact, (what, "chunk", k))
        if kind in (FLOAT, BFLOAT16):      # ... and the order of the additions is the header's
            with np.errstate(invalid="ignore"):      # (a signalling NaN on its way to binary64)
                x = vals[lo:hi].astype(np.float64)
            check_tree(got[k][7], tree_sum(np.where(mask[lo:hi] & ~np.isnan(x), x, 0.0)), (what, "chunk", k))
    total = entry(out.total)
    at = np.flatnonzero(live)
    want = expected_of(vals[at], raw[at], mask[at], kind, nbytes, 0)
    want = want[:3] + (int(at[want[3]]) if want[3] >= 0 else -1, int(at[want[4]]) if want[4] >= 0 else -1) + want[5:]
    check_entry(total, want, exact, (what, "total"))
    assert total == fold(got, kind, nbytes), (what, "the total is not the left fold of the chunks", total, fold(got, kind, nbytes))
    return total, got


def check_failure(env, source, row_bytes, fld, flt, want_rows, what=""):
    """a call that the census refuses: a negative answer, chunk_rows_out holds want_rows, every other output keeps its sentinel"""
    out = Outputs(env.pkg, nchunks_of(source))
    rc = raw_call(env.lib, source, row_bytes, fld, flt, out)
    assert rc < 0 and out.untouched(), (what, rc, "something was written")
    assert list(out.rows)[:out.n] == want_rows, (what, list(out.rows), want_rows)


# ---- the cases: env is where_checks.Env with declare_aggregate done ----
def make_env(pkg, lib, mem, oracle, writer):
    env = Env(pkg, lib, mem, oracle, writer)
    pkg.declare_aggregate(lib)
    return env


def filters_of(kind, nbytes, values, thin=False):
    """case 1's filters on the aggregated field: none; for the floating-point sets LT +inf and GT -inf, which take one infinity out each, then
    NE -0, EQ NaN (nothing) and NE NaN (every row); for the integers GE, NE and LT against set members"""
    if kind in (FLOAT, BFLOAT16):
        picks = [None, (LT, values[4]), (GT, values[5]), (NE, values[3]), (EQ, values[0]), (NE, values[1])]
        return picks[:3] if thin else picks
    picks = [None, (GE, values[2]), (NE, values[0]), (LT, values[3])]
    return picks[:2] if thin else picks


def case_kind(env, kind, nbytes, setting, turn=0, thin=False):
    """case 1: a field of this kind and width at offset 3 of rows of 17 bytes, drawn from where's value set, unfiltered and filtered on itself"""
    values = value_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, (17, 3, kind, nbytes), drawn(values, total_rows(17, setting[3])), turn)
    src = TakeSource(env.mem, chunks=chunks)
    for pick in filters_of(kind, nbytes, values, thin):
        flt = None if pick is None else (3, kind, nbytes, pick[0], pick[1])
        total, _ = check_aggregate(env, src, chunks, rows_plain, 17, (3, kind, nbytes), flt, what=setting)
        if kind in (FLOAT, BFLOAT16):
            got = as_f64(total[7])
            if pick is None: assert math.isnan(got) and total[2] > 0, "both infinities and NaNs are in the table"
            elif pick in ((LT, values[4]), (GT, values[5])): assert got == (-math.inf if pick[0] == LT else math.inf)
            elif pick == (EQ, values[0]): assert total[1] == 0 and total[3] == -1
            elif pick == (NE, values[1]): assert total[1] == total[0]
        elif nbytes == 8 and pick is None:      # the true sum leaves 64 bits
            v = field_of(rows_plain, 17, 3, kind, 8)
            true = sum(int(x) for x in v)
            assert not (0 <= true < 2 ** 64 if kind == UINT else -2 ** 63 <= true < 2 ** 63), "the sum does not wrap"
            assert total[7] == true % 2 ** 64


def case_neighbours(env, kind, nbytes, setting, turn=0, thin=False):
    """case 1 on where's neighbour set of the kind: unfiltered, and under LT c and GT c for every constant c of the set (thin: under two of
    where's thin_neighbour_picks)"""
    values = neighbour_set(kind, nbytes)
    patterns = drawn(values, total_rows(17, setting[3]), seed=6)
    if (kind, nbytes) == (FLOAT, 8):
        # binary64's largest finite value added to itself overflows, and an infinity made on the way meets the table's other one as a NaN:
        # float_sum's answer (an infinity among the values is the sum) holds for additions that do not overflow.  One row of each sign, then
        big, sign = regime(FLOAT, 8)["max_finite"], 1 << 63
        patterns = drawn([v for v in values if v & (sign - 1) != big], patterns.size, seed=6)
        patterns[5], patterns[700] = big, sign | big
    # (binary64: every row of the MEMCPYED chunk has its field set as well - random patterns reach 2^1023)
    chunks, rows_plain = table_call(env, setting, (17, 3, kind, nbytes), patterns, turn, memcpyed_step=1 if (kind, nbytes) == (FLOAT, 8) else 4)
    if kind in (FLOAT, BFLOAT16):
        with np.errstate(invalid="ignore"):      # (a signalling NaN on its way to binary64)
            x = field_of(rows_plain, 17, 3, kind, nbytes).astype(np.float64)
        for one_sign in (x[np.isfinite(x) & (x > 0)], -x[np.isfinite(x) & (x < 0)]):
            assert sum(map(Fraction, one_sign.tolist())) < 2 ** 1024 - 2 ** 970, "the finite values of one sign overflow binary64 on the way"
    src = TakeSource(env.mem, chunks=chunks)
    picks = [None] + (thin_neighbour_picks(kind, nbytes)[:2] if thin else [(op, c) for c in values for op in (LT, GT)])
    for pick in picks:
        flt = None if pick is None else (3, kind, nbytes, pick[0], pick[1])
        check_aggregate(env, src, chunks, rows_plain, 17, (3, kind, nbytes), flt, what=("neighbours", setting))


def neighbour16(kind, constant, op, row_of):
    """(row, pattern) of the maximum under LT constant / the minimum under GT constant in the table of every 16-bit pattern, from the format's
    order alone: the integer next to it; the floating-point key - the magnitude, negated under the sign - next to the constant's, key 0 being
    whichever zero has the lower row.  None: no row (the end of the range, a NaN constant).  row_of[pattern]: the pattern's row"""
    step = -1 if op == LT else 1
    if kind in (UINT, INT):
        v = (constant - 0x10000 if kind == INT and constant >= 0x8000 else constant) + step
        low, high = (0, 0xffff) if kind == UINT else (-0x8000, 0x7fff)
        if not low <= v <= high: return None
        return int(row_of[v % 0x10000]), v % 0x10000
    inf, mag = regime(kind, 2)["inf"], constant & 0x7fff
    key = (-mag if constant & 0x8000 else mag) + step
    if mag > inf or abs(key) > inf: return None
    p = min((0, 0x8000), key=lambda q: row_of[q]) if key == 0 else key if key > 0 else 0x8000 | -key
    return int(row_of[p]), p


def case_patterns16(env, kind, row_layout, constants, turn=0):
    """where's table of every 16-bit pattern: the field under LT c and under GT c for each constant c.  The maximum under LT c and the minimum
    under GT c are c's neighbours in the format's order - asserted against numpy by check_aggregate and against neighbour16"""
    row_bytes, offset = row_layout
    chunks, rows_plain = table16(env, row_layout, turn)
    src = TakeSource(env.mem, chunks=chunks)
    row_of = np.empty(1 << 16, np.int64)
    row_of[field_of(rows_plain, row_bytes, offset, UINT, 2)] = np.arange(1 << 16)
    for constant in constants:
        for op in (LT, GT):
            what = ("every pattern", kind_name(kind, 2), OPS[op].__name__, hex(constant))
            total, _ = check_aggregate(env, src, chunks, rows_plain, row_bytes, (offset, kind, 2), (offset, kind, 2, op, constant), what=what)
            want = neighbour16(kind, constant, op, row_of)
            got = (total[4], total[6]) if op == LT else (total[3], total[5])
            assert got == ((-1, bytes(8)) if want is None else (want[0], want[1].to_bytes(2, "little") + bytes(6))), (what, got, want)


def case_layout(env, layout, setting, turn=0, stream=None):
    """case 2, where's LAYOUTS: the layout's field aggregated, unfiltered and filtered on itself, through both entry points"""
    row_bytes, offset, kind, nbytes = layout
    values = value_set(kind, nbytes)
    chunks, rows_plain = table_call(env, setting, layout, drawn(values, total_rows(row_bytes, setting[3])), turn)
    pick = (LT, values[4]) if kind in (FLOAT, BFLOAT16) else (GE, values[2])
    for flt in (None, (offset, kind, nbytes) + pick):
        a, b = (check_aggregate(env, s, chunks, rows_plain, row_bytes, (offset, kind, nbytes), flt, stream=stream, what=(n, setting))
                for n, s in zip(("batch", "packed"), both_sources(env, chunks)))
        assert a == b, "batch and packed differ"


# (row_bytes, the float field: offset and bytes, the integer field: offset, kind and bytes)
TWO_FIELDS = [(12, (1, 4), (7, UINT, 2)), (96, (3, 8), (89, INT, 4))]


def case_other_field(env, two, setting, turn=0):
    """case 2: a float field aggregated under a filter on an integer field at another, unaligned offset - and the other way round"""
    row_bytes, (foff, fbytes), (ioff, ikind, ibytes) = two
    cname, T, shuffle, scale = setting
    fvalues, ivalues = value_set(FLOAT, fbytes), value_set(ikind, ibytes)
    write = env.writer(cname, T, shuffle, turn)
    chunks = []
    for k, size in enumerate((N * scale, 0, N * scale // 2)):
        if not size:
            chunks.append(orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
            continue
        rows = size // row_bytes
        tab = make_table(rows, row_bytes, foff, fbytes, drawn(fvalues, rows, seed=50 + k), seed=60 + k).reshape(rows, row_bytes)
        tab[:, ioff:ioff + ibytes] = np.ascontiguousarray(drawn(ivalues, rows, seed=70 + k), dtype=f"<u{ibytes}").view(np.uint8).reshape(rows, ibytes)
        chunks.append(write(k, tab.reshape(-1)))
    rows_plain = plaintext(env.oracle, chunks)
    batch, packed = both_sources(env, chunks)
    fargs, iargs = (foff, FLOAT, fbytes), (ioff, ikind, ibytes)
    check_aggregate(env, batch, chunks, rows_plain, row_bytes, fargs, iargs + (NE, ivalues[1]), what="float under an integer filter")
    check_aggregate(env, packed, chunks, rows_plain, row_bytes, fargs, iargs + (EQ, ivalues[2]), what="float under an integer filter")
    check_aggregate(env, batch, chunks, rows_plain, row_bytes, iargs, fargs + (GE, fvalues[2]), what="integer under a float filter")
    check_aggregate(env, packed, chunks, rows_plain, row_bytes, iargs, fargs + (NE, fvalues[0]), what="integer under a float filter")


EDGE_ROWS = [1, 63, 64, 0, 65, 1023, 1024, 1025, 2049]      # rows per chunk of case 3; tiles are 1024 rows, waves 64


def edge_call(env, patterns, turn=0):
    """the chunks of case 3 - rows of 4 bytes that are the field - with these patterns, and their plaintext"""
    write = env.writer("lz4", 4, 1, turn)
    chunks, first = [], 0
    for k, rows in enumerate(EDGE_ROWS):
        data = np.ascontiguousarray(patterns[first:first + rows], dtype="<u4").view(np.uint8)
        chunks.append(write(k, data) if rows else orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += rows
    assert chunk_rows(chunks, 4) == EDGE_ROWS
    return chunks, plaintext(env.oracle, chunks)


def case_edges(env, turn=0):
    """case 3: chunks of 1 ... 2049 rows in one call, a chunk of nbytes 0 among them; the extreme in row 0 of a chunk, in its last row, in the
    last row of a tile, in two rows of different tiles, in two rows of different chunks; -0 in front of +0 and the reverse; a chunk in which no
    row passes the filter; a chunk whose selected values are all NaN"""
    first = np.concatenate([[0], np.cumsum(EDGE_ROWS)])
    nrows, big = int(first[-1]), int(first[-2])      # big: the first row of the chunk of 2049 rows
    rng = np.random.default_rng(17)
    base = rng.integers(-100, 101, nrows).astype(np.int32)
    places = {"row 0 of a chunk": [big], "the last row of a chunk": [big + 2048], "the last row of a tile": [big + 1023],
              "two tiles": [big + 1500, big + 700], "two chunks": [big + 5, int(first[-3]) + 1024], "a chunk of one row": [0]}
    for name, at in places.items():
        p = base.copy()
        p[at] = 1000
        p[[r ^ 1 for r in at]] = -1000      # the minimum right next to each
        chunks, rows_plain = edge_call(env, p.view(np.uint32), turn)
        for src in both_sources(env, chunks):
            total, per_chunk = check_aggregate(env, src, chunks, rows_plain, 4, (0, INT, 4), what=name)
            assert total[4] == min(at) and total[3] == min(r ^ 1 for r in at) and total[6][:4] == (1000).to_bytes(4, "little"), (name, total)
        total, _ = check_aggregate(env, src, chunks, rows_plain, 4, (0, INT, 4), (0, INT, 4, GT, (-1000) % 2 ** 32), what=(name, "filtered"))
        assert total[4] == min(at) and total[3] != min(r ^ 1 for r in at)
    # floating point: positive values, the two zeros in different tiles of the last chunk; the chunk of 64 rows negative (no row passes GT 0),
    # the chunk of 65 rows all NaN
    f = rng.integers(1, 200, nrows).astype(np.float32) * np.float32(0.5)
    f[int(first[2]):int(first[3])] *= -1
    f[int(first[4]):int(first[5])] = np.nan
    minus, plus = np.float32(-0.0), np.float32(0.0)
    for name, (early, late) in {"-0 in front of +0": (minus, plus), "+0 in front of -0": (plus, minus)}.items():
        p = f.copy()
        p[big + 300], p[big + 1900] = early, late
        chunks, rows_plain = edge_call(env, p.view(np.uint32), turn + 1)
        src = TakeSource(env.mem, chunks=chunks)
        total, per_chunk = check_aggregate(env, src, chunks, rows_plain, 4, (0, FLOAT, 4), what=name)
        assert per_chunk[-1][3] == big + 300 and per_chunk[-1][5][:4] == early.tobytes(), (name, per_chunk[-1])
        assert per_chunk[4][1:5] == (65, 65, -1, -1) and per_chunk[4][7] == 0, ("all NaN", per_chunk[4])
        total, per_chunk = check_aggregate(env, src, chunks, rows_plain, 4, (0, FLOAT, 4), (0, FLOAT, 4, GT, 0), what=(name, "GT 0"))
        assert per_chunk[2] == (64, 0, 0, -1, -1, bytes(8), bytes(8), 0) and per_chunk[4][:3] == (65, 0, 0), ("no row passes", per_chunk[2], per_chunk[4])
        total, per_chunk = check_aggregate(env, src, chunks, rows_plain, 4, (0, FLOAT, 4), (0, FLOAT, 4, LE, 0), what=(name, "LE 0"))
        assert total[4] == big + 300 and total[6][:4] == early.tobytes() and int(first[2]) <= total[3] < int(first[3]), (name, "the maximum is the earlier zero", total)


def case_many_tiles(env, thin=False):
    """case 4: where's 320 000 rows of one byte in four chunks - tile counts that are no power of two, chunk ends inside tiles - as uint8 and as
    int8, unfiltered and filtered"""
    sizes = [120001, 0, 119999, 80000]
    pats = drawn(value_set(UINT, 1), sum(sizes), seed=9)
    write = env.writer("lz4", 4, 1, 0)
    chunks, first = [], 0
    for size in sizes:
        chunks.append(write(0, make_table(size, 1, 0, 1, pats[first:first + size])) if size else orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += size
    rows_plain = plaintext(env.oracle, chunks)
    src = TakeSource(env.mem, chunks=chunks)
    runs = [(UINT, (0, UINT, 1, GE, 1))] if thin else [(UINT, None), (UINT, (0, UINT, 1, GE, 1)), (INT, None), (INT, (0, INT, 1, LT, 1))]
    for kind, flt in runs:
        total, _ = check_aggregate(env, src, chunks, rows_plain, 1, (0, kind, 1), flt, what="many tiles")
        assert sum(sizes) // 3 < total[1] <= sum(sizes)


# ---- case 5: the float sum ----
FLOATS = [(FLOAT, 2), (BFLOAT16, 2), (FLOAT, 4), (FLOAT, 8)]
SMALLEST = {(FLOAT, 2): -24, (BFLOAT16, 2): -133, (FLOAT, 4): -149, (FLOAT, 8): -1074}      # the smallest subnormal: 2^this


def patterns_of(x, kind, nbytes):
    """the patterns of binary64 values that the format holds exactly"""
    x = np.asarray(x, np.float64)
    if kind == BFLOAT16:
        bits = x.astype(np.float32).view(np.uint32)
        assert not np.any(bits & 0xffff)
        p = (bits >> 16).astype(np.uint64)
    else:
        p = x.astype(f"<f{nbytes}").view(f"<u{nbytes}").astype(np.uint64)
    assert np.array_equal(comparable(p, kind, nbytes).astype(np.float64), x), "the format does not hold these values"
    return p


def sum_call(env, patterns, nbytes, turn=0):
    """rows of 12 bytes with the field at offset 3, in chunks of 3/8, none, 1/2 and 1/8 of the rows"""
    n = patterns.size
    sizes = [n * 3 // 8, 0, n // 2]
    sizes.append(n - sum(sizes))
    write = env.writer("lz4", 4, 1, turn)
    chunks, first = [], 0
    for k, rows in enumerate(sizes):
        chunks.append(write(k, make_table(rows, 12, 3, nbytes, patterns[first:first + rows], seed=80 + k)) if rows
                      else orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += rows
    return chunks, plaintext(env.oracle, chunks)


def case_sum_exact(env, kind, nbytes, nrows, turn=0):
    """values k / 2 with |k| <= 255, which all four formats hold: at most 2^20 of them, so every partial sum in any order is an exact binary64
    and the result equals math.fsum"""
    assert nrows <= 2 ** 20
    k = np.random.default_rng(31).integers(-255, 256, nrows)
    chunks, rows_plain = sum_call(env, patterns_of(k / 2.0, kind, nbytes), nbytes, turn)
    src = TakeSource(env.mem, chunks=chunks)
    total, _ = check_aggregate(env, src, chunks, rows_plain, 12, (3, kind, nbytes), exact=True, what="exact")
    assert as_f64(total[7]) == math.fsum((k / 2.0).tolist())
    check_aggregate(env, src, chunks, rows_plain, 12, (3, kind, nbytes), (3, kind, nbytes, GT, int(patterns_of([-3.5], kind, nbytes)[0])), exact=True,
                    what="exact, filtered")


def case_sum_subnormals(env, kind, nbytes, nrows, turn=0):
    """a column of the format's smallest subnormal: count x that value, exact in binary64 - a flushed denormal gives 0"""
    chunks, rows_plain = sum_call(env, np.ones(nrows, np.uint64), nbytes, turn)
    total, _ = check_aggregate(env, TakeSource(env.mem, chunks=chunks), chunks, rows_plain, 12, (3, kind, nbytes), exact=True, what="subnormals")
    assert total[1] == nrows and as_f64(total[7]) == math.ldexp(nrows, SMALLEST[(kind, nbytes)]) > 0


# ---- exact-sum windows: every value of a format widened and added ----
def assert_exact_window(patterns, kind, nbytes):
    """The precondition of an exact sum, in integers and fractions, for all the rows of a call: every value is finite and a multiple of
    2^q, and n max|x| < 2^(q + 53).  Then every sum of any of the values, in any order, is a multiple of 2^q below 2^(q + 53) - a binary64 -
    so the kernel's tree, the host's fold and math.fsum agree bit for bit.  Returns q"""
    x = comparable(patterns, kind, nbytes).astype(np.float64)
    assert np.all(np.isfinite(x)), "a window holds finite values"
    values = [Fraction(v) for v in x.tolist() if v]
    assert values, "a window of zeros"
    # the 2-adic valuation of a dyadic rational num / 2^k: the trailing zeros of num, less k
    q = min((f.numerator & -f.numerator).bit_length() - f.denominator.bit_length() for f in values)
    unit = Fraction(2) ** q
    assert all((f / unit).denominator == 1 for f in values)
    assert int(x.size) * max(abs(f) for f in values) < unit * 2 ** 53, ("the window's sums may round", int(x.size), q)
    return q


def windows_f16():
    """all 63 488 finite binary16 patterns in a seeded permutation, as 8 windows of 7 936 rows (q = -24, max 65 504: n < 2^13 suffices)"""
    p = np.arange(1 << 16, dtype=np.uint64)
    p = np.random.default_rng(51).permutation(p[(p & 0x7c00) != 0x7c00])
    assert p.size == 63488
    return [p[7936 * w:7936 * (w + 1)] for w in range(8)]


def windows_bf16():
    """all finite bfloat16 patterns in 8 windows by exponent field, e // 32 = 0 ... 7 without e = 255: 8 192 rows each, 7 936 in the last"""
    p = np.arange(1 << 16, dtype=np.uint64)
    e = (p >> np.uint64(7)) & np.uint64(0xff)
    rng = np.random.default_rng(52)
    out = [rng.permutation(p[(e // np.uint64(32) == w) & (e != 255)]) for w in range(8)]
    assert [w.size for w in out] == [8192] * 7 + [7936]
    return out


def window_f32(w, nrows=8000):
    """window w = 0 ... 14 of binary32: the 17 exponent fields 17 w ... 17 w + 16, both signs.  n 2^(e_min + 17) < 2^(e_min - 23 + 53) gives
    n < 2^13.  For every exponent field and sign the mantissas 0, all ones and every single bit; the rest random.  In window 0 half of the
    rows have exponent field 0: for every leading-bit position p of a subnormal 1 << p, (1 << (p + 1)) - 1 and a random pattern with that
    leading bit, then random ones with a random leading bit"""
    rng = np.random.default_rng(530 + w)
    e_min = 17 * w
    mants = [0, (1 << 23) - 1] + [1 << k for k in range(23)]
    rows = [(s << 31) | (e << 23) | m for e in range(e_min, e_min + 17) for s in (0, 1) for m in mants]
    if w == 0:
        def below(p):      # a random pattern whose leading bit is bit p
            return (1 << p) | int(rng.integers(0, 1 << p))
        rows += [(s << 31) | m for p in range(23) for s in (0, 1) for m in (1 << p, (1 << (p + 1)) - 1, below(p))]
        have = sum(1 for r in rows if not (r >> 23) & 0xff)
        rows += [(int(rng.integers(0, 2)) << 31) | below(int(rng.integers(0, 23))) for _ in range(nrows // 2 - have)]
    n = nrows - len(rows)
    e = rng.integers(max(e_min, 1) if w == 0 else e_min, e_min + 17, n).astype(np.uint64)
    rows = np.concatenate([np.array(rows, dtype=np.uint64), (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(31)) | (e << np.uint64(23))
                           | rng.integers(0, 1 << 23, n).astype(np.uint64)])
    assert rows.size == nrows and (w != 0 or int(((rows >> np.uint64(23)) & np.uint64(0xff) == 0).sum()) == nrows // 2)
    return rng.permutation(rows)


def window_f64(nrows=8000):
    """binary64 subnormals below 2^39 units, both signs: widening is the identity, the window is about the device's additions of subnormals"""
    rng = np.random.default_rng(54)
    return rng.integers(1, 1 << 39, nrows).astype(np.uint64) | (rng.integers(0, 2, nrows).astype(np.uint64) << np.uint64(63))


F32_WINDOWS = 15
WINDOWS = {(FLOAT, 2): lambda: windows_f16(), (BFLOAT16, 2): lambda: windows_bf16(), (FLOAT, 4): lambda: [window_f32(w) for w in range(F32_WINDOWS)],
           (FLOAT, 8): lambda: [window_f64()]}
THREE_WAYS = (None, GT, LT)      # unfiltered, the positive values alone, the negative values alone: no two wrong values cancel in all three


def case_sum_window(env, kind, nbytes, patterns, ways=THREE_WAYS, turn=0, what=""):
    """one window through sum_call: the precondition asserted for the whole call before it is made, then every chunk's sum and the call's
    compared with == against math.fsum - unfiltered, under GT +0 and under LT +0"""
    assert_exact_window(patterns, kind, nbytes)
    chunks, rows_plain = sum_call(env, patterns, nbytes, turn)
    assert np.array_equal(field_of(rows_plain, 12, 3, UINT, nbytes).astype(np.uint64), patterns)
    src = TakeSource(env.mem, chunks=chunks)
    for op in ways:
        flt = None if op is None else (3, kind, nbytes, op, 0)
        total, _ = check_aggregate(env, src, chunks, rows_plain, 12, (3, kind, nbytes), flt, exact=True, what=("window", what))
        assert total[2] == 0 and total[1] > 0 and (op is None) == (total[1] == patterns.size)


def rounding_values(nbytes, nrows):
    """values over about 30 binary orders of magnitude, both signs, |x| < 2^100; numpy's own pairwise sum stays within the bound on them"""
    assert nrows <= 2 ** 20
    rng = np.random.default_rng(41)
    x = (rng.uniform(1, 2, nrows) * np.exp2(rng.integers(-10, 21, nrows)) * rng.choice([-1.0, 1.0], nrows)).astype(f"<f{nbytes}").astype(np.float64)
    want = float_sum(x)
    assert want[0] == "finite" and np.abs(x).max() < 2.0 ** 100 and abs(Fraction(float(np.sum(x))) - Fraction(want[1])) <= want[2]
    return x


def case_sum_rounding(env, nbytes, nrows, side_stream=None, turn=0):
    """binary32 / binary64 values whose sum rounds: within the bound of n - 1 additions, and the same 64 bytes bit for bit from two identical
    calls, from batch and packed, under the default pass bound and one of 16 KiB, on the NULL stream and a side stream (where the caller has
    one), and for a chunk aggregated alone and inside the batch"""
    x = rounding_values(nbytes, nrows)
    chunks, rows_plain = sum_call(env, patterns_of(x, FLOAT, nbytes), nbytes, turn)
    batch, packed = both_sources(env, chunks)
    for flt in (None, (3, FLOAT, nbytes, GT, 0)):
        run = lambda src, stream=None, what="": check_aggregate(env, src, chunks, rows_plain, 12, (3, FLOAT, nbytes), flt, stream=stream, what=what)
        one = run(batch, what="rounding")
        assert run(batch, what="again") == one, "two identical calls differ"
        assert run(packed, what="packed") == one, "batch and packed differ"
        env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
        try:
            assert run(batch, what="16 KiB passes") == one and run(packed, what="16 KiB passes, packed") == one, "the pass bound changes the answer"
        finally:
            env.lib.blosc_amd_getitem_pass_bytes(0)
        if side_stream is not None:
            assert run(batch, stream=side_stream, what="side stream") == one, "the stream changes the answer"
        # a chunk in a call of its own: its entry with the two rows offset by its first row
        rows = chunk_rows(chunks, 12)
        for k in (2, 3):
            lo, hi = sum(rows[:k]), sum(rows[:k + 1])
            _, alone = check_aggregate(env, TakeSource(env.mem, chunks=[chunks[k]]), [chunks[k]], rows_plain[12 * lo:12 * hi], 12, (3, FLOAT, nbytes), flt,
                                       what=("alone", k))
            e = alone[0]
            assert e[:3] + (e[3] + lo, e[4] + lo) + e[5:] == one[1][k], ("a chunk alone and inside the batch differ", k, e, one[1][k])


# ---- chunks taller than 256 tiles: a lane of k_aggregate_chunks folds a second and a third tile ----
TALL_ROWS = [262144, 262145, 0, 524289, 1]      # 256 tiles (no lane folds twice), 257, none, 513 (lane 0 folds three), one row


def rounding_pool(size=300, seed=43):
    """binary64 patterns whose sums round in nearly every addition: full random 52-bit mantissas over seven binades around 1, both signs.
    A few hundred of them, for drawn(): the chunks still compress"""
    rng = np.random.default_rng(seed)
    mant = rng.integers(0, 1 << 52, size).astype(np.uint64)
    exp = (1023 + rng.integers(-3, 4, size)).astype(np.uint64)
    return (rng.integers(0, 2, size).astype(np.uint64) << np.uint64(63)) | (exp << np.uint64(52)) | mant


TALL_SEEDS = [24, 15, 12, 33, 12]      # drawn()'s seed of each chunk of TALL_ROWS


def tall_patterns(rows=None, seeds=None):
    """The binary64 field of every row of case_tall_chunks.  A chunk's first half is drawn from the pool; its second half is the first half
    rotated by 333 rows with the signs flipped.  The true sum of a chunk is then zero (or its one odd row), so what a tree of additions
    returns is the rounding errors it made on the way, in full precision: two different trees hardly ever agree.  Under GT +0 nothing
    cancels and about one tree in two agrees with another by chance, which is why each chunk has a seed of its own in TALL_SEEDS:
    tests/test_aggregate_tree_model.py asserts that these inputs separate the documented tree from every rival in both runs."""
    rows, seeds = TALL_ROWS if rows is None else rows, TALL_SEEDS if seeds is None else seeds
    pool, out = rounding_pool(), []
    for n, seed in zip(rows, seeds):
        half = drawn(pool, (n + 1) // 2, seed=seed) if n else np.zeros(0, np.uint64)
        out += [half, np.roll(half, -333)[:n // 2] ^ np.uint64(1 << 63)]
    return np.concatenate(out)


def tall_call(env, patterns, rows, turn=0):
    """rows of 8 bytes that are the field, in chunks of `rows` rows, the writers in turns"""
    write = env.writer("lz4", 8, 1, turn)
    chunks, first = [], 0
    for k, n in enumerate(rows):
        chunks.append(write(k, np.ascontiguousarray(patterns[first:first + n], dtype="<u8").view(np.uint8)) if n
                      else orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1])
        first += n
    assert chunk_rows(chunks, 8) == list(rows)
    return chunks, plaintext(env.oracle, chunks)


def case_tall_chunks(env, rows=None, seeds=None, turn=0, thin=False):
    """chunks of 256, 257 and 513 tiles, an empty one and one of a single row: unfiltered and under GT +0, from both sources and once under a
    pass bound of 16 KiB.  check_aggregate holds every chunk's sum against tree_sum bit for bit - on values that separate the documented
    tree from its neighbours (tests/test_aggregate_tree_model.py)"""
    rows = TALL_ROWS if rows is None else rows
    chunks, rows_plain = tall_call(env, tall_patterns(rows, seeds), rows, turn)
    batch, packed = both_sources(env, chunks)
    for flt in (None, (0, FLOAT, 8, GT, 0)):
        one = check_aggregate(env, batch, chunks, rows_plain, 8, (0, FLOAT, 8), flt, what="tall chunks")
        assert math.isfinite(as_f64(one[0][7])) and one[0][2] == 0
        if thin: return      # (the emulator: one call, unfiltered)
        assert check_aggregate(env, packed, chunks, rows_plain, 8, (0, FLOAT, 8), flt, what="tall chunks, packed") == one, "batch and packed differ"
    env.lib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        assert check_aggregate(env, batch, chunks, rows_plain, 8, (0, FLOAT, 8), flt, what="tall chunks, 16 KiB passes") == one, "the pass bound changes the answer"
    finally:
        env.lib.blosc_amd_getitem_pass_bytes(0)


TALL_PLANTS = (3 * 1024 + 17, 258 * 1024 + 5, 259 * 1024 + 700)      # the minimum: tile 3 (lane 3's first), tile 258 (lane 2's second, folded in front of lane 3), tile 259 (lane 3's second)


def case_tall_extremes(env, kind, turn=0):
    """the chunk of 524 289 rows alone, as binary64 or int64: the minimum in three rows of three tiles that two lanes of the chunk fold meet
    in another order than the rows' - min_row is the lowest; the maximum in the last row, alone in the partial tile 512"""
    nrows = TALL_ROWS[3]
    p = tall_patterns([nrows], [TALL_SEEDS[3]]).copy()
    if kind == FLOAT: low, high = int(patterns_of([-32.0], FLOAT, 8)[0]), int(patterns_of([32.0], FLOAT, 8)[0])      # the pool stays below 16
    else: low, high = 1 << 63, (1 << 63) - 1
    p[list(TALL_PLANTS)], p[nrows - 1] = low, high
    chunks, rows_plain = tall_call(env, p, [nrows], turn)
    total, per_chunk = check_aggregate(env, TakeSource(env.mem, chunks=chunks), chunks, rows_plain, 8, (0, kind, 8), what=("tall extremes", kind_name(kind, 8)))
    assert total == per_chunk[0] and total[3:7] == (TALL_PLANTS[0], nrows - 1, low.to_bytes(8, "little"), high.to_bytes(8, "little")), total[:7]
    if kind == INT:
        true = sum(int(v) for v in field_of(rows_plain, 8, 0, INT, 8))
        assert not -2 ** 63 <= true < 2 ** 63 and total[7] == true % 2 ** 64, "the integer sum wraps on the way"


def case_tall_bytes(env):
    """one chunk of 300 000 rows of one byte (293 tiles) as uint8: count and sum, unfiltered and under GE 1"""
    pats = drawn(value_set(UINT, 1), 300000, seed=13)
    chunks = [env.writer("lz4", 4, 1, 0)(0, make_table(300000, 1, 0, 1, pats))]
    rows_plain = plaintext(env.oracle, chunks)
    src = TakeSource(env.mem, chunks=chunks)
    for flt in (None, (0, UINT, 1, GE, 1)):
        total, _ = check_aggregate(env, src, chunks, rows_plain, 1, (0, UINT, 1), flt, what="tall, one-byte rows")
        assert 100000 < total[1] <= 300000 and total[7] == int(rows_plain[rows_plain >= (1 if flt else 0)].astype(np.uint64).sum())


def case_damage(env, chunk_of, what="", thin=False):
    """case 6: where's construction - a chunk that does not decode between two that do: its status, its zeroed entry, unread, and the totals
    of the other two alone (check_aggregate leaves the dead rows out of numpy's answer)"""
    from getitem_ranges_checks import pick_damage
    values = value_set(INT, 4)
    rows = N // 17
    good = [chunk_of(make_table(rows, 17, 3, 4, drawn(values, rows, seed=30 + k), seed=40 + k)) for k in range(3)]
    rows_plain = plaintext(env.oracle, good)
    found, _ = pick_damage(env.oracle, good[1])
    for name, bad in found[:1 if thin else None]:
        chunks = [good[0], bad, good[2]]
        code = decoder_code(env.oracle, bad)
        for src in both_sources(env, chunks):
            for flt in (None, (3, INT, 4, NE, values[2]))[:1 if src.packed else 2]:
                total, per_chunk = check_aggregate(env, src, chunks, rows_plain, 17, (3, INT, 4), flt, dead={1: code}, what=(what, name))
                assert total[0] == 2 * rows and per_chunk[1] == NOTHING and per_chunk[0][1] > 0 and per_chunk[2][1] > 0


def case_refused(env):
    """case 7: where's three census failures with the code at its place in chunk_rows_out and every other output still holding its sentinel"""
    good = orc_compress(env.oracle, plain(N), 17, 5, 1, "lz4", blocksize=8192)[1]
    odd = orc_compress(env.oracle, plain(N + 8), 17, 5, 1, "lz4", blocksize=8192)[1]
    version = good.copy(); version[0] = 3
    rows = N // 16
    fld, flt = env.pkg.field(UINT, 4, offset=4), predicate(env.pkg, UINT, 4, NE, 0, 4)
    mem = env.mem
    check_failure(env, TakeSource(mem, chunks=[good, odd, good]), 16, fld, None, [rows, -1, rows], "no multiple")
    check_failure(env, TakeSource(mem, chunks=[good, good, version]), 16, fld, flt, [rows, rows, -9], "version")
    check_failure(env, TakeSource(mem, *(None,) + pack_container([version, odd])), 16, fld, flt, [-9, -1], "both, packed")
    offs, parts = [0], []
    for k, c in enumerate([good, good, good]):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    check_failure(env, TakeSource(mem, container=np.concatenate(parts), offsets=offs), 16, fld, None, [rows, -1, rows], "a slot eight bytes short")
