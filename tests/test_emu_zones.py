"""CPU: the calls of include/blosc_gpu_zones.h on the emulated library - blosc_api.hip's openings and the prune rule, engine.hip's widened
aggregate body and RowScan's pruned chunks, k_aggregate_tiles_fields and k_aggregate_chunks_fields.  The checks are those of
tests/test_gpu_zones.py (tests/zones_checks.py), the grid thinned to what the emulator runs in a few minutes."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import NumpyMem
from helpers import orc_compress, ptr, ref_compress
from take_checks import BLOCKSIZE
from test_emu_library import emulib  # noqa: F401  (the fixture)
import clauses_checks as K
import where_checks as W
import zones_checks as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_zones", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def env(emulib, pkgmod, oracle, ref):
    assert hasattr(emulib, "blosc_gpu_where_zoned_batch"), "the library has no zone calls"
    assert hasattr(pkgmod, "declare_zones"), "the loader has no zone calls"

    def lib_compress(data, T, shuffle, cname):
        out = np.zeros(data.size + 16, np.uint8)
        r = emulib.blosc_compress_ctx(5, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname.encode(), BLOCKSIZE, 1)
        assert r > 0
        return out[:r].copy()

    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle, by the reference where it is built, by the emulated library (small chunks), in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 1 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            if who == 2 and data.size <= W.N // 2: return lib_compress(data, T, shuffle, cname)
            return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        return write
    return Z.Env(pkgmod, emulib, NumpyMem(), oracle, writer)


@pytest.fixture(scope="module")
def table20(env):
    """(the device: chunks of clauses_checks.EDGE_ROWS rows; here they come in a test of their own)"""
    return Z.table20(env, rows=[63, 0, 65, 1025, 1])


@pytest.fixture(scope="module")
def zoned_table(env):
    return Z.zoned_table(env)


def test_fields_equal_the_single_field_calls(env, table20):
    """1 and 16 fields with no terms and 16, batch; 2 and 15 fields with one term, packed (the device: every combination)"""
    Z.case_shape_fields(env, table20, counts=(1, 16), lists=("16 terms",), sources=(0,))
    Z.case_shape_fields(env, table20, counts=(2, 15), lists=("one term",), sources=(1,))
    Z.case_shape_fields(env, table20, counts=(2,), lists=("no terms",), sources=(0,))


def test_tile_and_chunk_edges(env):
    """chunks of 1 ... 2049 rows, a chunk of nbytes 0 and a MEMCPYED chunk: 16 fields, every row"""
    chunks, rows_plain = Z.table20(env, turn=1)
    Z.check_fields(env, K.TakeSource(env.mem, chunks=chunks), chunks, rows_plain, K.SHAPE_ROW, Z.nfields_of(K.SHAPE_LAYOUT, 16), [], grounded=(3,), what="edges")


def test_sixteen_fields_of_every_kind(env):
    table = Z.table96(env, [63, 0, 300])
    Z.case_wide_fields(env, table, lists=(0,), sources=(1,))
    Z.case_wide_fields(env, table, lists=(16,), sources=(0,))


def test_fields_a_chunk_that_does_not_decode(env):
    Z.case_fields_damage(env, lambda data: orc_compress(env.oracle, data, 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1], "lz4")


def test_fields_passes_give_the_same(env, table20):
    Z.case_fields_passes(env, table20, sources=(1,))


def test_fields_sums_that_round(env):
    Z.case_fields_rounding(env, rows=[1025, 0, 700])


@pytest.mark.parametrize("family", list(Z.zoned_lists()))
def test_zoned_calls_equal_the_clause_calls(env, zoned_table, family):
    at = list(Z.zoned_lists()).index(family)
    Z.case_zoned_family(env, zoned_table, family, sources=(at % 2,))


def test_zoned_nothing_and_everything(env, zoned_table):
    Z.case_zoned_nothing_and_everything(env, zoned_table)


def test_a_pruned_chunk_is_not_read(env, zoned_table):
    Z.case_zoned_garbage(env, zoned_table)


def test_a_map_of_other_rows_is_refused(env, zoned_table):
    Z.case_zoned_stale_rows(env, zoned_table)


def test_zoned_capacity_and_passes(env, zoned_table):
    Z.case_zoned_capacity_and_passes(env, zoned_table, sources=(1,), caps=(1, -1))


def test_row_helpers(env, zoned_table):
    """RowAggregateFields / RowWhereZoned / RowAggregateZoned and zone_excludes: the classes the tensors module drives give what the raw calls give"""
    chunks, rows_plain = zoned_table
    rows = K.chunk_rows(chunks, Z.Z_ROW)
    first = [int(x) for x in np.concatenate([[0], np.cumsum(rows)])]
    terms = [Z.at_row(first[1] + 10, K.GE, 0), Z.at_row(first[2] + 20, K.LT, 1)]
    listed = [env.pkg.term(W.predicate(env.pkg, kind, nbytes, op, constant, offset), clause) for offset, kind, nbytes, op, constant, clause in terms]
    zf = [env.pkg.field(kind, nbytes, offset=offset) for offset, kind, nbytes in Z.Z_ZONED]
    want = np.nonzero(K.mask_of(rows_plain, Z.Z_ROW, terms))[0]
    want_pruned = Z.excluded_chunks(rows_plain, Z.Z_ROW, rows, terms, Z.Z_ZONED)
    for src in K.both_sources(env, chunks):
        fields = env.pkg.RowAggregateFields(Z.Z_ROW, lib=env.lib)
        rc = fields.packed(src.container, src.size, src.offsets, zf) if src.packed else fields.batch(src.ptrs, zf)
        assert rc == 0 and fields.chunk_rows() == rows and fields.unread() == 0 and len(fields.totals()) == 3 and len(fields.chunks()) == len(rows)
        assert fields.totals()[0].count == sum(rows) and fields.chunks()[1][0].min_row == first[1]
        assert [env.pkg.zone_excludes(listed, zf, fields.chunks()[k], rows[k], lib=env.lib) for k in range(len(rows))] == want_pruned
        where, agg = env.pkg.RowWhereZoned(Z.Z_ROW, lib=env.lib), env.pkg.RowAggregateZoned(Z.Z_ROW, lib=env.lib)
        out = np.zeros(want.size, np.int64)
        fld = env.pkg.field(W.FLOAT, 4, offset=4)
        if src.packed:
            rc = where.packed(src.container, src.size, src.offsets, listed, zf, fields.entries(), out.ctypes.data, out.size)
            rc2 = agg.packed(src.container, src.size, src.offsets, fld, listed, zf, fields.entries())
        else:
            rc = where.batch(src.ptrs, listed, zf, fields.entries(), out.ctypes.data, out.size)
            rc2 = agg.batch(src.ptrs, fld, listed, zf, fields.entries())
        assert rc == 0 and where.total() == want.size and np.array_equal(out, want) and where.pruned() == want_pruned and where.unread() == 0
        assert rc2 == 0 and agg.total().count == want.size and agg.total().rows == sum(rows) and agg.pruned() == want_pruned
