"""CPU: the calls of include/blosc_gpu_clauses.h on the emulated library - the host's term table (blosc_api.hip: terms_opening), the shared
pass bodies of engine.hip, k_where_mark_terms and k_aggregate_tiles_terms in front of the unchanged k_where_scan, k_where_write and
k_aggregate_chunks.  The checks are those of tests/test_gpu_clauses.py (tests/clauses_checks.py), the grid thinned to what the emulator runs
in about two minutes."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_clauses", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def env(emulib, pkgmod, oracle, ref):
    assert hasattr(emulib, "blosc_gpu_where_clauses_batch"), "the library has no clause calls"
    assert hasattr(pkgmod, "declare_clauses"), "the loader has no clause calls"

    def lib_compress(data, T, shuffle, cname):
        out = np.zeros(data.size + 16, np.uint8)
        r = emulib.blosc_compress_ctx(5, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname.encode(), BLOCKSIZE, 1)
        assert r > 0
        return out[:r].copy()

    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle, by the reference where it is built, by the emulated library (small chunks: it compresses 40 KB a second), in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 1 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            if who == 2 and data.size <= W.N // 2: return lib_compress(data, T, shuffle, cname)
            return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        return write
    return K.Env(pkgmod, emulib, NumpyMem(), oracle, writer)


@pytest.fixture(scope="module")
def shape_table(env):
    return K.shape_table(env)


@pytest.mark.parametrize("kind,nbytes", W.KINDS, ids=[W.kind_name(*k) for k in W.KINDS])
def test_one_term_equals_the_existing_call(env, kind, nbytes):
    """one op a kind, the entry points in turns (the device: all six ops through both)"""
    at = W.KINDS.index((kind, nbytes))
    K.case_one_term(env, kind, nbytes, ops=(at % 6,), packed_ops=(at % 6,) if at % 2 else (), turn=at)


@pytest.mark.parametrize("name", K.THIN_SHAPES)
def test_term_counts_and_clause_shapes(env, shape_table, name):
    K.case_shape(env, name, shape_table, thin=True)


@pytest.mark.parametrize("name", list(K.FIELD_CASES))
def test_fields(env, name):
    K.case_fields(env, name, turn=list(K.FIELD_CASES).index(name))


def test_tile_and_chunk_edges(env):
    K.case_edges(env)


@pytest.mark.parametrize("name", K.EDGE_DENSITIES)
def test_densities(env, name):
    K.case_density(env, name, turn=K.EDGE_DENSITIES.index(name))


def test_a_chunk_that_does_not_decode(env):
    K.case_damage(env, lambda data: orc_compress(env.oracle, data, 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1], "lz4")


def test_capacity(env, shape_table):
    K.case_capacity(env, shape_table)


def test_passes_give_the_same(env, shape_table):
    K.case_passes(env, shape_table)


def test_index_out_inside_a_source_is_refused(env):
    K.case_overlap(env)


def test_row_helpers(env, shape_table):
    """RowWhereClauses / RowAggregateClauses: the classes the tensors module drives give what the raw calls give"""
    chunks, rows_plain = shape_table
    terms = K.PLAIN_TERMS
    want = np.nonzero(K.mask_of(rows_plain, K.SHAPE_ROW, terms))[0]
    listed = [env.pkg.term(W.predicate(env.pkg, kind, nbytes, op, constant, offset), clause) for offset, kind, nbytes, op, constant, clause in terms]
    for src in K.both_sources(env, chunks):
        where, agg = env.pkg.RowWhereClauses(K.SHAPE_ROW, lib=env.lib), env.pkg.RowAggregateClauses(K.SHAPE_ROW, lib=env.lib)
        out = np.zeros(want.size, np.int64)
        fld = env.pkg.field(W.UINT, 1, offset=0)
        if src.packed:
            rc = where.packed(src.container, src.size, src.offsets, listed, out.ctypes.data, out.size)
            rc2 = agg.packed(src.container, src.size, src.offsets, fld, listed)
        else:
            rc = where.batch(src.ptrs, listed, out.ctypes.data, out.size)
            rc2 = agg.batch(src.ptrs, fld, listed)
        assert rc == 0 and where.total() == want.size and np.array_equal(out, want)
        assert where.chunk_rows() == K.chunk_rows(chunks, K.SHAPE_ROW) and sum(where.chunk_matches()) == want.size and where.unread() == 0
        assert rc2 == 0 and agg.total().count == want.size and agg.chunk_rows() == where.chunk_rows()
