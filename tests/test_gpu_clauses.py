"""The calls of include/blosc_gpu_clauses.h on the device: where and aggregate by a term list - an AND of OR clauses over any fields of a
row - in one decode.  The checks and cases are tests/clauses_checks.py's: numpy on the oracle's plaintext, everything compared exactly, a
list of one term byte for byte against blosc_gpu_where_* and blosc_gpu_aggregate_* (other kernels)."""
import numpy as np
import pytest

from getitem_ranges_checks import TorchMem
from helpers import orc_compress, ref_compress
from take_checks import BLOCKSIZE
import clauses_checks as K
import where_checks as W

pytestmark = pytest.mark.gpu
CODECS = ["lz4", "blosclz", "zstd", "zlib"]


@pytest.fixture(scope="module")
def mem(pkg):
    return TorchMem()


def lib_chunk(pkg, mem, data, T, shuffle, cname, blocksize):
    """blosc_gpu_compress_batch of one buffer"""
    src, dst = mem.put(data), mem.filled(data.size + 16, 0)
    b = pkg.DeviceBatch([src[1]], [data.size], [dst[1]], [data.size + 16])
    assert b.compress(T, 5, shuffle, cname.encode(), blocksize) == 0 and b.results()[0] > 0, b.results()
    return mem.get(dst[0])[:b.results()[0]].copy()


@pytest.fixture(scope="module")
def env(pkg, lib, mem, oracle, ref):
    assert hasattr(pkg, "declare_clauses") and hasattr(lib, "blosc_gpu_where_clauses_batch"), "the library has no clause calls"

    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle (LZ4, BloscLZ), by the reference where it is built, by this library, in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 0 and cname in ("lz4", "blosclz"): return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
            if who != 2 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            return lib_chunk(pkg, mem, data, T, shuffle, cname, BLOCKSIZE)
        return write
    return K.Env(pkg, lib, mem, oracle, writer)


@pytest.fixture(scope="module")
def shape_table(env):
    return K.shape_table(env, turn=1)


@pytest.mark.parametrize("kind,nbytes", W.KINDS, ids=[W.kind_name(*k) for k in W.KINDS])
def test_one_term_equals_the_existing_call(env, kind, nbytes):
    """all six ops, both entry points"""
    K.case_one_term(env, kind, nbytes, turn=W.KINDS.index((kind, nbytes)))


@pytest.mark.parametrize("name", list(K.SHAPES))
def test_term_counts_and_clause_shapes(env, shape_table, name):
    K.case_shape(env, name, shape_table)


@pytest.mark.parametrize("name", list(K.FIELD_CASES))
def test_fields(env, name):
    at = list(K.FIELD_CASES).index(name)
    K.case_fields(env, name, turn=at)
    K.case_fields(env, name, turn=at + 1)


def test_tile_and_chunk_edges(env):
    K.case_edges(env)
    K.case_edges(env, turn=2)


@pytest.mark.parametrize("name", K.EDGE_DENSITIES)
def test_densities(env, name):
    at = K.EDGE_DENSITIES.index(name)
    K.case_density(env, name, turn=at)
    K.case_density(env, name, turn=at + 1)


@pytest.mark.parametrize("cname", CODECS)
def test_a_chunk_that_does_not_decode(env, pkg, mem, oracle, ref, cname):
    def chunk_of(data):
        if cname in ("lz4", "blosclz"): return orc_compress(oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
        if ref is not None: return ref_compress(ref, data, 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
        return lib_chunk(pkg, mem, data, 17, 1, cname, BLOCKSIZE)
    K.case_damage(env, chunk_of, cname)


def test_capacity(env, shape_table):
    K.case_capacity(env, shape_table)


def test_passes_give_the_same(env, pkg, lib, shape_table):
    """... and under a pass bound of 16 KiB the new kernels are launched once per chunk that holds rows, the existing mark and tile kernels never"""
    K.case_passes(env, shape_table)
    chunks, rows_plain = shape_table
    src = K.TakeSource(env.mem, chunks=chunks)
    holding = sum(1 for r in K.chunk_rows(chunks, K.SHAPE_ROW) if r)
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        K.check_where(env, src, chunks, rows_plain, K.SHAPE_ROW, K.PLAIN_TERMS[:1], what="launches")      # one term too
        K.check_aggregate(env, src, chunks, rows_plain, K.SHAPE_ROW, K.SHAPE_LAYOUT[3], [], what="launches")      # and none
        names = ("k_where_mark_terms", "k_where_scan", "k_where_write", "k_aggregate_tiles_terms", "k_aggregate_chunks", "k_where_mark", "k_aggregate_tiles")
        assert [pkg.profile_get(k)[1] for k in names] == [holding] * 5 + [0, 0]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


def test_a_callers_stream(env, shape_table):
    import torch
    stream = torch.cuda.Stream()
    K.case_stream(env, shape_table, stream.cuda_stream)
    stream.synchronize()


def test_index_out_inside_a_source_is_refused(env):
    K.case_overlap(env)
