"""The calls of include/blosc_gpu_zones.h on the device: several fields aggregated in one decode, byte for byte what the clause call answers
for each field alone; where and aggregate that do not decode the chunks a zone map excludes, byte for byte what the clause calls answer.
The checks and cases are tests/zones_checks.py's."""
import numpy as np
import pytest

from getitem_ranges_checks import TorchMem
from helpers import orc_compress, ref_compress
from take_checks import BLOCKSIZE
import clauses_checks as K
import zones_checks as Z

pytestmark = pytest.mark.gpu


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
    assert hasattr(pkg, "declare_zones") and hasattr(lib, "blosc_gpu_where_zoned_batch"), "the library has no zone calls"

    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle (LZ4, BloscLZ), by the reference where it is built, by this library, in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 0 and cname in ("lz4", "blosclz"): return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
            if who != 2 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            return lib_chunk(pkg, mem, data, T, shuffle, cname, BLOCKSIZE)
        return write
    return Z.Env(pkg, lib, mem, oracle, writer)


@pytest.fixture(scope="module")
def table20(env):
    return Z.table20(env, turn=1)


@pytest.fixture(scope="module")
def zoned_table(env):
    return Z.zoned_table(env, turn=1)


@pytest.mark.parametrize("name", list(Z.TERM_LISTS))
def test_fields_equal_the_single_field_calls(env, table20, name):
    """1, 2, 15 and 16 fields, batch and packed, over chunks of 1 ... 2049 rows, a chunk of nbytes 0 and a MEMCPYED chunk"""
    Z.case_shape_fields(env, table20, lists=(name,))


@pytest.mark.parametrize("nterms", [0, 1, 16])
def test_sixteen_fields_of_every_kind(env, nterms):
    Z.case_wide_fields(env, Z.table96(env, K.EDGE_ROWS, turn=nterms), lists=(nterms,))


def test_fields_a_chunk_that_does_not_decode(env, oracle):
    Z.case_fields_damage(env, lambda data: orc_compress(oracle, data, 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1], "lz4")


def test_fields_passes_give_the_same(env, pkg, lib, table20):
    """... and under a pass bound of 16 KiB the two new kernels are launched once per pass that holds a row, the single-field kernels never"""
    Z.case_fields_passes(env, table20)
    chunks, rows_plain = table20
    src = K.TakeSource(env.mem, chunks=chunks)
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        out = Z.FieldsOut(pkg, len(chunks), 3)
        assert Z.raw_fields(lib, src, K.SHAPE_ROW, Z.fields_table(pkg, K.SHAPE_LAYOUT[:3]), 3, None, 0, out) == 0
        counts = [pkg.profile_get(k)[1] for k in ("k_aggregate_tiles_fields", "k_aggregate_chunks_fields", "k_aggregate_tiles_terms", "k_aggregate_chunks",
                                                  "k_aggregate_tiles")]
        assert counts[0] == counts[1] > 1 and counts[2:] == [0, 0, 0], counts
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


def test_fields_sums_that_round(env):
    Z.case_fields_rounding(env, turn=1)


def test_fields_a_chunk_of_257_tiles(env):
    Z.case_fields_tall(env)


def test_fields_on_a_callers_stream(env, table20):
    import torch
    stream = torch.cuda.Stream()
    Z.case_fields_stream(env, table20, stream.cuda_stream)
    stream.synchronize()


@pytest.mark.parametrize("family", list(Z.zoned_lists()))
def test_zoned_calls_equal_the_clause_calls(env, zoned_table, family):
    Z.case_zoned_family(env, zoned_table, family)


def test_zoned_nothing_and_everything(env, pkg, lib, zoned_table):
    """... and the all-pruned call launches no decode"""
    Z.case_zoned_nothing_and_everything(env, zoned_table)
    chunks, rows_plain = zoned_table
    src = K.TakeSource(env.mem, chunks=chunks)
    ftab, zones = Z.build_map(env, src, chunks, rows_plain)
    name, terms, _ = Z.zoned_lists()["nothing"][0]
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        rc, _, out, pruned = Z.run_where_zoned(env, src, terms, ftab, len(Z.Z_ZONED), zones, 4)
        assert rc == 0 and out.total.value == 0 and out.unread.value == 0 and sum(pruned) == sum(1 for r in K.chunk_rows(chunks, Z.Z_ROW) if r)
        rc, _, _, pruned = Z.run_aggregate_zoned(env, src, Z.Z_NOISE, terms, ftab, len(Z.Z_ZONED), zones)
        assert rc == 0
        counts = {k: pkg.profile_get(k)[1] for k in ("k_decode_streams", "k_where_mark_terms", "k_where_scan", "k_where_write", "k_aggregate_tiles_terms",
                                                     "k_aggregate_chunks")}
        assert not any(counts.values()), counts
        # the same list without the map decodes
        lib.blosc_gpu_profile_reset()
        K.check_where(env, src, chunks, rows_plain, Z.Z_ROW, terms, what="unzoned")
        assert pkg.profile_get("k_decode_streams")[1] > 0
    finally:
        lib.blosc_gpu_profile(0)


def test_a_pruned_chunk_is_not_read(env, zoned_table):
    Z.case_zoned_garbage(env, zoned_table)


def test_a_map_of_other_rows_is_refused(env, zoned_table):
    Z.case_zoned_stale_rows(env, zoned_table)


def test_zoned_capacity_and_passes(env, zoned_table):
    Z.case_zoned_capacity_and_passes(env, zoned_table)
