"""blosc_gpu_where_batch / blosc_gpu_where_packed on the device (include/blosc_gpu_where.h): the rows of compressed chunks whose field
satisfies a predicate, as an index table in device memory.  The checks and cases are tests/where_checks.py's: the expected table is
numpy.nonzero on the field view of the oracle's plaintexts, a damaged chunk's code is the oracle's orc_decompress.  The last tests run the
loop the calls exist for: where_rows -> take_rows -> put_rows of c-blosc_amd/tensors.py."""
import importlib.util
import operator
import os

import numpy as np
import pytest

from getitem_ranges_checks import TorchMem
from helpers import orc_compress, ref_compress
from take_checks import BLOCKSIZE, many_chunks
from test_emu_take import SETTINGS
import where_checks as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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
    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle (LZ4, BloscLZ), by the reference where it is built, by this library, in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 0 and cname in ("lz4", "blosclz"): return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
            if who != 2 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            return lib_chunk(pkg, mem, data, T, shuffle, cname, BLOCKSIZE)
        return write
    return W.Env(pkg, lib, mem, oracle, writer)


@pytest.mark.parametrize("kind,nbytes", W.KINDS, ids=[W.kind_name(*k) for k in W.KINDS])
def test_every_kind_width_and_op(env, kind, nbytes):
    """every op against every constant of the kind's value set, NaN included"""
    at = W.KINDS.index((kind, nbytes))
    W.case_kind(env, kind, nbytes, SETTINGS[at % len(SETTINGS)], W.all_picks, turn=at)


@pytest.mark.parametrize("row_layout", W.LAYOUTS16, ids=[f"{l[0]}-at-{l[1]}" for l in W.LAYOUTS16])
@pytest.mark.parametrize("kind,nbytes", W.KINDS16, ids=[W.kind_name(*k) for k in W.KINDS16])
def test_every_16_bit_pattern_against_each_constant(env, kind, nbytes, row_layout):
    """the 65 536 patterns as rows, every op against the byte carries and the sign change (integers), against both zeros and every change of
    regime up to the first NaN (binary16, bfloat16); three of the ops through the packed entry point as well"""
    W.case_patterns16(env, kind, row_layout, W.constants16(kind), turn=W.KINDS16.index((kind, nbytes)))


@pytest.mark.parametrize("kind,nbytes", W.NEIGHBOUR_KINDS, ids=[W.kind_name(*k) for k in W.NEIGHBOUR_KINDS])
def test_neighbours_of_the_wide_kinds(env, kind, nbytes):
    """every op against every constant of the kind's neighbour set: around 2^31, 2^32 and 2^63, the regime changes of binary32 and binary64,
    8-byte values that differ in one half only"""
    at = W.NEIGHBOUR_KINDS.index((kind, nbytes))
    W.case_neighbours(env, kind, nbytes, SETTINGS[(at + 1) % len(SETTINGS)], turn=at)


@pytest.mark.parametrize("layout", W.LAYOUTS, ids=[f"{l[0]}-at-{l[1]}" for l in W.LAYOUTS])
def test_row_layouts_and_both_entry_points(env, layout):
    """every op on every row layout under two settings, one of them a Zstd or zlib one; one layout on a caller's side stream"""
    import torch
    at = W.LAYOUTS.index(layout)
    W.case_layout(env, layout, SETTINGS[(at + 2) % len(SETTINGS)], turn=at)
    stream = torch.cuda.Stream() if at == 1 else None
    W.case_layout(env, layout, (CODECS[2 + at % 2], (1, 4, 8, 17)[at % 4], at % 3, 1 if at % 4 == 3 else 8), turn=at + 1,
                  stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()


@pytest.mark.parametrize("name", W.DENSITIES)
def test_densities(env, name):
    at = W.DENSITIES.index(name)
    W.case_density(env, name, SETTINGS[at % len(SETTINGS)], turn=at)


def test_many_tiles(env):
    W.case_many_tiles(env)


@pytest.mark.parametrize("name", list(W.WIDE))
def test_more_tiles_in_a_pass_than_scan_threads(env, name):
    """1024, 1025 and 2051 tiles in one pass: every thread of k_where_scan with one tile; threads with two, one and no tiles; three tiles a
    thread with a chunk boundary inside a thread's stretch"""
    W.case_wide_pass(env, name)


def test_more_chunks_than_tiles_a_thread(env):
    """1300 small chunks, more than 1024 tiles: in one pass and in dozens of passes of 16 KiB"""
    W.case_many_chunks(env, many_chunks(env.oracle, env.writer("lz4", 4, 1, 0), 48, 1300))


def test_capacity(env):
    W.case_capacity(env, SETTINGS[1], turn=1)
    W.case_capacity(env, SETTINGS[4], turn=2)


def test_passes_give_the_same(env, pkg, lib):
    """a pass bound of 16 KiB: one launch of k_where_mark, k_where_scan and k_where_write per chunk that holds rows, the table that of one pass"""
    W.case_passes(env, SETTINGS[2], W.LAYOUTS[2], turn=2)
    W.case_passes(env, ("zstd", 8, 1, 8), W.LAYOUTS[4], turn=0)
    values = W.value_set(W.UINT, 4)
    chunks, rows_plain = W.table_call(env, SETTINGS[0], W.LAYOUTS[1], W.drawn(values, W.total_rows(12)), turn=0)
    src = W.TakeSource(env.mem, chunks=chunks)
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        W.check_where(lib, env.mem, src, chunks, rows_plain, 12, (5, W.UINT, 4, 0, values[2]), pkg, what="launches")
        holding = sum(1 for r in W.chunk_rows(chunks, 12) if r)
        assert [pkg.profile_get(k)[1] for k in ("k_where_mark", "k_where_scan", "k_where_write")] == [holding] * 3
        lib.blosc_gpu_profile_reset()
        W.check_where(lib, env.mem, src, chunks, rows_plain, 12, (5, W.UINT, 4, 0, values[2]), pkg, capacity=0, what="the count alone")
        assert [pkg.profile_get(k)[1] for k in ("k_where_mark", "k_where_scan", "k_where_write")] == [holding, 0, 0]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", CODECS)
def test_a_chunk_that_does_not_decode(env, pkg, mem, oracle, ref, cname):
    def chunk_of(data):
        if cname in ("lz4", "blosclz"): return orc_compress(oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
        if ref is not None: return ref_compress(ref, data, 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
        return lib_chunk(pkg, mem, data, 17, 1, cname, BLOCKSIZE)
    W.case_damage(env, chunk_of, cname)


def test_refused_calls(env):
    W.case_refused(env)


# ---- the loop the calls exist for: tensors.where_rows -> take_rows -> put_rows ----
@pytest.fixture(scope="module")
def tensors():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_where", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DTYPES = ["uint8", "bool", "int8", "int16", "int32", "int64", "float16", "float32", "float64", "bfloat16"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_where_rows_of_every_dtype(lib, tensors, dtype):
    """a table of 5000 rows of 6 elements in five chunks: where_rows on a column is torch.nonzero of the torch comparison, for every op"""
    import torch
    dev = torch.device("cuda:0")
    dt = getattr(torch, dtype)
    g = torch.Generator(device=dev); g.manual_seed(7)
    table = torch.randint(-3 if dt.is_signed else 0, 4, (5000, 6), device=dev, generator=g).to(dt)
    if dt.is_floating_point:
        table = table * 0.5
        table[::37, 4] = float("nan"); table[5::41, 4] = float("inf"); table[3::43, 4] = -0.0
        table[::29, 1] = 0.1; table[1::31, 1] = 0.125; table[2::31, 1] = 0.0625      # column 1: the dtype's 0.1 between its neighbours
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=1000, cname=b"lz4", shuffle=1)
    for name, fn in (("eq", operator.eq), ("ne", operator.ne), ("lt", operator.lt), ("le", operator.le), ("gt", operator.gt), ("ge", operator.ge)):
        for value in ((True,) if dt == torch.bool else (1, 0) + ((float("nan"), -0.5) if dt.is_floating_point else ())):
            index, total = tensors.where_rows(lib, cont, off, meta, name if value != 0 else fn, value, column=4)
            want = torch.nonzero(fn(table[:, 4], value)).flatten()
            assert index.dtype == torch.int64 and index.is_cuda and total == want.numel() and torch.equal(index, want), (dtype, name, value)
        if dt.is_floating_point:      # 0.1 is no value of the dtype: rounded to it, as torch rounds the scalar of its comparison
            index, total = tensors.where_rows(lib, cont, off, meta, name, 0.1, column=1)
            want = torch.nonzero(fn(table[:, 1], 0.1)).flatten()
            assert 0 < want.numel() < 5000 and total == want.numel() and torch.equal(index, want), (dtype, name, 0.1)
        else:                         # 1.5 is no value of an integer column: refused, not answered for the constant 1
            with pytest.raises(ValueError, match="1.5"):
                tensors.where_rows(lib, cont, off, meta, name, 1.5, column=4)
    want = torch.nonzero(table[:, 4] >= 1).flatten()
    index, total = tensors.where_rows(lib, cont, off, meta, "ge", 1, column=4, max_matches=want.numel() // 2)
    assert total == want.numel() > 2 and torch.equal(index, want[:want.numel() // 2])
    index, total = tensors.where_rows(lib, cont, off, meta, "ge", 1, column=4, max_matches=want.numel() + 9)
    assert total == want.numel() and torch.equal(index, want)
    with pytest.raises(ValueError):
        tensors.where_rows(lib, cont, off, meta, "ge", 1, column=6)


def test_where_then_take_then_put(lib, tensors):
    """select by value, gather and update without the table's plaintext: the rows are table[nonzero(...)], the update is index_copy_"""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(11)
    table = torch.cumsum(torch.randn(6000 * 17, device=dev, generator=g) * 1e-3, 0).reshape(6000, 17)
    keys = torch.randint(0, 50, (6000,), device=dev, generator=g)
    table[:, 3] = keys.to(table.dtype)
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=1000, cname=b"lz4", shuffle=1)
    index, total = tensors.where_rows(lib, cont, off, meta, "eq", 7.0, column=3)
    want = torch.nonzero(table[:, 3] == 7.0).flatten()
    assert total == want.numel() > 50 and torch.equal(index, want)
    rows = tensors.take_rows(lib, cont, off, meta, index)
    assert torch.equal(rows, table[want])
    new = rows * 2 + 1
    cont2, off2 = tensors.put_rows(lib, cont, off, meta, index, new)
    back = torch.cat(tensors.unpack_tensors(lib, cont2, off2, meta))
    assert torch.equal(back, table.clone().index_copy_(0, want, new))
    none, total = tensors.where_rows(lib, cont, off, meta, "gt", 1e9, column=3)
    assert total == 0 and none.numel() == 0 and none.dtype == torch.int64
    with pytest.raises(ValueError):
        tensors.where_rows(lib, cont, off, [(torch.complex64, s) for _, s in meta], "eq", 1, column=0)
    with pytest.raises(RuntimeError, match="does not hold this table"):
        tensors.where_rows(lib, cont, off, [(dt, (s[0] + 1,) + tuple(s[1:])) for dt, s in meta], "eq", 1.0, column=3)
