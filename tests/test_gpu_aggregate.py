"""blosc_gpu_aggregate_batch / blosc_gpu_aggregate_packed on the device (include/blosc_gpu_aggregate.h): count, sum, min and max of a row
field of compressed chunks, per chunk and for the call.  The checks and cases are tests/aggregate_checks.py's: every expected answer is
numpy's on the field view of the oracle's plaintexts, a damaged chunk's code is the oracle's orc_decompress.  The last tests drive
tensors.aggregate_rows against torch, and against where_rows -> take_rows -> a torch reduction."""
import importlib.util
import os

import pytest

import aggregate_checks as A
from getitem_ranges_checks import TorchMem
from helpers import orc_compress, ref_compress
from take_checks import BLOCKSIZE
from test_gpu_where import CODECS, DTYPES, lib_chunk

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = A.SETTINGS


@pytest.fixture(scope="module")
def mem(pkg):
    return TorchMem()


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
    return A.make_env(pkg, lib, mem, oracle, writer)


@pytest.mark.parametrize("kind,nbytes", A.KINDS, ids=[A.kind_name(*k) for k in A.KINDS])
def test_every_kind_and_width(env, kind, nbytes):
    """every kind on where's value sets - integer extremes, NaNs, both zeros, both infinities, the smallest subnormal - unfiltered and under
    every filter of the case; the 64-bit sums wrap"""
    at = A.KINDS.index((kind, nbytes))
    A.case_kind(env, kind, nbytes, SETTINGS[at % len(SETTINGS)], turn=at)


@pytest.mark.parametrize("two", A.TWO_FIELDS, ids=[f"rows-of-{t[0]}" for t in A.TWO_FIELDS])
def test_filter_on_another_field(env, two):
    at = A.TWO_FIELDS.index(two)
    A.case_other_field(env, two, SETTINGS[at], turn=at)
    A.case_other_field(env, two, (CODECS[2 + at], 4, 1, 1), turn=at + 1)


@pytest.mark.parametrize("layout", A.LAYOUTS, ids=[f"{l[0]}-at-{l[1]}" for l in A.LAYOUTS])
def test_row_layouts_and_both_entry_points(env, layout):
    """every row layout under two settings, one of them a Zstd or zlib one; one layout on a caller's side stream"""
    import torch
    at = A.LAYOUTS.index(layout)
    A.case_layout(env, layout, SETTINGS[(at + 2) % len(SETTINGS)], turn=at)
    stream = torch.cuda.Stream() if at == 1 else None
    A.case_layout(env, layout, (CODECS[2 + at % 2], (1, 4, 8, 17)[at % 4], at % 3, 1 if at % 4 == 3 else 8), turn=at + 1,
                  stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()


def test_tile_and_chunk_edges(env):
    A.case_edges(env)


def test_many_tiles(env):
    A.case_many_tiles(env)


def test_chunks_taller_than_256_tiles(env):
    """chunks of 256, 257 and 513 tiles: a lane of k_aggregate_chunks folds a second and a third tile, every sum bit for bit the documented tree's"""
    A.case_tall_chunks(env)


@pytest.mark.parametrize("kind", [A.FLOAT, A.INT], ids=["float64", "int64"])
def test_extremes_across_the_second_turn_of_the_tile_loop(env, kind):
    A.case_tall_extremes(env, kind, turn=kind)


def test_one_byte_rows_of_a_tall_chunk(env):
    A.case_tall_bytes(env)


@pytest.mark.parametrize("kind,nbytes", A.FLOATS, ids=[A.kind_name(*k) for k in A.FLOATS])
def test_float_sum_exact_and_subnormals(env, kind, nbytes):
    """sums whose every partial sum is exact equal math.fsum; a column of the format's smallest subnormal is count x that value"""
    at = A.FLOATS.index((kind, nbytes))
    A.case_sum_exact(env, kind, nbytes, 40000, turn=at)
    A.case_sum_subnormals(env, kind, nbytes, 30000, turn=at + 1)


@pytest.mark.parametrize("kind,nbytes", A.FLOATS, ids=[A.kind_name(*k) for k in A.FLOATS])
def test_exact_sum_windows(env, kind, nbytes):
    """every finite binary16 and bfloat16 pattern, binary32 over all its exponent fields with every leading bit of a subnormal, binary64
    subnormals: windows whose sums are exact in any order, each unfiltered, under GT +0 and under LT +0, equal to math.fsum"""
    for w, patterns in enumerate(A.WINDOWS[(kind, nbytes)]()):
        A.case_sum_window(env, kind, nbytes, patterns, turn=w, what=w)


@pytest.mark.parametrize("row_layout", A.LAYOUTS16, ids=[f"{l[0]}-at-{l[1]}" for l in A.LAYOUTS16])
@pytest.mark.parametrize("kind,nbytes", A.KINDS16, ids=[A.kind_name(*k) for k in A.KINDS16])
def test_every_16_bit_pattern_below_and_above_each_constant(env, kind, nbytes, row_layout):
    """the 65 536 patterns as rows: max under LT c and min under GT c are c's neighbours, across both zeros and every change of regime"""
    A.case_patterns16(env, kind, row_layout, A.constants16(kind), turn=A.KINDS16.index((kind, nbytes)))


@pytest.mark.parametrize("kind,nbytes", A.NEIGHBOUR_KINDS, ids=[A.kind_name(*k) for k in A.NEIGHBOUR_KINDS])
def test_neighbours_of_the_wide_kinds(env, kind, nbytes):
    """the neighbours of 2^31, 2^32 and 2^63, the regime changes of binary32 and binary64, halves of 8-byte values: under LT c and GT c"""
    at = A.NEIGHBOUR_KINDS.index((kind, nbytes))
    A.case_neighbours(env, kind, nbytes, SETTINGS[at % len(SETTINGS)], turn=at)


@pytest.mark.parametrize("nbytes", [4, 8])
def test_float_sum_rounding_and_bit_identity(env, nbytes):
    import torch
    stream = torch.cuda.Stream()
    A.case_sum_rounding(env, nbytes, 40000, side_stream=stream.cuda_stream, turn=nbytes)
    stream.synchronize()


def test_one_launch_of_each_kernel_per_pass(env, pkg, lib):
    """a pass bound of 16 KiB: k_aggregate_tiles and k_aggregate_chunks are each launched once per chunk that holds rows"""
    values = A.value_set(A.UINT, 4)
    chunks, rows_plain = A.table_call(env, SETTINGS[0], A.LAYOUTS[1], A.drawn(values, A.total_rows(12)), turn=0)
    src = A.TakeSource(env.mem, chunks=chunks)
    holding = sum(1 for r in A.chunk_rows(chunks, 12) if r)
    lib.blosc_amd_getitem_pass_bytes(16 << 10)
    lib.blosc_gpu_profile(1)
    try:
        for flt in (None, (5, A.UINT, 4, A.NE, values[2])):
            lib.blosc_gpu_profile_reset()
            A.check_aggregate(env, src, chunks, rows_plain, 12, (5, A.UINT, 4), flt, what="launches")
            assert [pkg.profile_get(k)[1] for k in ("k_aggregate_tiles", "k_aggregate_chunks")] == [holding] * 2
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", CODECS)
def test_a_chunk_that_does_not_decode(env, pkg, mem, oracle, ref, cname):
    def chunk_of(data):
        if cname in ("lz4", "blosclz"): return orc_compress(oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
        if ref is not None: return ref_compress(ref, data, 17, 5, 1, cname.encode(), blocksize=BLOCKSIZE)[1]
        return lib_chunk(pkg, mem, data, 17, 1, cname, BLOCKSIZE)
    A.case_damage(env, chunk_of, cname)


def test_refused_calls(env):
    A.case_refused(env)


# ---- tensors.aggregate_rows ----
@pytest.fixture(scope="module")
def tensors():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_aggregate", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torch_answer(torch, col, mask):
    """(count, nans, sum, min, max, argmin, argmax) of col[mask] by torch; the extremes over the values that are no NaN, their first occurrence
    from torch.nonzero"""
    nan = torch.isnan(col) if col.dtype.is_floating_point else torch.zeros_like(mask)
    sel = mask & ~nan
    if col.dtype.is_floating_point: total = col[sel].double().sum().item()
    elif col.dtype == torch.bool: total = int(col[sel].sum().item())
    else: total = int(col[sel].to(torch.int64).sum().item())
    low = high = at_low = at_high = None
    if sel.any():
        v = col[sel].double() if col.dtype.is_floating_point else col[sel].to(torch.int64)
        low, high = v.min(), v.max()
        wide = col.double() if col.dtype.is_floating_point else col.to(torch.int64)
        at_low, at_high = int(torch.nonzero(sel & (wide == low))[0]), int(torch.nonzero(sel & (wide == high))[0])
        low, high = col[at_low].item(), col[at_high].item()
    return int(mask.sum()), int((mask & nan).sum()), total, low, high, at_low, at_high


def same(got, want):
    """an Aggregated against torch_answer's tuple: the sums equal (exact on this data), the extremes with their rows - and, for zeros, their sign"""
    import math
    assert (got.count, got.nans, got.argmin, got.argmax) == (want[0], want[1], want[5], want[6]), (got, want)
    assert got.sum == want[2] and (got.min, got.max) == (want[3], want[4]), (got, want)
    for a, b in ((got.min, want[3]), (got.max, want[4])):
        assert not isinstance(a, float) or math.copysign(1, a) == math.copysign(1, b), (got, want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_aggregate_rows_of_every_dtype(lib, tensors, dtype):
    """a table of 5000 rows of 6 elements in five chunks, multiples of 0.5 with NaN, inf and -0 sprinkled into the floating-point ones:
    aggregate_rows on a column, unfiltered and under a filter on the same and on another column, is torch's answer - for the table and per chunk"""
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
    col = table[:, 4]
    everything = torch.ones(5000, dtype=torch.bool, device=dev)
    one = True if dt == torch.bool else 1
    runs = [(None, everything), (("lt", one, 4), col < one), (("ge", one, 2), table[:, 2] >= one), (("ne", one, 4), col != one)]
    if dt.is_floating_point:
        runs += [(("lt", float("inf"), 4), col < float("inf")), (("eq", float("nan"), 4), ~everything), (("ne", float("nan"), 4), everything)]
        # 0.1 is no value of the dtype: rounded to it, as torch rounds the scalar of its comparison
        runs += [(("eq", 0.1, 1), table[:, 1] == 0.1), (("gt", 0.1, 1), table[:, 1] > 0.1)]
        assert 0 < int((table[:, 1] == 0.1).sum()) < 5000
    else:      # 1.5 is no value of an integer column: refused, not answered for the constant 1
        with pytest.raises(ValueError, match="1.5"):
            tensors.aggregate_rows(lib, cont, off, meta, column=4, where=("lt", 1.5, 4))
    for where, mask in runs:
        got = tensors.aggregate_rows(lib, cont, off, meta, column=4, where=where)
        same(got, torch_answer(torch, col, mask))
        assert len(got.chunks) == 5
        for k, c in enumerate(got.chunks):
            inside = torch.zeros_like(mask); inside[1000 * k:1000 * (k + 1)] = True
            same(c, torch_answer(torch, col, mask & inside))
    with pytest.raises(ValueError):
        tensors.aggregate_rows(lib, cont, off, meta, column=6)
    with pytest.raises(ValueError):
        tensors.aggregate_rows(lib, cont, off, meta, column=1, where=("eq", one, 6))
    with pytest.raises(ValueError):
        tensors.aggregate_rows(lib, cont, off, meta, column=1, where=("like", one, 0))
    with pytest.raises(ValueError):
        tensors.aggregate_rows(lib, cont, off, [(torch.complex64, s) for _, s in meta], column=0)
    with pytest.raises(RuntimeError, match="does not hold this table"):
        tensors.aggregate_rows(lib, cont, off, [(d, (s[0] + 1,) + tuple(s[1:])) for d, s in meta], column=4)


def test_unread_rows_raise(lib, tensors):
    """a chunk that does not decode: aggregate_rows raises, like where_rows, and names the unread rows"""
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    table = (torch.arange(6000 * 4, device=dev) % 97).to(torch.float32).reshape(6000, 4)
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=1000, cname=b"lz4", shuffle=1)
    assert tensors.aggregate_rows(lib, cont, off, meta, column=1).count == 6000
    head = cont[off[2]:off[2] + 16].cpu().numpy()
    assert not head[2] & 2, "chunk 2 came out MEMCPYED"
    broken = cont.clone()      # the first bstarts entry of chunk 2 sent behind the chunk, as getitem_ranges_checks.pick_damage does
    broken[off[2] + 16:off[2] + 20] = torch.from_numpy(np.array([int(head[12:16].view("<i4")[0]) + 100], "<i4").view(np.uint8)).to(dev)
    with pytest.raises(RuntimeError, match="1000 of 6000 rows were not read"):
        tensors.aggregate_rows(lib, broken, off, meta, column=1)


def test_aggregate_is_where_then_take_then_reduce(lib, tensors):
    """aggregate_rows(where=("eq", k, column)) agrees with where_rows -> take_rows -> a torch reduction on the same container"""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(11)
    table = (torch.randint(-2000, 2001, (6000, 17), device=dev, generator=g) * 0.5).to(torch.float32)
    table[:, 3] = torch.randint(0, 50, (6000,), device=dev, generator=g).to(table.dtype)
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=1000, cname=b"lz4", shuffle=1)
    got = tensors.aggregate_rows(lib, cont, off, meta, column=9, where=("eq", 7.0, 3))
    index, total = tensors.where_rows(lib, cont, off, meta, "eq", 7.0, column=3)
    rows = tensors.take_rows(lib, cont, off, meta, index)
    assert got.count == total == rows.shape[0] > 50 and got.nans == 0
    v = rows[:, 9]
    assert got.sum == v.double().sum().item() and got.min == v.min().item() and got.max == v.max().item()
    assert got.argmin == int(index[torch.nonzero(v == v.min())[0]]) and got.argmax == int(index[torch.nonzero(v == v.max())[0]])
    assert sum(c.count for c in got.chunks) == total
    none = tensors.aggregate_rows(lib, cont, off, meta, column=9, where=("gt", 1e9, 3))
    assert (none.count, none.nans, none.sum, none.min, none.max, none.argmin, none.argmax) == (0, 0, 0.0, None, None, None, None)
