"""CPU: blosc_gpu_aggregate_batch / blosc_gpu_aggregate_packed (include/blosc_gpu_aggregate.h) on the emulated library - the host engine's
census, passes and tile tables, k_aggregate_tiles, k_aggregate_chunks and the fold on the host.  The checks are those of
tests/test_gpu_aggregate.py (tests/aggregate_checks.py), the grid thinned to what the emulator runs in about a minute per test."""
import importlib.util
import os

import numpy as np
import pytest

import aggregate_checks as A
from getitem_ranges_checks import NumpyMem
from helpers import orc_compress, ptr, ref_compress
from take_checks import BLOCKSIZE
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = A.SETTINGS


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_aggregate", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def env(emulib, pkgmod, oracle, ref):
    assert hasattr(emulib, "blosc_gpu_aggregate_batch"), "the library has no aggregate calls"

    def lib_compress(data, T, shuffle, cname):
        out = np.zeros(data.size + 16, np.uint8)
        r = emulib.blosc_compress_ctx(5, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname.encode(), BLOCKSIZE, 1)
        assert r > 0
        return out[:r].copy()

    def writer(cname, T, shuffle, turn):
        """chunk k by the oracle, by the reference where it is built, by the emulated library (the half-size chunks: it compresses 40 KB a second), in turns"""
        def write(k, data):
            who = (k + turn) % 3
            if who == 1 and ref is not None: return ref_compress(ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            if who == 2 and data.size <= A.N // 2: return lib_compress(data, T, shuffle, cname)
            return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        return write
    return A.make_env(pkgmod, emulib, NumpyMem(), oracle, writer)


@pytest.mark.parametrize("kind,nbytes", A.KINDS, ids=[A.kind_name(*k) for k in A.KINDS])
def test_every_kind_and_width(env, kind, nbytes):
    at = A.KINDS.index((kind, nbytes))
    A.case_kind(env, kind, nbytes, SETTINGS[at % 3], turn=at, thin=True)


@pytest.mark.parametrize("two", A.TWO_FIELDS, ids=[f"rows-of-{t[0]}" for t in A.TWO_FIELDS])
def test_filter_on_another_field(env, two):
    at = A.TWO_FIELDS.index(two)
    A.case_other_field(env, two, SETTINGS[at], turn=at)


@pytest.mark.parametrize("layout", A.LAYOUTS, ids=[f"{l[0]}-at-{l[1]}" for l in A.LAYOUTS])
def test_row_layouts_and_both_entry_points(env, layout):
    at = A.LAYOUTS.index(layout)
    A.case_layout(env, layout, SETTINGS[(at + 1) % 3], turn=at)


def test_tile_and_chunk_edges(env):
    A.case_edges(env)


def test_many_tiles(env):
    A.case_many_tiles(env, thin=True)


def test_a_chunk_taller_than_256_tiles(env):
    """the device's chunk of 257 tiles, its empty one and its chunk of one row: lane 0 of k_aggregate_chunks folds a second tile"""
    A.case_tall_chunks(env, rows=A.TALL_ROWS[1:3] + A.TALL_ROWS[4:], seeds=A.TALL_SEEDS[1:3] + A.TALL_SEEDS[4:], thin=True)


@pytest.mark.parametrize("kind,nbytes", A.FLOATS, ids=[A.kind_name(*k) for k in A.FLOATS])
def test_float_sum_exact_and_subnormals(env, kind, nbytes):
    at = A.FLOATS.index((kind, nbytes))
    A.case_sum_exact(env, kind, nbytes, 3000, turn=at)
    A.case_sum_subnormals(env, kind, nbytes, 2500, turn=at + 1)


@pytest.mark.parametrize("kind,nbytes", A.FLOATS[:2], ids=[A.kind_name(*k) for k in A.FLOATS[:2]])
def test_exact_sum_windows_of_every_16_bit_value(env, kind, nbytes):
    """every finite binary16 / bfloat16 pattern widened and added, unfiltered (the device runs each window under GT +0 and LT +0 as well)"""
    for w, patterns in enumerate(A.WINDOWS[(kind, nbytes)]()):
        A.case_sum_window(env, kind, nbytes, patterns, ways=(None,), turn=w, what=w)


@pytest.mark.parametrize("w", [0, 9])
def test_exact_sum_windows_of_binary32(env, w):
    """the window that holds the subnormals, every leading bit among them, and one of normals - of the device's 15"""
    A.case_sum_window(env, A.FLOAT, 4, A.window_f32(w), turn=w, what=w)


def test_exact_sum_window_of_binary64_subnormals(env):
    A.case_sum_window(env, A.FLOAT, 8, A.window_f64(), ways=(None,), what="binary64")


@pytest.mark.parametrize("kind,nbytes", A.KINDS16, ids=[A.kind_name(*k) for k in A.KINDS16])
def test_every_16_bit_pattern_below_and_above_each_constant(env, kind, nbytes):
    """rows of 2 bytes, the four constants of the kind that sit on a change of regime (the device: both layouts, every constant)"""
    A.case_patterns16(env, kind, A.LAYOUTS16[0], A.thin_constants16(kind), turn=A.KINDS16.index((kind, nbytes)))


@pytest.mark.parametrize("kind,nbytes", A.NEIGHBOUR_KINDS, ids=[A.kind_name(*k) for k in A.NEIGHBOUR_KINDS])
def test_neighbours_of_the_wide_kinds(env, kind, nbytes):
    at = A.NEIGHBOUR_KINDS.index((kind, nbytes))
    A.case_neighbours(env, kind, nbytes, SETTINGS[at % 3], turn=at, thin=True)


@pytest.mark.parametrize("nbytes", [4, 8])
def test_float_sum_rounding_and_bit_identity(env, nbytes):
    A.case_sum_rounding(env, nbytes, 4000, turn=nbytes)


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_a_chunk_that_does_not_decode(env, cname):
    A.case_damage(env, lambda data: orc_compress(env.oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1], cname, thin=(cname == "blosclz"))


def test_refused_calls(env):
    A.case_refused(env)


def test_row_aggregate_helper(env):
    """RowAggregate.batch / .packed: the class the tensors module drives gives what the raw calls give"""
    values = A.value_set(A.INT, 4)
    chunks, rows_plain = A.table_call(env, SETTINGS[0], (12, 5, A.INT, 4), A.drawn(values, A.total_rows(12)), turn=0)
    fld = env.pkg.field(env.pkg.FIELD_INT, 4, offset=5)
    flt = env.pkg.predicate(env.pkg.FIELD_INT, 4, env.pkg.WHERE_GE, 0, offset=5)
    for src in A.both_sources(env, chunks):
        want = A.check_aggregate(env, src, chunks, rows_plain, 12, (5, A.INT, 4), (5, A.INT, 4, A.GE, 0), what="raw")
        agg = env.pkg.RowAggregate(12, lib=env.lib)
        rc = agg.packed(src.container, src.size, src.offsets, fld, flt) if src.packed else agg.batch(src.ptrs, fld, flt)
        assert rc == 0 and (A.entry(agg.total()), [A.entry(c) for c in agg.chunks()]) == want
        assert agg.chunk_rows() == A.chunk_rows(chunks, 12) and agg.chunk_status() == [0] * len(chunks) and agg.unread() == 0
        rc = agg.packed(src.container, src.size, src.offsets, fld) if src.packed else agg.batch(src.ptrs, fld)
        assert rc == 0 and agg.total().count == agg.total().rows == sum(A.chunk_rows(chunks, 12))
