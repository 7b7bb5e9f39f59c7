"""CPU: blosc_gpu_where_batch / blosc_gpu_where_packed (include/blosc_gpu_where.h) on the emulated library - the host engine's census, passes
and tile tables, k_where_mark, k_where_scan and k_where_write.  The checks are those of tests/test_gpu_where.py (tests/where_checks.py), the
grid thinned to what the emulator runs in about a minute."""
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import NumpyMem
from helpers import orc_compress, ptr, ref_compress
from take_checks import BLOCKSIZE, many_chunks
from test_emu_library import emulib  # noqa: F401  (the fixture)
from test_emu_take import SETTINGS
import where_checks as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_where", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def env(emulib, pkgmod, oracle, ref):
    assert hasattr(emulib, "blosc_gpu_where_batch"), "the library has no where calls"

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
            if who == 2 and data.size <= W.N // 2: return lib_compress(data, T, shuffle, cname)
            return orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
        return write
    return W.Env(pkgmod, emulib, NumpyMem(), oracle, writer)


@pytest.mark.parametrize("kind,nbytes", W.KINDS, ids=[W.kind_name(*k) for k in W.KINDS])
def test_every_kind_width_and_op(env, kind, nbytes):
    at = W.KINDS.index((kind, nbytes))
    W.case_kind(env, kind, nbytes, SETTINGS[at % 3], W.thin_picks, turn=at)


@pytest.mark.parametrize("kind,nbytes", W.KINDS16, ids=[W.kind_name(*k) for k in W.KINDS16])
def test_every_16_bit_pattern_against_each_constant(env, kind, nbytes):
    """rows of 2 bytes, EQ / LT / GE against the four constants of the kind that sit on a change of regime (the device: both layouts, every
    constant, every op)"""
    W.case_patterns16(env, kind, W.LAYOUTS16[0], W.thin_constants16(kind), ops=(0, 2, 5), packed_ops=(), turn=W.KINDS16.index((kind, nbytes)))


@pytest.mark.parametrize("kind,nbytes", W.NEIGHBOUR_KINDS, ids=[W.kind_name(*k) for k in W.NEIGHBOUR_KINDS])
def test_neighbours_of_the_wide_kinds(env, kind, nbytes):
    at = W.NEIGHBOUR_KINDS.index((kind, nbytes))
    W.case_neighbours(env, kind, nbytes, SETTINGS[at % 3], W.thin_neighbour_picks(kind, nbytes), turn=at)


@pytest.mark.parametrize("layout", W.LAYOUTS, ids=[f"{l[0]}-at-{l[1]}" for l in W.LAYOUTS])
def test_row_layouts_and_both_entry_points(env, layout):
    at = W.LAYOUTS.index(layout)
    W.case_layout(env, layout, SETTINGS[(at + 1) % 3], turn=at, ops=(at % 6, (at + 2) % 6, (at + 4) % 6), packed_ops=(at % 6,))


@pytest.mark.parametrize("setting", SETTINGS[3:], ids=lambda s: f"{s[0]}-T{s[1]}-filter{s[2]}")
def test_split_typesizes(env, setting):
    """the settings whose blocks are widened to 64 KiB, at 8 N"""
    W.case_layout(env, W.LAYOUTS[3] if setting[1] == 4 else W.LAYOUTS[4], setting, turn=0, ops=(setting[1] // 4,), packed_ops=(2,))


@pytest.mark.parametrize("name", W.DENSITIES)
def test_densities(env, name):
    W.case_density(env, name, SETTINGS[W.DENSITIES.index(name) % 3], turn=W.DENSITIES.index(name))


def test_many_tiles(env):
    W.case_many_tiles(env, thin=True)


def test_more_tiles_in_a_pass_than_scan_threads(env):
    """1025 tiles in one pass: threads of k_where_scan with two tiles, one with one, the rest with none (the device: 1024 and 2051 tiles as
    well, and each with the table cut inside a late tile)"""
    W.case_wide_pass(env, "1025 tiles", thin=True)


def test_more_chunks_than_tiles_a_thread(env):
    """1300 small chunks, more than 1024 tiles, in one pass under EQ (the device: in dozens of passes of 16 KiB as well, and under NE with the table cut)"""
    W.case_many_chunks(env, many_chunks(env.oracle, env.writer("lz4", 4, 1, 0), 48, 1300), pass_bytes=(0,), thin=True)


def test_capacity(env):
    W.case_capacity(env, SETTINGS[1], turn=1)


def test_passes_give_the_same(env):
    W.case_passes(env, SETTINGS[2], W.LAYOUTS[2], turn=2)


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_a_chunk_that_does_not_decode(env, cname):
    W.case_damage(env, lambda data: orc_compress(env.oracle, data, 17, 5, 1, cname, blocksize=BLOCKSIZE)[1], cname, thin=(cname == "blosclz"))


def test_refused_calls(env):
    W.case_refused(env)


def test_row_where_helper(env):
    """RowWhere.batch / .packed: the class the tensors module drives gives what the raw calls give"""
    values = W.value_set(W.UINT, 4)
    layout = (12, 5, W.UINT, 4)
    chunks, rows_plain = W.table_call(env, SETTINGS[0], layout, W.drawn(values, W.total_rows(12)), turn=0)
    want = W.expected(rows_plain, 12, 5, W.UINT, 4, 0, values[1])
    pred = env.pkg.predicate(env.pkg.FIELD_UINT, 4, env.pkg.WHERE_EQ, values[1], offset=5)
    for src in W.both_sources(env, chunks):
        where = env.pkg.RowWhere(12, lib=env.lib)
        out = np.zeros(want.size, np.int64)
        rc = (where.packed(src.container, src.size, src.offsets, pred, out.ctypes.data, out.size) if src.packed
              else where.batch(src.ptrs, pred, out.ctypes.data, out.size))
        assert rc == 0 and where.total() == want.size and np.array_equal(out, want)
        assert where.chunk_rows() == W.chunk_rows(chunks, 12) and sum(where.chunk_matches()) == want.size and where.unread() == 0
