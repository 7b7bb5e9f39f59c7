"""CPU: include/blosc_gpu_checksum.h on the emulated library - the host side (tile table, one upload, two launches), k_checksum_tiles
and k_checksum_combine of c-blosc_amd/csrc/k_checksum.hip.  The yardstick is Python's zlib for both digests.  The tile is set to 4 KiB
through the exported hook so that the cases around one and three tiles stay small; one case runs the default tile."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from checksum_checks import (KIND_IDS, KINDS, LONG_COUNTS, ZLIB, aligned_copy, alignment_case, check_runs, expected, grid_case, lay_out, long_search_case,
                             many_runs_case)
from packed_checks import mixed_batch
from test_emu_library import emulib  # noqa: F401  (the fixture)
from test_emu_packed import BLOCKSIZE, EMU_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def elib(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_checksum_batch"), "the library has no checksum calls"
    pkgmod.declare_packed(emulib)
    pkgmod.declare_checksum(emulib)
    emulib.blosc_amd_checksum_tile_bytes(TILE)
    yield emulib
    emulib.blosc_amd_checksum_tile_bytes(0)


@pytest.fixture(scope="module")
def grid():
    buf, runs = grid_case(TILE)
    return aligned_copy(buf), runs


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lengths_and_contents(elib, pkgmod, grid, kind):
    buf, runs = grid
    check_runs(pkgmod, elib, kind, buf.ctypes.data, buf, runs, "grid")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_the_default_tile(elib, pkgmod, kind):
    """two tiles and a tail of the size the product runs with"""
    rng = np.random.default_rng(14)
    buf, runs = lay_out([rng.integers(0, 256, (512 << 10) + 7, dtype=np.uint8), np.full((256 << 10) + 1, 0xFF, np.uint8)], shifts=[3, 0])
    buf = aligned_copy(buf)
    elib.blosc_amd_checksum_tile_bytes(0)
    try:
        check_runs(pkgmod, elib, kind, buf.ctypes.data, buf, runs, "default tile")
    finally:
        elib.blosc_amd_checksum_tile_bytes(TILE)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_neighbouring_bytes_do_not_leak(elib, pkgmod, kind):
    buf, runs = alignment_case()
    buf = aligned_copy(buf)
    assert buf.ctypes.data % 16 == 0 and [o % 16 for o, _ in runs] == list(range(16))
    check_runs(pkgmod, elib, kind, buf.ctypes.data, buf, runs, "alignment")
    other = buf.copy(); other = aligned_copy(other)
    mask = np.ones(buf.size, bool)
    for o, n in runs:
        mask[o:o + n] = False
    other[mask] = 0x3C                                   # other neighbours, the same digests
    check_runs(pkgmod, elib, kind, other.ctypes.data, other, runs, "alignment, other neighbours")
    assert expected(kind, other, runs) == expected(kind, buf, runs)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_more_runs_than_one_workgroup_is_wide(elib, pkgmod, kind):
    buf, runs = many_runs_case()
    assert len(runs) == 300 and sum(1 for _, n in runs if n == 0) >= 4
    check_runs(pkgmod, elib, kind, buf.ctypes.data, buf, runs, "300 runs")


@pytest.mark.parametrize("nruns", LONG_COUNTS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_more_runs_than_two_rounds_of_the_search(elib, pkgmod, kind, nruns):
    """4096 runs are found in two rounds of the 64-way search of a tile's run, 4097 and 5000 take a third; stretches of 70 and 4100 empty runs"""
    buf, runs = long_search_case(nruns)
    assert len(runs) == nruns
    buf = aligned_copy(buf)
    check_runs(pkgmod, elib, kind, buf.ctypes.data, buf, runs, f"{nruns} runs")


@pytest.mark.parametrize("align", [1, 16])
def test_container_of_compress_packed(elib, pkgmod, align):
    hosts = mixed_batch(EMU_SIZES)
    b = pkgmod.PackedBatch(len(hosts), lib=elib)
    room = b.bound([h.size for h in hosts], align)
    cont = np.full(room, 0xEE, np.uint8)
    assert b.compress([h.ctypes.data for h in hosts], [h.size for h in hosts], cont.ctypes.data, room, 8, 5, 1, b"lz4", BLOCKSIZE, align) == 0
    off, cb = b.offsets(), b.results()
    assert all(c > 0 for c in cb)
    for kind in KINDS:
        got = pkgmod.checksums_packed(kind, cont.ctypes.data, room, off, cb, lib=elib)
        assert got == [ZLIB[kind](cont[off[i]:off[i] + cb[i]].tobytes()) for i in range(len(hosts))], (kind, "length = cbytes")
        got = pkgmod.checksums_packed(kind, cont.ctypes.data, room, off, None, lib=elib)
        assert got == [ZLIB[kind](cont[off[i]:off[i + 1]].tobytes()) for i in range(len(hosts))], (kind, "length = NULL")


def test_whole_call_errors_leave_the_digests_alone(elib):
    buf = np.arange(64, dtype=np.uint8)
    dig = (C.c_uint * 2)(0xDEAD, 0xBEEF)
    ptrs = (C.c_void_p * 2)(buf.ctypes.data, buf.ctypes.data + 10)
    sizes = (C.c_size_t * 2)(10, 20)
    off = (C.c_size_t * 3)(0, 10, 30)
    for kind in (0, 3):
        assert elib.blosc_gpu_checksum_batch(kind, 2, ptrs, sizes, dig, None) < 0
        assert elib.blosc_gpu_checksum_packed(kind, 2, buf.ctypes.data, buf.size, off, None, dig, None) < 0
    assert elib.blosc_gpu_checksum_packed(1, 2, buf.ctypes.data, buf.size, (C.c_size_t * 3)(0, 10, 9), None, dig, None) < 0      # offsets decrease
    assert elib.blosc_gpu_checksum_packed(1, 2, buf.ctypes.data, buf.size, off, (C.c_size_t * 2)(11, 20), dig, None) < 0         # a length beyond its span
    assert elib.blosc_gpu_checksum_packed(1, 2, buf.ctypes.data, 29, off, None, dig, None) < 0                                    # offsets[n] > containersize
    assert list(dig) == [0xDEAD, 0xBEEF]
    assert elib.blosc_gpu_checksum_packed(2, 2, buf.ctypes.data, buf.size, off, None, dig, None) == 0
    assert list(dig) == [ZLIB[2](buf[:10].tobytes()), ZLIB[2](buf[10:30].tobytes())]
    assert elib.blosc_gpu_checksum_batch(1, 0, None, None, None, None) == 0
    # an empty run's pointer is never read
    ptrs = (C.c_void_p * 2)(None, buf.ctypes.data); sizes = (C.c_size_t * 2)(0, 5)
    for kind, empty in ((1, 1), (2, 0)):
        assert elib.blosc_gpu_checksum_batch(kind, 2, ptrs, sizes, dig, None) == 0 and list(dig) == [empty, ZLIB[kind](buf[:5].tobytes())]
