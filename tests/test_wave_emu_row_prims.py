"""CPU: the pieces that the row kernels (k_take.hip, k_put.hip, k_where.hip, k_aggregate.hip) and k_getitem_gather share
(c-blosc_amd/csrc/row_prims.h: tile_owner, move_row, wave_copy_tile), each on its own on the wavefront emulator - the SAME source the
GPU runs - against numpy.  The call families (tests/test_emu_take.py, test_emu_put.py, ...) reach them through whole calls; here
every alignment case of a helper is one small run.  Destinations lie between canaries; with `guard` the entry point (tests/tools/
lz_wave_cpu.cpp) reads the source from a copy that ends at an unreadable page, so one byte read beyond it stops the run."""
import ctypes as C

import numpy as np
import pytest

from helpers import ptr
from test_wave_emu_encoders import emu  # noqa: F401

CANARY, FRESH = 0xEE, 0xCD      # around the destination / the destination before the call
ROOM = 64                       # canary bytes on each side


def _api(emu):
    emu.emu_tile_owner.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    emu.emu_tile_owner.restype = None
    emu.emu_move_row.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int]
    emu.emu_move_row.restype = None
    emu.emu_copy_tile.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_int]
    emu.emu_copy_tile.restype = None
    return emu


def _at(buf, residue, front=0):
    """the first offset >= front of buf whose address is `residue` modulo 16"""
    return front + (residue - (buf.ctypes.data + front)) % 16


class _Dest:
    """n bytes at an address `residue` modulo 16, ROOM canary bytes on both sides"""

    def __init__(self, n, residue):
        self.buf = np.full(ROOM + 16 + n + ROOM, CANARY, np.uint8)
        self.n, self.at = n, _at(self.buf, residue, ROOM)
        self.buf[self.at:self.at + n] = FRESH
        self.addr = self.buf.ctypes.data + self.at

    def check(self, want, what):
        got = self.buf[self.at:self.at + self.n]
        assert np.array_equal(got, want), (what, "first wrong byte", int(np.flatnonzero(got != want)[0]))
        assert np.all(self.buf[:self.at] == CANARY) and np.all(self.buf[self.at + self.n:] == CANARY), (what, "wrote outside the destination")


def _source(rng, n, residue):
    """n random bytes (never FRESH, CANARY or 0) at an address `residue` modulo 16, at the end of their buffer but for the alignment's slack"""
    buf = np.zeros(n + 15, np.uint8)
    at = _at(buf, residue)
    data = rng.integers(1, 200, n, dtype=np.uint8)
    buf[at:at + n] = data
    return buf, buf.ctypes.data + at, data


def _prefixes(n, rng):
    """tile counts per owner: owners without tiles at the front, in the middle, at the end, at all three, and at random"""
    base = rng.integers(1, 6, n)
    front, middle, end, three = base.copy(), base.copy(), base.copy(), base.copy()
    front[:max(1, n // 5)] = 0
    middle[n // 3:max(n // 3 + 1, 2 * n // 3)] = 0
    end[n - max(1, n // 5):] = 0
    three[0] = 0; three[n // 2] = 0; three[n - 1] = 0
    sparse = rng.integers(0, 3, n) * rng.integers(0, 2, n)
    return {"none empty": base, "front": front, "middle": middle, "end": end, "front, middle and end": three, "random": sparse}


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 1025])
def test_tile_owner_is_the_last_of_equal_entries(emu, n):
    e = _api(emu)
    rng = np.random.default_rng(n)
    checked = 0
    for name, counts in _prefixes(n, rng).items():
        tile_first = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        ntiles = int(tile_first[n])
        if not ntiles:      # (n = 1 with its one owner empty, ...: there is no tile to ask for)
            continue
        got = np.full(ntiles + 8, 0xFFFFFFFF, np.uint32)
        e.emu_tile_owner(ptr(tile_first), n, ptr(got))
        want = np.searchsorted(tile_first, np.arange(ntiles, dtype=np.uint32), side="right") - 1
        assert np.array_equal(got[:ntiles], want), (n, name)
        assert np.all(got[ntiles:] == 0xFFFFFFFF), (n, name)
        assert np.all(counts[got[:ntiles]] > 0), (n, name)      # never an owner without tiles
        checked += 1
    assert checked >= (1 if n == 1 else 3)


def _row_lanes_log2(row_bytes, misaligned):
    """engine.hip: row_lanes_log2, the host's rule for the lanes that move one row"""
    lanes_log2 = 0
    if row_bytes > 16:
        while (16 << lanes_log2) < row_bytes and lanes_log2 < 6:
            lanes_log2 += 1
        if misaligned and lanes_log2 < 4:
            lanes_log2 = 4
    return lanes_log2


@pytest.mark.parametrize("row_bytes", [1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 48, 100, 1024])
def test_move_row(emu, row_bytes):
    """every destination residue, source residues 0 / 1 / 8 / 15 and the guarded source, the host's group size and the next larger one"""
    e = _api(emu)
    rng = np.random.default_rng(row_bytes)
    for d_res in range(16):
        host = _row_lanes_log2(row_bytes, d_res != 0 or row_bytes % 16 != 0)
        for s_res in (0, 1, 8, 15, "guard"):
            keep, s_addr, data = _source(rng, row_bytes, 0 if s_res == "guard" else s_res)
            for lanes_log2 in (host, host + 1):
                d = _Dest(row_bytes, d_res)
                e.emu_move_row(d.addr, s_addr, row_bytes, lanes_log2, 1 if s_res == "guard" else 0)
                d.check(data, (row_bytes, d_res, s_res, lanes_log2))


def _live_values(n):
    return sorted({0, min(1, n), min(n, (n // 2) | 1), max(n - 1, 0), n})


def _tile_cases():
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025):
        yield n, range(16), (0, 3, "guard")
    for n in (16383, 16384):
        yield n, (0, 1, 15), (0, "guard")


@pytest.mark.parametrize("zeros", [0, 1], ids=["copy", "zeros behind live"])
def test_wave_copy_tile(emu, zeros):
    """k_getitem_gather's form (all n bytes from the source) and k_put_assemble's (`live` bytes from the source, zeros behind them; the
    guarded source holds `live` bytes and no more)"""
    e = _api(emu)
    rng = np.random.default_rng(7 + zeros)
    runs = 0
    for n, d_residues, s_residues in _tile_cases():
        for d_res in d_residues:
            for s_res in s_residues:
                for live in (_live_values(n) if zeros else [n]):
                    keep, s_addr, data = _source(rng, live, 0 if s_res == "guard" else s_res)
                    d = _Dest(n, d_res)
                    e.emu_copy_tile(zeros, d.addr, s_addr, n, live, 1 if s_res == "guard" else 0)
                    d.check(np.concatenate([data, np.zeros(n - live, np.uint8)]), (n, d_res, s_res, live))
                    runs += 1
    assert runs == (1644 if zeros else 396)      # (nothing above was skipped by accident)
