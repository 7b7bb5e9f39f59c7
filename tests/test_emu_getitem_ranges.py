"""CPU: blosc_gpu_getitem_batch / blosc_gpu_getitem_packed (include/blosc_gpu_getitem.h) and the single calls blosc_getitem / blosc_gpu_getitem
on the emulated library - the host engine's range validation, runs, tables and passes, the decode kernels' per-block status words and k_getitem_gather.  The checks are those of
tests/test_gpu_getitem_ranges.py (tests/getitem_ranges_checks.py), the chunk grid thinned to what the emulator decodes in seconds."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from getitem_ranges_checks import (BIG, BLOCKSIZE, SENTINEL, SMALL, NumpyMem, check_batch, check_damage, check_single, chunk_ranges, damaged_single_chunks,
                                   expected, pick_damage, plain, prefix, single_grid_chunks)
from helpers import header, orc_compress, ptr, ref_compress
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_getitem", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def elib(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_getitem_batch"), "the library has no batched getitem"
    pkgmod.declare_getitem(emulib)
    pkgmod.declare_packed(emulib)
    emulib.blosc_gpu_getitem.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return emulib


def lib_compress(L, data, T, shuffle, cname, blocksize):
    out = np.zeros(data.size + 16, np.uint8)
    r = L.blosc_compress_ctx(5, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname, blocksize, 1)
    assert r > 0
    return out[:r].copy()


@pytest.fixture(scope="module")
def chunks(elib, oracle, ref):
    """LZ4 and BloscLZ: typesize 17 (six blocks of 8177 bytes) in every filter mode, the split typesizes (one block at this size) in one
    mode each, one chunk of 64 KiB blocks; written by the oracle, by the reference where it is built, by the emulated library; the specials"""
    small, big = plain(SMALL), plain(BIG)
    rng = np.random.default_rng(3)
    out = []
    for k, (T, shuffle) in enumerate([(17, 0), (17, 1), (17, 2), (1, 0), (2, 1), (4, 2), (8, 1)]):
        for cname in ("lz4", "blosclz"):
            writer = (k + (cname == "lz4")) % 3
            if writer == 1 and ref is not None: out.append(ref_compress(ref, small, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1])
            elif writer == 2: out.append(lib_compress(elib, small, T, shuffle, cname.encode(), BLOCKSIZE))
            else: out.append(orc_compress(oracle, small, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1])
    out.append(orc_compress(oracle, big, 4, 5, 1, "lz4", blocksize=BLOCKSIZE)[1])
    out.append(orc_compress(oracle, rng.integers(0, 256, 9000, dtype=np.uint8), 4, 5, 1, "lz4")[1])      # MEMCPYED: random bytes
    out.append(orc_compress(oracle, plain(100), 4, 5, 1, "lz4")[1])                                    # 100 bytes
    out.append(orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1])                                      # nbytes 0
    assert header(out[-3])["flags"] & 2 and header(out[-1])["nbytes"] == 0
    assert sum(-(-header(c)["nbytes"] // header(c)["blocksize"]) == 6 for c in out[:-3]) >= 7
    return out


def all_ranges(chunks):
    r = [(ci, s, k) for ci, c in enumerate(chunks) for s, k in chunk_ranges(c)]
    return r + [(len(chunks), 0, 1)]


def test_one_batch_over_every_chunk(elib, pkgmod, oracle, chunks):
    got = check_batch(pkgmod, elib, NumpyMem(), oracle, chunks, all_ranges(chunks))
    assert sum(g > 0 for g in got) > 8 * len(chunks) and got[-1] == -1


def test_passes_depend_on_bytes_and_give_the_same(elib, pkgmod, oracle, chunks):
    """a pass bound of 16 KiB: every chunk of more than two blocks is a pass of its own"""
    sub = chunks[:6] + chunks[-3:]
    ranges = all_ranges(sub)[::-1]              # ... and the ranges in another order than the chunks
    elib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        check_batch(pkgmod, elib, NumpyMem(), oracle, sub, ranges, "16 KiB passes")
    finally:
        elib.blosc_amd_getitem_pass_bytes(0)


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_a_damaged_block_fails_the_ranges_that_touch_it(elib, pkgmod, oracle, cname):
    chunk = orc_compress(oracle, plain(SMALL), 17, 5, 1, cname, blocksize=BLOCKSIZE)[1]
    found, rngs = pick_damage(oracle, chunk)
    for kind, bad in found:
        ranges = [(0, s, k) for s, k in rngs] + [(1, s, k) for s, k in rngs]      # chunk 1: the intact copy, same blocks in the same call
        got = check_batch(pkgmod, elib, NumpyMem(), oracle, [bad, chunk], ranges, (cname, kind))
        assert got[0] < 0 and got[1] == 7 * 17 and got[2] < 0 and got[3:] == [7 * 17] * 3, (kind, got)


def test_packed(elib, pkgmod, oracle):
    mem = NumpyMem()
    rng = np.random.default_rng(4)
    hosts = [plain(SMALL), rng.integers(0, 256, 9000, dtype=np.uint8), plain(100), plain(0), plain(3 * 8177 + 5, seed=5)]
    n = len(hosts)
    for cname, shuffle, T in ((b"lz4", 1, 17), (b"blosclz", 2, 4)):
        pb = pkgmod.PackedBatch(n, lib=elib)
        cap = pb.bound([h.size for h in hosts], 256)
        cont = np.zeros(cap, np.uint8)
        assert pb.compress([h.ctypes.data if h.size else None for h in hosts], [h.size for h in hosts], cont.ctypes.data, cap, T, 5, shuffle, cname, BLOCKSIZE, 256) == 0
        off, cb = pb.offsets(), pb.results()
        assert all(c > 0 for c in cb) and all(o % 256 == 0 for o in off)
        chunks = [cont[off[i]:off[i] + cb[i]].copy() for i in range(n)]
        ranges = [(ci, s, k) for ci, c in enumerate(chunks) for s, k in chunk_ranges(c)] + [(n, 0, 1)]
        want = expected(oracle, chunks, ranges)
        res, offs = [r for r, _ in want], prefix([r for r, _ in want])
        b = pkgmod.ItemRanges(ranges, lib=elib)
        # the size query
        assert b.packed(cont.ctypes.data, cap, off, None, 0) == 0
        assert b.results() == res and b.offsets() == offs
        # a dest of exactly that size
        total = offs[-1]
        out = np.full(total + 64, SENTINEL, np.uint8)
        assert b.packed(cont.ctypes.data, cap, off, out.ctypes.data, total) == 0
        assert b.results() == res and b.offsets() == offs
        exp = np.concatenate([d for r, d in want if r > 0])
        assert np.array_equal(out[:total], exp) and np.all(out[total:] == SENTINEL)
        # one byte short: the last valid range answers -1, everything before it is intact
        last = max(k for k, r in enumerate(res) if r > 0)
        out[:] = SENTINEL
        assert b.packed(cont.ctypes.data, cap, off, out.ctypes.data, total - 1) == 0
        assert b.results() == res[:last] + [-1] + res[last + 1:]
        assert np.array_equal(out[:offs[last]], exp[:offs[last]]) and np.all(out[offs[last]:] == SENTINEL)
    # an offset table built by hand, the slot of chunk 1 eight bytes short of its cbytes: every range of that chunk answers -1
    chunks = [orc_compress(oracle, plain(SMALL), 17, 5, 1, "lz4", blocksize=BLOCKSIZE)[1] for _ in range(3)]
    offs, parts = [0], []
    for k, c in enumerate(chunks):
        part = c[:c.size - 8] if k == 1 else c
        parts.append(part); offs.append(offs[-1] + part.size)
    cont = np.concatenate(parts)
    ranges = [(ci, s, k) for ci in range(3) for s, k in chunk_ranges(chunks[ci])[:7]]
    want = expected(oracle, chunks, ranges)
    res = [-1 if ci == 1 else r for (ci, _, _), (r, _) in zip(ranges, want)]
    b = pkgmod.ItemRanges(ranges, lib=elib)
    out = np.full(prefix(res)[-1] + 64, SENTINEL, np.uint8)
    assert b.packed(cont.ctypes.data, cont.size, offs, out.ctypes.data, out.size - 64) == 0
    assert b.results() == res and b.offsets() == prefix(res)
    assert np.array_equal(out[:out.size - 64], np.concatenate([d for (ci, _, _), (r, d) in zip(ranges, want) if ci != 1 and r > 0]))
    # tables that are unusable as a whole
    assert b.packed(cont.ctypes.data, cont.size - 1, offs, None, 0) < 0
    assert b.packed(cont.ctypes.data, cont.size, [0, 5, 4, offs[-1]], None, 0) < 0


# ---- the single calls: one range of one chunk through the same pipeline (the emulator's "device" memory is the host's, so each entry point runs as it is) ----
def single_calls(elib):
    return [("blosc_getitem", elib.blosc_getitem), ("blosc_gpu_getitem", lambda src, s, k, dst: elib.blosc_gpu_getitem(src, s, k, dst, None))]


@pytest.fixture(scope="module")
def single_chunks(elib, oracle, ref):
    return single_grid_chunks(oracle, ref, lambda d, T, shuffle, cname, bs: lib_compress(elib, d, T, shuffle, cname.encode(), bs))


@pytest.mark.parametrize("entry", [0, 1], ids=["blosc_getitem", "blosc_gpu_getitem"])
def test_single_call_grid(elib, oracle, ref, single_chunks, entry):
    name, call = single_calls(elib)[entry]
    for cname, chunk in single_chunks:
        got = check_single(call, NumpyMem(), NumpyMem(), oracle, ref, chunk, chunk_ranges(chunk), (name, cname))
        assert got[-2] == -1                                       # start = -1


@pytest.mark.parametrize("entry", [0, 1], ids=["blosc_getitem", "blosc_gpu_getitem"])
def test_single_call_in_passes(elib, oracle, ref, single_chunks, entry):
    """a pass bound of 16 KiB: a single chunk beyond the bound still decodes, as a pass of its own"""
    name, call = single_calls(elib)[entry]
    elib.blosc_amd_getitem_pass_bytes(16 << 10)
    try:
        for cname, chunk in single_chunks:
            check_single(call, NumpyMem(), NumpyMem(), oracle, ref, chunk, chunk_ranges(chunk), (name, cname, "16 KiB passes"))
    finally:
        elib.blosc_amd_getitem_pass_bytes(0)


def test_single_call_on_damaged_blocks(elib, oracle, ref):
    damaged = damaged_single_chunks(oracle, ref, lambda d, T, shuffle, cname, bs: lib_compress(elib, d, T, shuffle, cname.encode(), bs))
    assert len({n.split(",")[0] for n, _, _ in damaged}) == 4
    for name, call in single_calls(elib):
        check_damage(call, NumpyMem(), NumpyMem(), oracle, ref, damaged, name)
