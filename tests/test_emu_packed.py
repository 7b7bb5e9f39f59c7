"""CPU: the packed batch calls (include/blosc_gpu_packed.h) on the emulated library - host engine, the layout step behind the size scan
(k_encode.hip: k_chunk_scan_packed, k_packed_layout, k_packed_headers), compaction into the caller's one buffer, and the reverse call.
The checkers are tests/test_gpu_packed.py's: the emulated blosc_gpu_compress_batch's bytes, the oracle, and the reference where it ships."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from helpers import DATASETS, orc_compress, ptr, ref_compress
from packed_checks import (FILL, GUARD, SETTINGS, SETTING_IDS, capacity_cases, check_chunks_decode, check_container, host_offsets,
                           mixed_batch)
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the mixed batch of the device test, shrunk for the emulator: a leftover block (64 KiB blocks: BLOCKSIZE x typesize, or the 64 KiB floor
# of a split block), nbytes 0, a chunk below 128 bytes (MEMCPYED on the host), random bytes (MEMCPYED by the scan)
EMU_SIZES = [1 << 16, (1 << 16) + 3001 * 8, 8 * 1000, 0, 100, (1 << 14) + 8, 1 << 12]
BLOCKSIZE = 8192


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def elib(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_compress_packed"), "the library has no packed calls"
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    emulib.blosc_gpu_compress_batch.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i), vp]
    pkgmod.declare_packed(emulib)
    return emulib


def batch_chunks(L, hosts, T, shuffle, cname, blocksize):
    """blosc_gpu_compress_batch with destsize nbytes + 16 for every chunk (on the emulator "device memory" is the host's)"""
    n = len(hosts)
    dst = [np.full(h.size + 16, FILL, np.uint8) for h in hosts]
    res = (C.c_int * n)()
    r = L.blosc_gpu_compress_batch(5, shuffle, T, cname, blocksize, n, (C.c_void_p * n)(*[h.ctypes.data for h in hosts]), (C.c_size_t * n)(*[h.size for h in hosts]),
                                   (C.c_void_p * n)(*[d.ctypes.data for d in dst]), (C.c_size_t * n)(*[d.size for d in dst]), res, None)
    assert r == 0 and all(c > 0 for c in res), list(res)
    return [d[:c].copy() for d, c in zip(dst, res)]


def packed(pkgmod, L, hosts, T, shuffle, cname, blocksize, align, destsize):
    b = pkgmod.PackedBatch(len(hosts), lib=L)
    buf = np.full(destsize + GUARD, FILL, np.uint8)
    r = b.compress([h.ctypes.data for h in hosts], [h.size for h in hosts], buf.ctypes.data, destsize, T, 5, shuffle, cname, blocksize, align)
    assert r == 0
    return b.offsets(), b.results(), buf


@pytest.mark.parametrize("cname,shuffle,T", SETTINGS, ids=SETTING_IDS)
def test_mixed_batch_every_fallback(elib, pkgmod, oracle, ref, cname, shuffle, T):
    hosts = mixed_batch(EMU_SIZES)
    chunks = batch_chunks(elib, hosts, T, shuffle, cname, BLOCKSIZE)
    flags = [int(c[2]) for c in chunks]
    assert flags[4] & 2 and flags[6] & 2 and not flags[2] & 2, flags          # MEMCPYED: below 128 bytes, random bytes; not the zeros
    bs = int(chunks[1][8:12].view("<i4")[0])
    assert bs < hosts[1].size and hosts[1].size % bs                            # full blocks and a leftover block
    for align in (1, 16, 4096):
        need = host_offsets([c.size for c in chunks], align)[-1]
        assert need <= pkgmod.PackedBatch(len(hosts), lib=elib).bound([h.size for h in hosts], align)
        off, cb, buf = packed(pkgmod, elib, hosts, T, shuffle, cname, BLOCKSIZE, align, need)
        check_container(buf, off, cb, chunks, align, need, (cname, align))
        assert off == host_offsets(cb, align)
        check_chunks_decode([buf[off[i]:off[i] + cb[i]] for i in range(len(hosts))], hosts, oracle, ref)


def test_more_chunks_than_one_workgroup_is_wide(elib, pkgmod, oracle, ref):
    rng = np.random.default_rng(300)
    sizes = [int(s) * 8 for s in rng.integers(1024 // 8, 3072 // 8 + 1, 300)]
    hosts = [DATASETS["bench19" if k % 3 else "random"](n) for k, n in enumerate(sizes)]
    chunks = batch_chunks(elib, hosts, 8, 1, b"lz4", 0)
    for align in (256,):                    # (a call takes the emulator 15 s: align 1 is the cut below)
        need = host_offsets([c.size for c in chunks], align)[-1]
        off, cb, buf = packed(pkgmod, elib, hosts, 8, 1, b"lz4", 0, align, need)
        check_container(buf, off, cb, chunks, align, need, align)
        check_chunks_decode([buf[off[i]:off[i] + cb[i]] for i in range(len(hosts))], hosts, oracle, ref)
    # a buffer that ends inside chunk 280: the tiles of the layout scan behind the first carry the offset on
    off1 = host_offsets([c.size for c in chunks], 1)
    cut = off1[280] + 5
    off, cb, buf = packed(pkgmod, elib, hosts, 8, 1, b"lz4", 0, 1, cut)
    check_container(buf, off, cb, chunks, 1, cut, "cut at chunk 280")
    assert all(c > 0 for c in cb[:280]) and not any(cb[280:]) and off[-1] == off1[-1]


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(elib, pkgmod, align):
    hosts = mixed_batch(EMU_SIZES)
    n = len(hosts)
    chunks = batch_chunks(elib, hosts, 8, 1, b"lz4", BLOCKSIZE)
    need = host_offsets([c.size for c in chunks], align)[-1]
    for name, destsize in capacity_cases(chunks, align):
        off, cb, buf = packed(pkgmod, elib, hosts, 8, 1, b"lz4", BLOCKSIZE, align, destsize)
        assert off[n] == need, (name, off[n], need)
        check_container(buf, off, cb, chunks, align, destsize, name)
        if name == "the need": assert all(c > 0 for c in cb)
        if name == "need - 1" and align == 1: assert all(c > 0 for c in cb[:-1]) and cb[-1] == 0
        if name.startswith("a cut"): assert all(c > 0 for c in cb[:3]) and not any(cb[3:])
        if name == "nothing": assert not any(cb)
    # no buffer at all: the sizing call
    b = pkgmod.PackedBatch(n, lib=elib)
    assert b.compress([h.ctypes.data for h in hosts], [h.size for h in hosts], None, 0, 8, 5, 1, b"lz4", BLOCKSIZE, align) == 0
    assert b.offsets() == host_offsets([c.size for c in chunks], align) and not any(b.results())


def test_unusable_arguments_and_parameter_errors(elib, pkgmod):
    hosts = mixed_batch(EMU_SIZES)[2:5]
    n = len(hosts)
    src, sizes = [h.ctypes.data for h in hosts], [h.size for h in hosts]
    buf = np.full(20000, FILL, np.uint8)
    b = pkgmod.PackedBatch(n, lib=elib)
    for align in (3, 8192, 48):
        assert b.compress(src, sizes, buf.ctypes.data, buf.size, 8, align=align) < 0
    assert b.compress(src, sizes, None, 16, 8) < 0                             # a size without a buffer
    assert np.all(buf == FILL)
    assert b.compress(src, sizes, buf.ctypes.data, buf.size, 8, clevel=11, align=16) == 0      # a parameter error: its code, no room taken
    assert b.results() == [-10] * n and b.offsets() == [0] * (n + 1) and np.all(buf == FILL)
    assert b.compress(src, sizes, buf.ctypes.data, buf.size, 8, cname=b"snappy") == 0
    assert b.results() == [-5] * n and b.offsets() == [0] * (n + 1)
    assert b.bound(sizes, 0) == sum(s + 16 for s in sizes) and b.bound(sizes, 3) == 0


def test_decompress_packed(elib, pkgmod, oracle, ref):
    """A container of reference-written chunks (the oracle's where the reference is not built) with junk between them."""
    hosts = mixed_batch(EMU_SIZES)
    n = len(hosts)
    rng = np.random.default_rng(5)
    chunks = [(ref_compress(ref, h, 8, 5, 1, b"lz4") if ref is not None else orc_compress(oracle, h, 8, 5, 1, "lz4"))[1] for h in hosts]
    parts, offs = [], [0]
    for k, c in enumerate(chunks):
        junk = rng.integers(0, 256, k * 5 % 16, dtype=np.uint8)
        parts += [c, junk]
        offs.append(offs[-1] + c.size + junk.size)
    cont = np.concatenate(parts)
    sizes = [h.size for h in hosts]
    total = sum(sizes)
    b = pkgmod.PackedBatch(n, lib=elib)
    # the size query
    assert b.decompress(cont.ctypes.data, cont.size, offs, None, 0) == 0
    assert b.results() == sizes and b.offsets() == host_offsets(sizes, 1)
    # the real call
    out = np.full(total + GUARD, FILL, np.uint8)
    assert b.decompress(cont.ctypes.data, cont.size, offs, out.ctypes.data, total) == 0
    assert b.results() == sizes and b.offsets() == host_offsets(sizes, 1)
    assert np.array_equal(out[:total], np.concatenate(hosts)) and np.all(out[total:] == FILL)
    # a damaged version byte: that chunk fails alone and takes no room
    bad = cont.copy(); bad[offs[1]] = 9
    want = [s if k != 1 else 0 for k, s in enumerate(sizes)]
    out[:] = FILL
    assert b.decompress(bad.ctypes.data, bad.size, offs, out.ctypes.data, total) == 0
    assert b.results() == [s if k != 1 else -1 for k, s in enumerate(sizes)] and b.offsets() == host_offsets(want, 1)
    assert np.array_equal(out[:total - sizes[1]], np.concatenate([h for k, h in enumerate(hosts) if k != 1])) and np.all(out[total - sizes[1]:] == FILL)
    # a destination that cuts the last chunk
    out[:] = FILL
    assert b.decompress(cont.ctypes.data, cont.size, offs, out.ctypes.data, total - 1) == 0
    assert b.results() == sizes[:-1] + [-1] and b.offsets() == host_offsets(sizes, 1)
    assert np.array_equal(out[:total - sizes[-1]], np.concatenate(hosts[:-1])) and np.all(out[total - sizes[-1]:] == FILL)
    # a header that claims more than its slot holds; a slot too short for a header
    tight = list(offs); tight[n] = offs[n - 1] + chunks[n - 1].size - 1
    assert b.decompress(cont.ctypes.data, cont.size, tight, None, 0) == 0 and b.results() == sizes[:-1] + [-1] and b.offsets()[n] == total - sizes[-1]
    empty = list(offs); empty[3] = empty[4]
    assert b.decompress(cont.ctypes.data, cont.size, empty, None, 0) == 0 and b.results()[3] == -1 and b.results()[2] == sizes[2]
    # tables that are unusable as a whole
    down = list(offs); down[2] = down[1] - 1
    assert b.decompress(cont.ctypes.data, cont.size, down, out.ctypes.data, total) < 0
    assert b.decompress(cont.ctypes.data, cont.size - 1, offs, out.ctypes.data, total) < 0
    # blosc_cbuffer_sizes, batched
    got = b.sizes([cont.ctypes.data + o for o in offs[:-1]])
    for k, c in enumerate(chunks):
        one = [C.c_size_t() for _ in range(3)]
        elib.blosc_cbuffer_sizes(ptr(c), *[C.byref(x) for x in one])
        assert [g[k] for g in got] == [x.value for x in one]
    assert elib.blosc_gpu_cbuffer_sizes_batch(n, (C.c_void_p * n)(*[cont.ctypes.data + o for o in offs[:-1]]), None, None, None, None) == 0
