"""CPU: blpk.pack_device / blpk.unpack_device (c-blosc_amd/blpk.py) on the emulated library, with a numpy-backed `mem`: "device memory"
is host memory there.  pack_device must write byte for byte the file blpk.pack writes, and unpack_device must read both."""
import ctypes as C
import importlib.util
import io
import os
import struct
import zlib

import numpy as np
import pytest

from helpers import DATASETS, orc_compress
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CHUNK = 150000 + 8 * 13, 1 << 16            # three chunks, the last one short


def _module(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def blpk():
    return _module("blpk_for_emu", "c-blosc_amd", "blpk.py")


@pytest.fixture(scope="module")
def elib(emulib):
    pkgmod = _module("c_blosc_amd_for_emu", "c-blosc_amd", "__init__.py")
    assert hasattr(emulib, "blosc_gpu_checksum_packed"), "the library has no checksum calls"
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    emulib.blosc_gpu_compress_batch_host.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    emulib.blosc_gpu_decompress_batch_host.argtypes = [i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    pkgmod.declare_packed(emulib)
    pkgmod.declare_checksum(emulib)
    return emulib


class NumpyMem:
    """`mem` of pack_device / unpack_device over host arrays; counts what it is asked for"""

    def __init__(self):
        self.allocs, self.downloads, self.uploads = [], [], []

    def alloc(self, n):
        a = np.full(max(n, 1), 0xEE, np.uint8)
        self.allocs.append(n)
        return a.ctypes.data, a

    def to_host(self, ptr, n):
        self.downloads.append(n)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_ubyte)), (n,)).copy() if n else np.empty(0, np.uint8)

    def to_device(self, arr):
        a = np.array(arr, np.uint8)
        self.uploads.append(a.size)
        return a.ctypes.data, a


@pytest.fixture(scope="module")
def data():
    return DATASETS["bench19"](N)


def _files(blpk, elib, data, cname, checksum, **kw):
    a, b = io.BytesIO(), io.BytesIO()
    want = blpk.pack(elib, data, a, chunk_size=CHUNK, typesize=8, clevel=5, shuffle=1, cname=cname, checksum=checksum, **kw)
    mem = NumpyMem()
    got = blpk.pack_device(elib, data.ctypes.data, data.size, b, chunk_size=CHUNK, typesize=8, clevel=5, shuffle=1, cname=cname, checksum=checksum, mem=mem, **kw)
    assert got == want == (3, len(a.getvalue()))
    return a.getvalue(), b.getvalue(), mem


def _read(blpk, elib, blob, n, **kw):
    out = np.full(n + 64, 0xEE, np.uint8)
    mem = NumpyMem()
    assert blpk.unpack_device(elib, io.BytesIO(blob), out.ctypes.data, n, mem=mem, **kw) == n
    assert np.all(out[n:] == 0xEE) and mem.uploads == [len(blob)]
    return out[:n]


@pytest.mark.parametrize("cname,checksum", [(b"lz4", 1), (b"lz4", 2), (b"lz4", 0), (b"blosclz", 1), (b"blosclz", 2)])
def test_same_file_as_pack_and_round_trip(blpk, elib, data, cname, checksum):
    by_pack, by_device, mem = _files(blpk, elib, data, cname, checksum)
    assert by_device == by_pack
    assert len(mem.allocs) == 1 and len(mem.downloads) == 1 and mem.downloads[0] < mem.allocs[0]      # one container, one copy of the used bytes
    assert np.array_equal(_read(blpk, elib, by_pack, N), data)
    assert np.array_equal(_read(blpk, elib, by_device, N), data)
    assert np.array_equal(blpk.unpack(elib, io.BytesIO(by_device)), data)


def test_batches(blpk, elib, data):
    """a batch per chunk: the container is reused, the offsets go on counting"""
    by_pack, by_device, mem = _files(blpk, elib, data, b"lz4", 1, batch_bytes=CHUNK)
    assert by_device == by_pack and len(mem.allocs) == 1 and len(mem.downloads) == 3
    assert np.array_equal(_read(blpk, elib, by_device, N), data)


def _foreign_file(blpk, oracle, data, checksum=1):
    chunks = []
    for k in range(0, data.size, CHUNK):
        r, c = orc_compress(oracle, data[k:k + CHUNK], 8, 5, 1, "blosclz")
        assert r > 0
        chunks.append(c.tobytes())
    n = len(chunks)
    f = {1: zlib.adler32, 2: zlib.crc32}[checksum]
    pos = 32 + 8 * n; offs = []; body = b""
    for c in chunks:
        offs.append(pos + len(body)); body += c + struct.pack("<I", f(c) & 0xffffffff)
    return blpk.pack_header(n, CHUNK, data.size - (n - 1) * CHUNK, 8, checksum=checksum), offs, body


@pytest.mark.parametrize("checksum", [1, 2])
def test_foreign_file(blpk, elib, oracle, data, checksum):
    hdr, offs, body = _foreign_file(blpk, oracle, data, checksum)
    blob = hdr + np.array(offs, "<i8").tobytes() + body
    assert np.array_equal(_read(blpk, elib, blob, N), data)


def test_damaged_chunk_is_named(blpk, elib, oracle, data):
    hdr, offs, body = _foreign_file(blpk, oracle, data)
    blob = bytearray(hdr + np.array(offs, "<i8").tobytes() + body)
    k = 1
    blob[offs[k + 1] - 4 - 50] ^= 0x10                   # inside chunk 1's compressed bytes
    out = np.zeros(N, np.uint8)
    with pytest.raises(blpk.BlpkError, match=f"chunk {k}: checksum"):
        blpk.unpack_device(elib, io.BytesIO(bytes(blob)), out.ctypes.data, N, mem=NumpyMem())
    try:                                                   # not verified: whatever the decoder makes of it, nobody speaks of a checksum
        blpk.unpack_device(elib, io.BytesIO(bytes(blob)), out.ctypes.data, N, verify=False, mem=NumpyMem())
    except blpk.BlpkError as e:
        assert "checksum" not in str(e)
    # a damaged stored digest is a mismatch as well
    blob = bytearray(hdr + np.array(offs, "<i8").tobytes() + body)
    blob[-1] ^= 1
    with pytest.raises(blpk.BlpkError, match="chunk 2: checksum"):
        blpk.unpack_device(elib, io.BytesIO(bytes(blob)), out.ctypes.data, N, mem=NumpyMem())


def test_tables_this_path_does_not_take(blpk, elib, oracle, data):
    hdr, offs, body = _foreign_file(blpk, oracle, data)
    out = np.zeros(N, np.uint8)
    swapped = [offs[1], offs[0], offs[2]]
    with pytest.raises(blpk.BlpkError, match="use unpack"):
        blpk.unpack_device(elib, io.BytesIO(hdr + np.array(swapped, "<i8").tobytes() + body), out.ctypes.data, N, mem=NumpyMem())
    twice = [offs[0], offs[0], offs[2]]
    with pytest.raises(blpk.BlpkError, match="use unpack"):
        blpk.unpack_device(elib, io.BytesIO(hdr + np.array(twice, "<i8").tobytes() + body), out.ctypes.data, N, mem=NumpyMem())
    no_table = blpk.pack_header(3, CHUNK, N - 2 * CHUNK, 8, checksum=1, offsets=False)
    with pytest.raises(blpk.BlpkError, match="use unpack"):
        blpk.unpack_device(elib, io.BytesIO(no_table + body), out.ctypes.data, N, mem=NumpyMem())
    with pytest.raises(blpk.BlpkError):
        blpk.unpack_device(elib, io.BytesIO(hdr + np.array([offs[0], offs[1], 10**9], "<i8").tobytes() + body), out.ctypes.data, N, mem=NumpyMem())
    with pytest.raises(blpk.BlpkError):                   # a destination too small
        blpk.unpack_device(elib, io.BytesIO(hdr + np.array(offs, "<i8").tobytes() + body), out.ctypes.data, N - 1, mem=NumpyMem())
    assert not out.any()


def test_size_query_decodes_nothing(blpk, elib, oracle, data):
    hdr, offs, body = _foreign_file(blpk, oracle, data)

    class NoMem:
        def __getattr__(self, name):
            raise AssertionError("the size query touched device memory")
    assert blpk.unpack_device(None, io.BytesIO(hdr + np.array(offs, "<i8").tobytes() + body), mem=NoMem()) == N
    empty = io.BytesIO()
    assert blpk.pack_device(elib, 0, 0, empty, mem=NoMem()) == (0, 32)
    assert blpk.unpack_device(elib, io.BytesIO(empty.getvalue()), 0, 0, mem=NoMem()) == 0
