"""c-blosc_amd — Python-side loader for libblosc_amd.so (ctypes; test / bench plumbing only).

The product is the C-ABI shared library built from ``csrc/`` (see ``include/blosc.h`` and
``include/blosc_gpu.h``, ``include/blosc_gpu_packed.h``, ``include/blosc_gpu_params.h``, ``include/blosc_gpu_getitem.h``, ``include/blosc_gpu_checksum.h``).  This module only locates it, declares argument types and offers small
numpy conveniences that mirror how the reference is driven from Python through ctypes
(SURVEY.md §A.8).  There is no CPU implementation here: if the library is missing, ``load()``
raises; if there is no GPU, the library's calls return errors.

The directory name contains a hyphen (it mirrors the reference's repository name), so import it
with ``importlib`` — ``tests/conftest.py`` and ``__graft_entry__.py`` show how.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLOSC_AMD_LIB", os.path.join(_HERE, "libblosc_amd.so"))   # override: tuning experiments only

STOCK_SYMBOLS = [
    "blosc_init", "blosc_destroy", "blosc_compress", "blosc_compress_ctx", "blosc_decompress",
    "blosc_decompress_ctx", "blosc_getitem", "blosc_get_nthreads", "blosc_set_nthreads",
    "blosc_get_compressor", "blosc_set_compressor", "blosc_compcode_to_compname",
    "blosc_compname_to_compcode", "blosc_list_compressors", "blosc_get_version_string",
    "blosc_get_complib_info", "blosc_free_resources", "blosc_cbuffer_sizes", "blosc_cbuffer_validate",
    "blosc_cbuffer_metainfo", "blosc_cbuffer_versions", "blosc_cbuffer_complib", "blosc_get_blocksize",
    "blosc_set_blocksize", "blosc_set_splitmode",
]
GPU_SYMBOLS = [
    "blosc_gpu_set_device", "blosc_gpu_compress_batch", "blosc_gpu_decompress_batch", "blosc_gpu_getitem",
    "blosc_gpu_compress_batch_host", "blosc_gpu_decompress_batch_host",
    "blosc_gpu_device_count", "blosc_gpu_partition", "blosc_gpu_compress_batch_multi", "blosc_gpu_decompress_batch_multi",
    "blosc_gpu_profile", "blosc_gpu_profile_reset", "blosc_gpu_profile_get",
]
PACKED_SYMBOLS = [      # include/blosc_gpu_packed.h
    "blosc_gpu_packed_bound", "blosc_gpu_compress_packed", "blosc_gpu_decompress_packed", "blosc_gpu_cbuffer_sizes_batch",
]
GETITEM_SYMBOLS = [     # include/blosc_gpu_getitem.h
    "blosc_gpu_getitem_batch", "blosc_gpu_getitem_packed",
]
CHECKSUM_SYMBOLS = [    # include/blosc_gpu_checksum.h
    "blosc_gpu_checksum_batch", "blosc_gpu_checksum_packed",
]
PARAMS_SYMBOLS = [      # include/blosc_gpu_params.h
    "blosc_gpu_compress_batch_params", "blosc_gpu_compress_packed_params",
]
CHECKSUM_ADLER32, CHECKSUM_CRC32 = 1, 2
COMPCODES = {b"blosclz": 0, b"lz4": 1, b"lz4hc": 2, b"snappy": 3, b"zlib": 4, b"zstd": 5}      # include/blosc.h


class CParams(C.Structure):
    """blosc_gpu_cparams (include/blosc_gpu_params.h): one chunk's compression parameters"""
    _fields_ = [("clevel", C.c_int), ("doshuffle", C.c_int), ("compcode", C.c_int), ("splitmode", C.c_int),
                ("typesize", C.c_size_t), ("blocksize", C.c_size_t)]


def cparams(typesize, clevel=5, shuffle=1, cname=b"lz4", blocksize=0, splitmode=0):
    """A CParams from the arguments DeviceBatch.compress takes; cname: a name (bytes or str), a compcode, or None for the global compressor."""
    if cname is None:
        code = -1
    elif isinstance(cname, int):
        code = cname
    else:
        code = COMPCODES[cname.encode() if isinstance(cname, str) else cname]
    return CParams(clevel, shuffle, code, splitmode, typesize, blocksize)


def params_table(params):
    """The host array of blosc_gpu_cparams a call takes, from a list of CParams (or of argument tuples / dicts of cparams())"""
    rows = [p if isinstance(p, CParams) else (cparams(**p) if isinstance(p, dict) else cparams(*p)) for p in params]
    return (CParams * max(len(rows), 1))(*rows)

_lib = None


def load():
    """Return the ctypes handle of libblosc_amd.so with argtypes/restypes declared."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: build it with `make -C {_HERE}` (hipcc, gfx950). "
            "There is no fallback implementation.")
    L = C.CDLL(LIB_PATH)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.blosc_compress.argtypes = [i, i, sz, sz, vp, vp, sz]
    L.blosc_compress_ctx.argtypes = [i, i, sz, sz, vp, vp, sz, C.c_char_p, sz, i]
    L.blosc_decompress.argtypes = [vp, vp, sz]
    L.blosc_decompress_ctx.argtypes = [vp, vp, sz, i]
    L.blosc_getitem.argtypes = [vp, i, i, vp]
    L.blosc_set_compressor.argtypes = [C.c_char_p]
    L.blosc_get_compressor.restype = C.c_char_p
    L.blosc_list_compressors.restype = C.c_char_p
    L.blosc_get_version_string.restype = C.c_char_p
    L.blosc_cbuffer_complib.restype = C.c_char_p
    L.blosc_cbuffer_complib.argtypes = [vp]
    L.blosc_compname_to_compcode.argtypes = [C.c_char_p]
    L.blosc_compcode_to_compname.argtypes = [i, C.POINTER(C.c_char_p)]
    L.blosc_get_complib_info.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    L.blosc_cbuffer_sizes.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
    L.blosc_cbuffer_sizes.restype = None
    L.blosc_cbuffer_validate.argtypes = [vp, sz, C.POINTER(sz)]
    L.blosc_cbuffer_metainfo.argtypes = [vp, C.POINTER(sz), C.POINTER(i)]
    L.blosc_cbuffer_metainfo.restype = None
    L.blosc_cbuffer_versions.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
    L.blosc_cbuffer_versions.restype = None
    L.blosc_set_blocksize.argtypes = [sz]
    L.blosc_set_blocksize.restype = None
    L.blosc_set_splitmode.argtypes = [i]
    L.blosc_set_splitmode.restype = None
    L.blosc_gpu_compress_batch.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz),
                                           C.POINTER(vp), C.POINTER(sz), C.POINTER(i), vp]
    L.blosc_gpu_decompress_batch.argtypes = [i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz),
                                             C.POINTER(i), vp]
    L.blosc_gpu_compress_batch_host.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    L.blosc_gpu_decompress_batch_host.argtypes = [i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    if hasattr(L, "blosc_gpu_partition"):        # (A/B scripts also load builds of earlier rounds through this loader)
        L.blosc_gpu_partition.argtypes = [sz, i, i, C.POINTER(sz), C.POINTER(sz)]
        L.blosc_gpu_compress_batch_multi.argtypes = [i, C.POINTER(i), i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz),
                                                     C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
        L.blosc_gpu_decompress_batch_multi.argtypes = [i, C.POINTER(i), i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i)]
    if hasattr(L, "blosc_gpu_compress_packed"):
        declare_packed(L)
    if hasattr(L, "blosc_gpu_compress_batch_params"):
        declare_params(L)
    if hasattr(L, "blosc_gpu_getitem_batch"):
        declare_getitem(L)
    if hasattr(L, "blosc_gpu_checksum_batch"):
        declare_checksum(L)
    L.blosc_gpu_getitem.argtypes = [vp, i, i, vp, vp]
    L.blosc_gpu_profile.argtypes = [i]
    L.blosc_gpu_profile.restype = None
    L.blosc_gpu_profile_reset.restype = None
    L.blosc_gpu_profile_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(i)]
    for name in ("blosc_internal_shuffle", "blosc_internal_unshuffle"):
        getattr(L, name).argtypes = [sz, sz, vp, vp]
        getattr(L, name).restype = None
    for name in ("blosc_internal_bitshuffle", "blosc_internal_bitunshuffle"):
        getattr(L, name).argtypes = [sz, sz, vp, vp, vp]
    if hasattr(L, "blosc_amd_policy_blocksize"):
        L.blosc_amd_policy_blocksize.argtypes = [i, i, i, i, i, i]
        L.blosc_amd_policy_split.argtypes = [i, i, i, i]
    _lib = L
    return L


def declare_packed(L):
    """argtypes of include/blosc_gpu_packed.h on a library handle (load() calls it; the CPU tests call it on their emulator build)."""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.blosc_gpu_packed_bound.argtypes = [i, C.POINTER(sz), sz]
    L.blosc_gpu_packed_bound.restype = sz
    L.blosc_gpu_compress_packed.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz), vp, sz, sz,
                                            C.POINTER(sz), C.POINTER(i), vp]
    L.blosc_gpu_decompress_packed.argtypes = [i, vp, sz, C.POINTER(sz), vp, sz, C.POINTER(sz), C.POINTER(i), vp]
    L.blosc_gpu_cbuffer_sizes_batch.argtypes = [i, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz), C.POINTER(sz), vp]


def declare_params(L):
    """argtypes of include/blosc_gpu_params.h on a library handle (load() calls it; the CPU tests call it on their emulator build)."""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.blosc_gpu_compress_batch_params.argtypes = [i, C.POINTER(CParams), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i), vp]
    L.blosc_gpu_compress_packed_params.argtypes = [i, C.POINTER(CParams), C.POINTER(vp), C.POINTER(sz), vp, sz, sz, C.POINTER(sz), C.POINTER(i), vp]


def declare_getitem(L):
    """argtypes of include/blosc_gpu_getitem.h on a library handle (load() calls it; the CPU tests call it on their emulator build)."""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    ip = C.POINTER(i)
    L.blosc_gpu_getitem_batch.argtypes = [i, C.POINTER(vp), i, ip, ip, ip, C.POINTER(vp), ip, vp]
    L.blosc_gpu_getitem_packed.argtypes = [i, vp, sz, C.POINTER(sz), i, ip, ip, ip, vp, sz, C.POINTER(sz), ip, vp]
    L.blosc_amd_getitem_pass_bytes.argtypes = [sz]      # (test hook)
    L.blosc_amd_getitem_pass_bytes.restype = None


def declare_checksum(L):
    """argtypes of include/blosc_gpu_checksum.h on a library handle (load() calls it; the CPU tests call it on their emulator build)."""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.blosc_gpu_checksum_batch.argtypes = [i, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(C.c_uint), vp]
    L.blosc_gpu_checksum_packed.argtypes = [i, i, vp, sz, C.POINTER(sz), C.POINTER(sz), C.POINTER(C.c_uint), vp]
    L.blosc_amd_checksum_tile_bytes.argtypes = [sz]     # (test hook)
    L.blosc_amd_checksum_tile_bytes.restype = None


# ---- numpy conveniences (host buffers through the stock entry points) --------------------------
def compress(arr, typesize, clevel=5, shuffle=1, cname=b"lz4", blocksize=0, destsize=None):
    """blosc_compress_ctx on a numpy array; returns (return_code, bytes-or-None)."""
    import numpy as np
    L = load()
    a = np.ascontiguousarray(arr).view(np.uint8).ravel()
    cap = a.size + 16 if destsize is None else destsize
    out = np.empty(max(cap, 1), np.uint8)
    r = L.blosc_compress_ctx(clevel, shuffle, typesize, a.size, a.ctypes.data, out.ctypes.data, cap, cname, blocksize, 1)
    return r, (out[:r].copy() if r > 0 else None)


def decompress(chunk, nbytes):
    """blosc_decompress_ctx of a numpy uint8 chunk into a fresh array of nbytes."""
    import numpy as np
    L = load()
    c = np.ascontiguousarray(chunk)
    out = np.zeros(max(nbytes, 1), np.uint8)
    r = L.blosc_decompress_ctx(c.ctypes.data, out.ctypes.data, nbytes, 1)
    return r, out[:max(r, 0)]


class DeviceBatch:
    """Helper for the device-resident batched API: keeps the ctypes pointer/size arrays alive."""

    def __init__(self, src_ptrs, src_sizes, dst_ptrs, dst_sizes):
        n = len(src_ptrs)
        self.n = n
        self.src = (C.c_void_p * n)(*src_ptrs)
        self.dst = (C.c_void_p * n)(*dst_ptrs)
        self.ssz = (C.c_size_t * n)(*src_sizes)
        self.dsz = (C.c_size_t * n)(*dst_sizes)
        self.res = (C.c_int * n)()

    def compress(self, typesize, clevel=5, shuffle=1, cname=b"lz4", blocksize=0, stream=None):
        return load().blosc_gpu_compress_batch(clevel, shuffle, typesize, cname, blocksize, self.n, self.src,
                                               self.ssz, self.dst, self.dsz, self.res, stream)

    def compress_params(self, params, stream=None, lib=None):
        """chunk i with params[i] (include/blosc_gpu_params.h; params: see params_table), the whole batch in one call"""
        assert len(params) == self.n
        return (lib if lib is not None else load()).blosc_gpu_compress_batch_params(self.n, params_table(params), self.src, self.ssz, self.dst, self.dsz,
                                                                                    self.res, stream)

    def decompress(self, stream=None, with_srcsize=True):
        return load().blosc_gpu_decompress_batch(self.n, self.src, self.ssz if with_srcsize else None, self.dst,
                                                 self.dsz, self.res, stream)

    def results(self):
        return list(self.res)


class PackedBatch:
    """Helper for the packed calls (include/blosc_gpu_packed.h): the whole batch in one device buffer, chunk i at its offset.

    compress(): n sources -> one container; offsets() / results() give the offset table [n + 1] and the per-chunk cbytes.
    decompress(): a container and its offset table -> one buffer of plain bytes (dest 0 / None: the size query).
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, n, lib=None):
        self.n = n
        self.lib = lib if lib is not None else load()
        self.off = (C.c_size_t * (n + 1))()
        self.res = (C.c_int * n)()

    def bound(self, sizes, align=1):
        return self.lib.blosc_gpu_packed_bound(self.n, (C.c_size_t * self.n)(*sizes), align)

    def compress(self, src_ptrs, src_sizes, dest, destsize, typesize, clevel=5, shuffle=1, cname=b"lz4", blocksize=0, align=1, stream=None):
        return self.lib.blosc_gpu_compress_packed(clevel, shuffle, typesize, cname, blocksize, self.n, (C.c_void_p * self.n)(*src_ptrs),
                                                  (C.c_size_t * self.n)(*src_sizes), dest, destsize, align, self.off, self.res, stream)

    def compress_params(self, src_ptrs, src_sizes, params, dest, destsize, align=1, stream=None):
        """chunk i with params[i] (include/blosc_gpu_params.h; params: see params_table) into one container in the caller's order"""
        assert len(params) == self.n
        return self.lib.blosc_gpu_compress_packed_params(self.n, params_table(params), (C.c_void_p * self.n)(*src_ptrs),
                                                         (C.c_size_t * self.n)(*src_sizes), dest, destsize, align, self.off, self.res, stream)

    def decompress(self, container, containersize, offsets, dest, destsize, stream=None):
        return self.lib.blosc_gpu_decompress_packed(self.n, container, containersize, (C.c_size_t * (self.n + 1))(*offsets), dest, destsize,
                                                    self.off, self.res, stream)

    def sizes(self, src_ptrs, stream=None):
        """blosc_cbuffer_sizes of n device-resident chunks: three lists (nbytes, cbytes, blocksize)."""
        out = [(C.c_size_t * self.n)() for _ in range(3)]
        if self.lib.blosc_gpu_cbuffer_sizes_batch(self.n, (C.c_void_p * self.n)(*src_ptrs), out[0], out[1], out[2], stream) != 0:
            raise RuntimeError("blosc_gpu_cbuffer_sizes_batch failed")
        return [list(o) for o in out]

    def offsets(self):
        return list(self.off)

    def results(self):
        return list(self.res)


class ItemRanges:
    """Helper for include/blosc_gpu_getitem.h: many item ranges of many chunks in one call; keeps the ctypes tables alive.

    ranges: (chunk, start, nitems) triples.  batch(): chunk i at src_ptrs[i], range r to dst_ptrs[r].  packed(): the chunks in a container
    with its offset table [n + 1], the slices back to back in one dest (dest 0 / None: the size query); offsets() is then the table
    [nranges + 1].  results() gives blosc_getitem's return value per range.
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, ranges, lib=None):
        self.n = len(ranges)
        self.lib = lib if lib is not None else load()
        self.chunk = (C.c_int * self.n)(*[r[0] for r in ranges])
        self.start = (C.c_int * self.n)(*[r[1] for r in ranges])
        self.nitems = (C.c_int * self.n)(*[r[2] for r in ranges])
        self.off = (C.c_size_t * (self.n + 1))()
        self.res = (C.c_int * self.n)()

    def batch(self, src_ptrs, dst_ptrs, stream=None):
        nchunks = len(src_ptrs)
        return self.lib.blosc_gpu_getitem_batch(nchunks, (C.c_void_p * nchunks)(*src_ptrs), self.n, self.chunk, self.start, self.nitems,
                                                (C.c_void_p * self.n)(*dst_ptrs), self.res, stream)

    def packed(self, container, containersize, offsets, dest, destsize, stream=None):
        nchunks = len(offsets) - 1
        return self.lib.blosc_gpu_getitem_packed(nchunks, container, containersize, (C.c_size_t * (nchunks + 1))(*offsets), self.n, self.chunk,
                                                 self.start, self.nitems, dest, destsize, self.off, self.res, stream)

    def offsets(self):
        return list(self.off)

    def results(self):
        return list(self.res)


def checksums(kind, ptrs, sizes, lib=None, stream=None):
    """zlib's adler32 (kind 1) / crc32 (kind 2) of the sizes[i] bytes at the device pointers ptrs[i], one call (include/blosc_gpu_checksum.h);
    returns the digests as a list of ints.  The library handle may be given (an emulator build in the CPU tests); default: the product."""
    L = lib if lib is not None else load()
    n = len(ptrs)
    out = (C.c_uint * max(n, 1))()
    r = L.blosc_gpu_checksum_batch(kind, n, (C.c_void_p * max(n, 1))(*ptrs), (C.c_size_t * max(n, 1))(*sizes), out, stream)
    if r != 0:
        raise RuntimeError(f"blosc_gpu_checksum_batch answered {r}")
    return list(out)[:n]


def checksums_packed(kind, container, containersize, offsets, lengths=None, lib=None, stream=None):
    """The same for the runs of one device buffer: run i = the first lengths[i] bytes at container + offsets[i] (lengths None: the whole span
    up to offsets[i + 1]); offsets has one entry more than there are runs."""
    L = lib if lib is not None else load()
    n = len(offsets) - 1
    out = (C.c_uint * max(n, 1))()
    ln = (C.c_size_t * max(n, 1))(*lengths) if lengths is not None else None
    r = L.blosc_gpu_checksum_packed(kind, n, container, containersize, (C.c_size_t * (n + 1))(*offsets), ln, out, stream)
    if r != 0:
        raise RuntimeError(f"blosc_gpu_checksum_packed answered {r}")
    return list(out)[:n]


def profile_get(name):
    ms, cnt = C.c_double(0), C.c_int(0)
    load().blosc_gpu_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value
