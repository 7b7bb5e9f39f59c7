"""c-blosc_amd — Python-side loader for libblosc_amd.so (ctypes; test / bench plumbing only).

The product is the C-ABI shared library built from ``csrc/`` (see ``include/blosc.h`` and
``include/blosc_gpu.h``, ``include/blosc_gpu_packed.h``, ``include/blosc_gpu_params.h``, ``include/blosc_gpu_select.h``, ``include/blosc_gpu_getitem.h``, ``include/blosc_gpu_take.h``, ``include/blosc_gpu_put.h``, ``include/blosc_gpu_where.h``, ``include/blosc_gpu_aggregate.h``, ``include/blosc_gpu_clauses.h``, ``include/blosc_gpu_zones.h``, ``include/blosc_gpu_checksum.h``).  This module only locates it, declares argument types and offers small
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
SELECT_SYMBOLS = [      # include/blosc_gpu_select.h
    "blosc_gpu_compress_batch_select", "blosc_gpu_compress_packed_select",
]
TAKE_SYMBOLS = [        # include/blosc_gpu_take.h
    "blosc_gpu_take_batch", "blosc_gpu_take_packed",
]
PUT_SYMBOLS = [         # include/blosc_gpu_put.h
    "blosc_gpu_put_batch", "blosc_gpu_put_packed",
]
WHERE_SYMBOLS = [       # include/blosc_gpu_where.h
    "blosc_gpu_where_batch", "blosc_gpu_where_packed",
]
AGGREGATE_SYMBOLS = [   # include/blosc_gpu_aggregate.h
    "blosc_gpu_aggregate_batch", "blosc_gpu_aggregate_packed",
]
CLAUSES_SYMBOLS = [     # include/blosc_gpu_clauses.h
    "blosc_gpu_where_clauses_batch", "blosc_gpu_where_clauses_packed", "blosc_gpu_aggregate_clauses_batch", "blosc_gpu_aggregate_clauses_packed",
]
ZONES_SYMBOLS = [       # include/blosc_gpu_zones.h
    "blosc_gpu_aggregate_fields_batch", "blosc_gpu_aggregate_fields_packed", "blosc_gpu_zone_excludes", "blosc_gpu_where_zoned_batch",
    "blosc_gpu_where_zoned_packed", "blosc_gpu_aggregate_zoned_batch", "blosc_gpu_aggregate_zoned_packed",
]
MAX_TERMS = 16          # BLOSC_GPU_MAX_TERMS; clause numbers are 0 ... 15
MAX_ZONE_FIELDS = 16    # BLOSC_GPU_MAX_ZONE_FIELDS
WHERE_EQ, WHERE_NE, WHERE_LT, WHERE_LE, WHERE_GT, WHERE_GE = range(6)
FIELD_UINT, FIELD_INT, FIELD_FLOAT, FIELD_BFLOAT16 = range(4)
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


class Predicate(C.Structure):
    """blosc_gpu_predicate (include/blosc_gpu_where.h): field `op` value on `bytes` bytes at `offset` of every row"""
    _fields_ = [("offset", C.c_uint32), ("bytes", C.c_uint32), ("kind", C.c_int32), ("op", C.c_int32), ("value", C.c_uint8 * 8)]


def predicate(kind, nbytes, op, value, offset=0):
    """A Predicate.  value: a Python or numpy scalar, packed into the field's own little-endian representation - an integer of nbytes bytes
    (FIELD_UINT / FIELD_INT; it must fit), binary16 / 32 / 64 (FIELD_FLOAT), the upper half of the binary32 nearest to it (FIELD_BFLOAT16;
    a value that is no bfloat16 is rounded to nearest even, a NaN stays one) - or the `nbytes` bytes themselves as bytes."""
    import struct
    if isinstance(value, (bytes, bytearray)):
        raw = bytes(value)
    elif kind in (FIELD_UINT, FIELD_INT):
        raw = int(value).to_bytes(nbytes, "little", signed=(kind == FIELD_INT))
    elif kind == FIELD_FLOAT:
        raw = struct.pack({2: "<e", 4: "<f", 8: "<d"}[nbytes], float(value))
    elif kind == FIELD_BFLOAT16:
        bits = struct.unpack("<I", struct.pack("<f", float(value)))[0]
        if (bits & 0x7fffffff) > 0x7f800000: bits |= 0x00400000                  # a NaN keeps a mantissa bit in its upper half
        else: bits = (bits + 0x7fff + ((bits >> 16) & 1)) & 0xffffffff
        raw = struct.pack("<H", bits >> 16)
    else:
        raise ValueError(f"kind {kind}")
    if len(raw) != nbytes or nbytes > 8:
        raise ValueError(f"{len(raw)} bytes of value for a field of {nbytes}")
    return Predicate(offset, nbytes, kind, op, (C.c_uint8 * 8)(*raw))


class Term(C.Structure):
    """blosc_gpu_term (include/blosc_gpu_clauses.h): one test of a term list and the number of the clause it belongs to"""
    _fields_ = [("test", Predicate), ("clause", C.c_uint32), ("pad_", C.c_uint32)]


def term(pred, clause):
    """A Term: the Predicate `pred` (see predicate()) as a member of clause `clause`, 0 ... 15.  A row passes a list of terms when every
    clause that occurs in it has at least one true term"""
    if not 0 <= clause < MAX_TERMS:
        raise ValueError(f"clause {clause}: 0 ... {MAX_TERMS - 1}")
    return Term(pred, clause, 0)


def terms_table(terms):
    """(the host array of blosc_gpu_term a call takes, its length) from a list of Term; no terms: (None, 0)"""
    rows = list(terms or [])
    return ((Term * len(rows))(*rows) if rows else None), len(rows)


class Field(C.Structure):
    """blosc_gpu_field (include/blosc_gpu_aggregate.h): the `bytes` bytes at `offset` of every row, read as `kind`"""
    _fields_ = [("offset", C.c_uint32), ("bytes", C.c_uint32), ("kind", C.c_int32), ("pad_", C.c_int32)]


def field(kind, nbytes, offset=0):
    """A Field: FIELD_UINT / FIELD_INT of 1, 2, 4, 8 bytes, FIELD_FLOAT of 2, 4, 8, FIELD_BFLOAT16 of 2"""
    return Field(offset, nbytes, kind, 0)


class AggregateSum(C.Union):
    _fields_ = [("i", C.c_int64), ("u", C.c_uint64), ("f", C.c_double)]


class Aggregate(C.Structure):
    """blosc_gpu_aggregate (include/blosc_gpu_aggregate.h): rows read, rows counted, NaNs among them, the lowest rows holding the extremes (-1:
    none) with their bytes, and the sum - sum.u / sum.i / sum.f by the field's kind"""
    _fields_ = [("rows", C.c_uint64), ("count", C.c_uint64), ("nans", C.c_uint64), ("min_row", C.c_int64), ("max_row", C.c_int64),
                ("min", C.c_uint8 * 8), ("max", C.c_uint8 * 8), ("sum", AggregateSum)]


def params_table(params):
    """The host array of blosc_gpu_cparams a call takes, from a list of CParams (or of argument tuples / dicts of cparams())"""
    rows = [p if isinstance(p, CParams) else (cparams(**p) if isinstance(p, dict) else cparams(*p)) for p in params]
    return (CParams * max(len(rows), 1))(*rows)


def candidate_tables(cand_first, rows):
    """(cand_first as a C int array, the rows' table) of a call of include/blosc_gpu_select.h.  cand_first: [n + 1], chunk i has the
    candidates rows[cand_first[i]:cand_first[i + 1]]; rows: see params_table"""
    assert cand_first[-1] == len(rows)
    return (C.c_int * len(cand_first))(*cand_first), params_table(rows)

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
    _lib = declare(C.CDLL(LIB_PATH))
    return _lib


def _signatures():
    """name -> (argtypes, restype) of every exported function whose ctypes defaults (no argument check, an int back) do not fit."""
    vp, sz, i, s = C.c_void_p, C.c_size_t, C.c_int, C.c_char_p
    P = C.POINTER
    ip, zp, pp = P(i), P(sz), P(vp)
    batch = [pp, zp, pp, zp, ip]                        # src, their sizes, dest, their sizes, the results
    one = [i, i, sz, s, sz]                             # clevel, doshuffle, typesize, compressor, blocksize
    return {
        # include/blosc.h
        "blosc_compress": ([i, i, sz, sz, vp, vp, sz], i),
        "blosc_compress_ctx": ([i, i, sz, sz, vp, vp, sz, s, sz, i], i),
        "blosc_decompress": ([vp, vp, sz], i),
        "blosc_decompress_ctx": ([vp, vp, sz, i], i),
        "blosc_getitem": ([vp, i, i, vp], i),
        "blosc_set_compressor": ([s], i),
        "blosc_get_compressor": (None, s),
        "blosc_list_compressors": (None, s),
        "blosc_get_version_string": (None, s),
        "blosc_cbuffer_complib": ([vp], s),
        "blosc_compname_to_compcode": ([s], i),
        "blosc_compcode_to_compname": ([i, P(s)], i),
        "blosc_get_complib_info": ([s, P(s), P(s)], i),
        "blosc_cbuffer_sizes": ([vp, zp, zp, zp], None),
        "blosc_cbuffer_validate": ([vp, sz, zp], i),
        "blosc_cbuffer_metainfo": ([vp, zp, ip], None),
        "blosc_cbuffer_versions": ([vp, ip, ip], None),
        "blosc_set_blocksize": ([sz], None),
        "blosc_set_splitmode": ([i], None),
        # include/blosc_gpu.h
        "blosc_gpu_compress_batch": (one + [i] + batch + [vp], i),
        "blosc_gpu_decompress_batch": ([i] + batch + [vp], i),
        "blosc_gpu_compress_batch_host": (one + [i] + batch, i),
        "blosc_gpu_decompress_batch_host": ([i] + batch, i),
        "blosc_gpu_partition": ([sz, i, i, zp, zp], i),
        "blosc_gpu_compress_batch_multi": ([i, ip] + one + [i] + batch, i),
        "blosc_gpu_decompress_batch_multi": ([i, ip, i] + batch, i),
        "blosc_gpu_getitem": ([vp, i, i, vp, vp], i),
        "blosc_gpu_profile": ([i], None),
        "blosc_gpu_profile_reset": (None, None),
        "blosc_gpu_profile_get": ([s, P(C.c_double), ip], i),
        # include/blosc_gpu_packed.h
        "blosc_gpu_packed_bound": ([i, zp, sz], sz),
        "blosc_gpu_compress_packed": (one + [i, pp, zp, vp, sz, sz, zp, ip, vp], i),
        "blosc_gpu_decompress_packed": ([i, vp, sz, zp, vp, sz, zp, ip, vp], i),
        "blosc_gpu_cbuffer_sizes_batch": ([i, pp, zp, zp, zp, vp], i),
        # include/blosc_gpu_params.h
        "blosc_gpu_compress_batch_params": ([i, P(CParams)] + batch + [vp], i),
        "blosc_gpu_compress_packed_params": ([i, P(CParams), pp, zp, vp, sz, sz, zp, ip, vp], i),
        # include/blosc_gpu_select.h
        "blosc_gpu_compress_batch_select": ([i, ip, P(CParams)] + batch + [ip, ip, vp], i),
        "blosc_gpu_compress_packed_select": ([i, ip, P(CParams), pp, zp, vp, sz, sz, zp, ip, ip, ip, vp], i),
        # include/blosc_gpu_getitem.h
        "blosc_gpu_getitem_batch": ([i, pp, i, ip, ip, ip, pp, ip, vp], i),
        "blosc_gpu_getitem_packed": ([i, vp, sz, zp, i, ip, ip, ip, vp, sz, zp, ip, vp], i),
        # include/blosc_gpu_take.h
        "blosc_gpu_take_batch": ([i, pp, sz, sz, vp, vp, vp, ip, zp, vp], i),
        "blosc_gpu_take_packed": ([i, vp, sz, zp, sz, sz, vp, vp, vp, ip, zp, vp], i),
        # include/blosc_gpu_put.h
        "blosc_gpu_put_batch": ([i, pp, sz, sz, vp, vp, P(CParams), vp, sz, sz, zp, ip, ip, vp, ip, zp, vp], i),
        "blosc_gpu_put_packed": ([i, vp, sz, zp, sz, sz, vp, vp, P(CParams), vp, sz, sz, zp, ip, ip, vp, ip, zp, vp], i),
        # include/blosc_gpu_where.h
        "blosc_gpu_where_batch": ([i, pp, sz, P(Predicate), vp, sz, zp, ip, ip, zp, vp], i),
        "blosc_gpu_where_packed": ([i, vp, sz, zp, sz, P(Predicate), vp, sz, zp, ip, ip, zp, vp], i),
        # include/blosc_gpu_aggregate.h
        "blosc_gpu_aggregate_batch": ([i, pp, sz, P(Field), P(Predicate), P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        "blosc_gpu_aggregate_packed": ([i, vp, sz, zp, sz, P(Field), P(Predicate), P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        # include/blosc_gpu_clauses.h
        "blosc_gpu_where_clauses_batch": ([i, pp, sz, P(Term), i, vp, sz, zp, ip, ip, zp, vp], i),
        "blosc_gpu_where_clauses_packed": ([i, vp, sz, zp, sz, P(Term), i, vp, sz, zp, ip, ip, zp, vp], i),
        "blosc_gpu_aggregate_clauses_batch": ([i, pp, sz, P(Field), P(Term), i, P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        "blosc_gpu_aggregate_clauses_packed": ([i, vp, sz, zp, sz, P(Field), P(Term), i, P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        # include/blosc_gpu_zones.h
        "blosc_gpu_aggregate_fields_batch": ([i, pp, sz, P(Field), i, P(Term), i, P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        "blosc_gpu_aggregate_fields_packed": ([i, vp, sz, zp, sz, P(Field), i, P(Term), i, P(Aggregate), P(Aggregate), ip, ip, zp, vp], i),
        "blosc_gpu_zone_excludes": ([P(Term), i, P(Field), i, P(Aggregate), C.c_uint64], i),
        "blosc_gpu_where_zoned_batch": ([i, pp, sz, P(Term), i, P(Field), i, P(Aggregate), vp, sz, zp, ip, ip, zp, P(C.c_uint8), vp], i),
        "blosc_gpu_where_zoned_packed": ([i, vp, sz, zp, sz, P(Term), i, P(Field), i, P(Aggregate), vp, sz, zp, ip, ip, zp, P(C.c_uint8), vp], i),
        "blosc_gpu_aggregate_zoned_batch": ([i, pp, sz, P(Field), P(Term), i, P(Field), i, P(Aggregate), P(Aggregate), P(Aggregate), ip, ip, zp, P(C.c_uint8), vp], i),
        "blosc_gpu_aggregate_zoned_packed": ([i, vp, sz, zp, sz, P(Field), P(Term), i, P(Field), i, P(Aggregate), P(Aggregate), P(Aggregate), ip, ip, zp,
                                              P(C.c_uint8), vp], i),
        # include/blosc_gpu_checksum.h
        "blosc_gpu_checksum_batch": ([i, i, pp, zp, P(C.c_uint), vp], i),
        "blosc_gpu_checksum_packed": ([i, i, vp, sz, zp, zp, P(C.c_uint), vp], i),
        # test hooks
        "blosc_internal_shuffle": ([sz, sz, vp, vp], None),
        "blosc_internal_unshuffle": ([sz, sz, vp, vp], None),
        "blosc_internal_bitshuffle": ([sz, sz, vp, vp, vp], i),
        "blosc_internal_bitunshuffle": ([sz, sz, vp, vp, vp], i),
        "blosc_amd_policy_blocksize": ([i, i, i, i, i, i], i),
        "blosc_amd_policy_split": ([i, i, i, i], i),
        "blosc_amd_getitem_pass_bytes": ([sz], None),
        "blosc_amd_checksum_tile_bytes": ([sz], None),
    }


SIGNATURES = _signatures()


def declare(L):
    """SIGNATURES on a library handle, for every symbol the handle has: the product in load(), the emulator build of the CPU tests, and
    the builds of earlier rounds that A/B scripts load through this module, which lack the newer calls.  Returns the handle."""
    for name, (argtypes, restype) in SIGNATURES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            if argtypes is not None:
                f.argtypes = argtypes
            f.restype = restype
    return L


declare_packed = declare_params = declare_select = declare_getitem = declare_take = declare_put = declare_where = declare_aggregate = declare_clauses = declare_zones = declare_checksum = declare    # the names from when every header had a function of its own


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

    def compress_select(self, cand_first, rows, stream=None, lib=None):
        """chunk i with the best of rows[cand_first[i]:cand_first[i + 1]] (include/blosc_gpu_select.h), the whole batch in one call;
        results() are the winners' sizes, choices() their indices inside their ranges, candidate_results() every candidate's size"""
        assert len(cand_first) == self.n + 1
        first, table = candidate_tables(cand_first, rows)
        self.choice = (C.c_int * max(self.n, 1))()
        self.cand = (C.c_int * max(len(rows), 1))()
        self.ncand = len(rows)
        return (lib if lib is not None else load()).blosc_gpu_compress_batch_select(self.n, first, table, self.src, self.ssz, self.dst, self.dsz, self.res,
                                                                                    self.choice, self.cand, stream)

    def choices(self):
        return list(self.choice)[:self.n]

    def candidate_results(self):
        return list(self.cand)[:self.ncand]

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

    def compress_select(self, src_ptrs, src_sizes, cand_first, rows, dest, destsize, align=1, stream=None):
        """chunk i with the best of rows[cand_first[i]:cand_first[i + 1]] (include/blosc_gpu_select.h) into one container in the
        caller's order; choices() are the winners' indices inside their ranges, candidate_results() every candidate's size"""
        assert len(cand_first) == self.n + 1
        first, table = candidate_tables(cand_first, rows)
        self.choice = (C.c_int * max(self.n, 1))()
        self.cand = (C.c_int * max(len(rows), 1))()
        self.ncand = len(rows)
        return self.lib.blosc_gpu_compress_packed_select(self.n, first, table, (C.c_void_p * self.n)(*src_ptrs), (C.c_size_t * self.n)(*src_sizes),
                                                         dest, destsize, align, self.off, self.res, self.choice, self.cand, stream)

    def choices(self):
        return list(self.choice)[:self.n]

    def candidate_results(self):
        return list(self.cand)[:self.ncand]

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


class RowTake:
    """Helper for include/blosc_gpu_take.h: rows of row_bytes bytes of many chunks by an index table on the device.

    batch(): chunk i at src_ptrs[i].  packed(): the chunks in a container with its offset table [n + 1].  Both take the device addresses
    of the int64 indices, of dest (nidx * row_bytes bytes) and of the int32 status table (0 / None: no status wanted) and return the
    call's answer.  chunk_rows() gives every chunk's row count (or its negative census code), failed() the rows with a negative status.
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, row_bytes, lib=None):
        self.row_bytes = row_bytes
        self.lib = lib if lib is not None else load()
        self.rows = (C.c_int * 1)()
        self.nchunks = 0
        self.nfailed = C.c_size_t(0)

    def _outputs(self, nchunks):
        self.nchunks = nchunks
        self.rows = (C.c_int * max(nchunks, 1))()
        self.nfailed = C.c_size_t(0)

    def batch(self, src_ptrs, index, nidx, dest, status=None, stream=None):
        self._outputs(len(src_ptrs))
        return self.lib.blosc_gpu_take_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, nidx, index, dest, status,
                                             self.rows, C.byref(self.nfailed), stream)

    def packed(self, container, containersize, offsets, index, nidx, dest, status=None, stream=None):
        self._outputs(len(offsets) - 1)
        return self.lib.blosc_gpu_take_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes, nidx,
                                              index, dest, status, self.rows, C.byref(self.nfailed), stream)

    def chunk_rows(self):
        return list(self.rows)[:self.nchunks]

    def failed(self):
        return int(self.nfailed.value)


class RowPut:
    """Helper for include/blosc_gpu_put.h: rows of row_bytes bytes written into many chunks by an index table on the device; the result is a
    new packed container in `dest`.

    batch(): chunk i at src_ptrs[i].  packed(): the chunks in a container with its offset table [n + 1].  Both take the device addresses of
    the int64 indices, of the rows (nidx * row_bytes bytes), of dest and of the int32 status table (0 / None: no status wanted), and the
    parameters of every chunk (see params_table); they return the call's answer.  offsets() is the new offset table [n + 1], results() the
    per-chunk cbytes, rewritten() 1 / 0 / -1 per chunk, chunk_rows() every chunk's row count (or its negative census code), failed() the
    indices with a negative status.
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, row_bytes, lib=None):
        self.row_bytes = row_bytes
        self.lib = lib if lib is not None else load()
        self._outputs(0)

    def _outputs(self, nchunks):
        self.nchunks = nchunks
        self.off = (C.c_size_t * (nchunks + 1))()
        self.res = (C.c_int * max(nchunks, 1))()
        self.rew = (C.c_int * max(nchunks, 1))()
        self.rows = (C.c_int * max(nchunks, 1))()
        self.nfailed = C.c_size_t(0)

    def batch(self, src_ptrs, index, nidx, rows, params, dest, destsize, align=1, status=None, stream=None):
        self._outputs(len(src_ptrs))
        return self.lib.blosc_gpu_put_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, nidx, index, rows,
                                            params_table(params), dest, destsize, align, self.off, self.res, self.rew, status, self.rows,
                                            C.byref(self.nfailed), stream)

    def packed(self, container, containersize, offsets, index, nidx, rows, params, dest, destsize, align=1, status=None, stream=None):
        self._outputs(len(offsets) - 1)
        return self.lib.blosc_gpu_put_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                             nidx, index, rows, params_table(params), dest, destsize, align, self.off, self.res, self.rew, status,
                                             self.rows, C.byref(self.nfailed), stream)

    def offsets(self):
        return list(self.off)

    def results(self):
        return list(self.res)[:self.nchunks]

    def rewritten(self):
        return list(self.rew)[:self.nchunks]

    def chunk_rows(self):
        return list(self.rows)[:self.nchunks]

    def failed(self):
        return int(self.nfailed.value)


class RowWhere:
    """Helper for include/blosc_gpu_where.h: the rows of row_bytes bytes of many chunks whose field satisfies a Predicate (see predicate()),
    as an int64 index table on the device.

    batch(): chunk i at src_ptrs[i].  packed(): the chunks in a container with its offset table [n + 1].  Both take the predicate, the device
    address of the int64 table (0 / None with capacity 0: the count alone) and its capacity in entries, and return the call's answer.
    total() is the number of matches whatever the capacity, chunk_matches() every chunk's matches (or the negative answer of the decoder),
    chunk_rows() every chunk's row count (or its negative census code), unread() the rows of the chunks that did not decode.
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, row_bytes, lib=None):
        self.row_bytes = row_bytes
        self.lib = lib if lib is not None else load()
        self._outputs(0)

    def _outputs(self, nchunks):
        self.nchunks = nchunks
        self.matches = (C.c_int * max(nchunks, 1))()
        self.rows = (C.c_int * max(nchunks, 1))()
        self.ntotal = C.c_size_t(0)
        self.nunread = C.c_size_t(0)

    def batch(self, src_ptrs, pred, index_out, capacity, stream=None):
        self._outputs(len(src_ptrs))
        return self.lib.blosc_gpu_where_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, C.byref(pred), index_out,
                                              capacity, C.byref(self.ntotal), self.matches, self.rows, C.byref(self.nunread), stream)

    def packed(self, container, containersize, offsets, pred, index_out, capacity, stream=None):
        self._outputs(len(offsets) - 1)
        return self.lib.blosc_gpu_where_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                               C.byref(pred), index_out, capacity, C.byref(self.ntotal), self.matches, self.rows,
                                               C.byref(self.nunread), stream)

    def total(self):
        return int(self.ntotal.value)

    def chunk_matches(self):
        return list(self.matches)[:self.nchunks]

    def chunk_rows(self):
        return list(self.rows)[:self.nchunks]

    def unread(self):
        return int(self.nunread.value)


class RowAggregate:
    """Helper for include/blosc_gpu_aggregate.h: count, sum, min and max of a Field (see field()) of the rows of row_bytes bytes of many chunks,
    of the rows a Predicate lets through (filter None: of every row).

    batch(): chunk i at src_ptrs[i].  packed(): the chunks in a container with its offset table [n + 1].  Both return the call's answer.
    total() is the call's Aggregate, chunks() every chunk's, chunk_status() 0 or the negative answer of the decoder per chunk, chunk_rows()
    every chunk's row count (or its negative census code), unread() the rows of the chunks that did not decode.
    The library handle may be given (an emulator build in the CPU tests); default: the product."""

    def __init__(self, row_bytes, lib=None):
        self.row_bytes = row_bytes
        self.lib = lib if lib is not None else load()
        self._outputs(0)

    def _outputs(self, nchunks):
        self.nchunks = nchunks
        self.result = Aggregate()
        self.per_chunk = (Aggregate * max(nchunks, 1))()
        self.status = (C.c_int * max(nchunks, 1))()
        self.rows = (C.c_int * max(nchunks, 1))()
        self.nunread = C.c_size_t(0)

    def batch(self, src_ptrs, fld, filter=None, stream=None):
        self._outputs(len(src_ptrs))
        return self.lib.blosc_gpu_aggregate_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, C.byref(fld),
                                                  C.byref(filter) if filter is not None else None, C.byref(self.result), self.per_chunk, self.status,
                                                  self.rows, C.byref(self.nunread), stream)

    def packed(self, container, containersize, offsets, fld, filter=None, stream=None):
        self._outputs(len(offsets) - 1)
        return self.lib.blosc_gpu_aggregate_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                   C.byref(fld), C.byref(filter) if filter is not None else None, C.byref(self.result), self.per_chunk,
                                                   self.status, self.rows, C.byref(self.nunread), stream)

    def total(self):
        return self.result

    def chunks(self):
        return list(self.per_chunk)[:self.nchunks]

    def chunk_status(self):
        return list(self.status)[:self.nchunks]

    def chunk_rows(self):
        return list(self.rows)[:self.nchunks]

    def unread(self):
        return int(self.nunread.value)


class RowWhereClauses(RowWhere):
    """RowWhere for include/blosc_gpu_clauses.h: batch() and packed() take a list of Term (see term()) in the predicate's place - the rows for
    which every clause of the list has a true term - through blosc_gpu_where_clauses_*.  The outputs are RowWhere's."""

    def batch(self, src_ptrs, terms, index_out, capacity, stream=None):
        self._outputs(len(src_ptrs))
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_where_clauses_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, table, n, index_out,
                                                      capacity, C.byref(self.ntotal), self.matches, self.rows, C.byref(self.nunread), stream)

    def packed(self, container, containersize, offsets, terms, index_out, capacity, stream=None):
        self._outputs(len(offsets) - 1)
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_where_clauses_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                       table, n, index_out, capacity, C.byref(self.ntotal), self.matches, self.rows,
                                                       C.byref(self.nunread), stream)


class RowAggregateClauses(RowAggregate):
    """RowAggregate for include/blosc_gpu_clauses.h: batch() and packed() take a list of Term (see term()) in the filter's place (None or
    empty: every row) through blosc_gpu_aggregate_clauses_*.  The outputs are RowAggregate's."""

    def batch(self, src_ptrs, fld, terms=None, stream=None):
        self._outputs(len(src_ptrs))
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_aggregate_clauses_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, C.byref(fld), table, n,
                                                          C.byref(self.result), self.per_chunk, self.status, self.rows, C.byref(self.nunread), stream)

    def packed(self, container, containersize, offsets, fld, terms=None, stream=None):
        self._outputs(len(offsets) - 1)
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_aggregate_clauses_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                           C.byref(fld), table, n, C.byref(self.result), self.per_chunk, self.status, self.rows,
                                                           C.byref(self.nunread), stream)


def fields_table(fields):
    """(the host array of blosc_gpu_field a call takes, its length) from a list of Field; no fields: (None, 0)"""
    rows = list(fields or [])
    return ((Field * len(rows))(*rows) if rows else None), len(rows)


class RowAggregateFields:
    """Helper for blosc_gpu_aggregate_fields_* (include/blosc_gpu_zones.h): the aggregates of up to 16 Field of the rows a list of Term lets
    through (None or empty: every row), in ONE decode.  batch() and packed() return the call's answer.  totals() is one Aggregate per field,
    chunks() every chunk's list of them, entries() the ctypes array [nchunks * nfields], chunk-major - with no terms, the zone map the zoned
    calls read; chunk_status(), chunk_rows() and unread() are RowAggregate's."""

    def __init__(self, row_bytes, lib=None):
        self.row_bytes = row_bytes
        self.lib = lib if lib is not None else load()
        self._outputs(0, 1)

    def _outputs(self, nchunks, nfields):
        self.nchunks, self.nfields = nchunks, nfields
        self.result = (Aggregate * max(nfields, 1))()
        self.per_chunk = (Aggregate * max(nchunks * nfields, 1))()
        self.status = (C.c_int * max(nchunks, 1))()
        self.rows = (C.c_int * max(nchunks, 1))()
        self.nunread = C.c_size_t(0)

    def batch(self, src_ptrs, fields, terms=None, stream=None):
        ftab, nf = fields_table(fields)
        self._outputs(len(src_ptrs), nf)
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_aggregate_fields_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, ftab, nf, table, n,
                                                         self.result, self.per_chunk, self.status, self.rows, C.byref(self.nunread), stream)

    def packed(self, container, containersize, offsets, fields, terms=None, stream=None):
        ftab, nf = fields_table(fields)
        self._outputs(len(offsets) - 1, nf)
        table, n = terms_table(terms)
        return self.lib.blosc_gpu_aggregate_fields_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                          ftab, nf, table, n, self.result, self.per_chunk, self.status, self.rows, C.byref(self.nunread),
                                                          stream)

    def totals(self):
        return list(self.result)[:self.nfields]

    def entries(self):
        return self.per_chunk

    def chunks(self):
        return [list(self.per_chunk)[k * self.nfields:(k + 1) * self.nfields] for k in range(self.nchunks)]

    def chunk_status(self):
        return list(self.status)[:self.nchunks]

    def chunk_rows(self):
        return list(self.rows)[:self.nchunks]

    def unread(self):
        return int(self.nunread.value)


def zone_excludes(terms, zfields, entries, chunk_rows, lib=None):
    """blosc_gpu_zone_excludes (include/blosc_gpu_zones.h): 1 if no row of a chunk of chunk_rows rows, whose fields `zfields` the Aggregate
    `entries` describe, can pass the list of Term; 0 if one may; negative for arguments the rule refuses.  Host only"""
    L = lib if lib is not None else load()
    table, n = terms_table(terms)
    ftab, nf = fields_table(zfields)
    etab = (Aggregate * nf)(*entries) if nf else None
    return L.blosc_gpu_zone_excludes(table, n, ftab, nf, etab, chunk_rows)


class RowWhereZoned(RowWhere):
    """RowWhereClauses through blosc_gpu_where_zoned_* (include/blosc_gpu_zones.h): batch() and packed() take, behind the list of Term, the
    zone fields (a list of Field) and the map - a ctypes array of Aggregate [nchunks * len(zfields)], chunk-major, RowAggregateFields.entries()
    of a call without terms.  pruned() is 1 for every chunk that was not decoded.  The other outputs are RowWhere's."""

    def _zoned(self, nchunks):
        self._outputs(nchunks)
        self.skipped = (C.c_uint8 * max(nchunks, 1))()

    def batch(self, src_ptrs, terms, zfields, zones, index_out, capacity, stream=None):
        self._zoned(len(src_ptrs))
        table, n = terms_table(terms)
        ftab, nf = fields_table(zfields)
        return self.lib.blosc_gpu_where_zoned_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, table, n, ftab, nf, zones,
                                                    index_out, capacity, C.byref(self.ntotal), self.matches, self.rows, C.byref(self.nunread), self.skipped,
                                                    stream)

    def packed(self, container, containersize, offsets, terms, zfields, zones, index_out, capacity, stream=None):
        self._zoned(len(offsets) - 1)
        table, n = terms_table(terms)
        ftab, nf = fields_table(zfields)
        return self.lib.blosc_gpu_where_zoned_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                     table, n, ftab, nf, zones, index_out, capacity, C.byref(self.ntotal), self.matches, self.rows,
                                                     C.byref(self.nunread), self.skipped, stream)

    def pruned(self):
        return list(self.skipped)[:self.nchunks]


class RowAggregateZoned(RowAggregate):
    """RowAggregateClauses through blosc_gpu_aggregate_zoned_* (include/blosc_gpu_zones.h): zfields, zones and pruned() as in RowWhereZoned."""

    def _zoned(self, nchunks):
        self._outputs(nchunks)
        self.skipped = (C.c_uint8 * max(nchunks, 1))()

    def batch(self, src_ptrs, fld, terms, zfields, zones, stream=None):
        self._zoned(len(src_ptrs))
        table, n = terms_table(terms)
        ftab, nf = fields_table(zfields)
        return self.lib.blosc_gpu_aggregate_zoned_batch(self.nchunks, (C.c_void_p * max(self.nchunks, 1))(*src_ptrs), self.row_bytes, C.byref(fld), table, n,
                                                        ftab, nf, zones, C.byref(self.result), self.per_chunk, self.status, self.rows, C.byref(self.nunread),
                                                        self.skipped, stream)

    def packed(self, container, containersize, offsets, fld, terms, zfields, zones, stream=None):
        self._zoned(len(offsets) - 1)
        table, n = terms_table(terms)
        ftab, nf = fields_table(zfields)
        return self.lib.blosc_gpu_aggregate_zoned_packed(self.nchunks, container, containersize, (C.c_size_t * (self.nchunks + 1))(*offsets), self.row_bytes,
                                                         C.byref(fld), table, n, ftab, nf, zones, C.byref(self.result), self.per_chunk, self.status, self.rows,
                                                         C.byref(self.nunread), self.skipped, stream)

    def pruned(self):
        return list(self.skipped)[:self.nchunks]


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
