"""CPU: include/blosc_gpu_aggregate.h against the Python loader and the built library - the declared names, the exported symbols, the header as
C, and the whole-call answers that need no device (no field, a field with pad_ set, outside the kind / bytes table or ending behind the row, a
filter that where refuses, a row size outside 1 ... 65536, a negative count, NULL tables, an offset table that decreases or ends behind the
container; no chunks): 0 or a negative value; a refused call leaves every host output untouched, the call without chunks writes the total of
nothing."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_aggregate_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_aggregate_packed"), "the library has no aggregate calls"
    return pkgmod.declare_aggregate(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_aggregate.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.AGGREGATE_SYMBOLS) and len(set(declared)) == len(declared) == 2, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS + pkgmod.TAKE_SYMBOLS + pkgmod.PUT_SYMBOLS + pkgmod.WHERE_SYMBOLS)
    assert not set(pkgmod.AGGREGATE_SYMBOLS) & set(others)
    for s in pkgmod.AGGREGATE_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_aggregate.h"\n'
                   'int (*batch)(int, const void* const*, size_t, const blosc_gpu_field*, const blosc_gpu_predicate*, blosc_gpu_aggregate*,'
                   ' blosc_gpu_aggregate*, int*, int*, size_t*, void*) = blosc_gpu_aggregate_batch;\n'
                   'int (*packed)(int, const void*, size_t, const size_t*, size_t, const blosc_gpu_field*, const blosc_gpu_predicate*, blosc_gpu_aggregate*,'
                   ' blosc_gpu_aggregate*, int*, int*, size_t*, void*) = blosc_gpu_aggregate_packed;\n'
                   'blosc_gpu_field f = {5, 4, BLOSC_GPU_FIELD_FLOAT, 0};\n'
                   'double total(const blosc_gpu_aggregate* a) { return a->min_row < 0 ? 0.0 : a->sum.f + (double)a->sum.i + (double)a->sum.u + a->min[0]; }\n'
                   'int sizes[sizeof(blosc_gpu_aggregate) == 64 && sizeof(blosc_gpu_field) == 16 ? 1 : -1];\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_the_field_builder_and_the_structs(pkgmod):
    assert C.sizeof(pkgmod.Field) == 16 and C.sizeof(pkgmod.Aggregate) == 64
    f = pkgmod.field(pkgmod.FIELD_BFLOAT16, 2, offset=7)
    assert (f.offset, f.bytes, f.kind, f.pad_) == (7, 2, 3, 0)
    f = pkgmod.field(pkgmod.FIELD_UINT, 8)
    assert (f.offset, f.bytes, f.kind, f.pad_) == (0, 8, 0, 0)
    a = pkgmod.Aggregate()
    a.sum.u = 2 ** 64 - 1
    assert a.sum.i == -1 and pkgmod.Aggregate.sum.offset == 56 and pkgmod.Aggregate.min.offset == 40 and pkgmod.Aggregate.max.offset == 48


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    falls, beyond = (sz * 3)(0, 40, 32), (sz * 3)(0, 32, 65)
    rows, status, unread = (i * 2)(-7, -7), (i * 2)(-8, -8), sz(78)
    total, per_chunk = pkgmod.Aggregate(), (pkgmod.Aggregate * 2)()
    cont = vp(12288)      # addresses nobody reads: every call below is answered from its arguments

    def fill():
        C.memset(C.byref(total), 0xA5, 64); C.memset(per_chunk, 0xA5, 128)
        unread.value = 78

    def untouched():
        return (bytes(total) == b"\xa5" * 64 and bytes(per_chunk) == b"\xa5" * 128 and (list(rows), list(status), unread.value) == ([-7, -7], [-8, -8], 78))

    fill()
    outs = (C.byref(total), per_chunk, status, rows, C.byref(unread), None)
    good = pkgmod.field(pkgmod.FIELD_UINT, 4, offset=4)
    batch, packed = L.blosc_gpu_aggregate_batch, L.blosc_gpu_aggregate_packed

    def refused(fld, flt=None, rb=8, n=2, s=src, c=cont, o=off, size=64):
        f = C.byref(fld) if fld is not None else None
        p = C.byref(flt) if flt is not None else None
        assert batch(n, s, rb, f, p, *outs) < 0
        assert packed(n, c, size, o, rb, f, p, *outs) < 0
        assert untouched()

    # no field; pad_ set; kind / bytes pairs that are not in the table; a field that ends behind the row
    refused(None)
    refused(pkgmod.Field(0, 4, pkgmod.FIELD_UINT, 1))
    refused(pkgmod.Field(0, 4, pkgmod.FIELD_UINT, -1))
    for kind, nbytes in ((pkgmod.FIELD_UINT, 0), (pkgmod.FIELD_UINT, 3), (pkgmod.FIELD_INT, 16), (pkgmod.FIELD_FLOAT, 1), (pkgmod.FIELD_FLOAT, 3),
                         (pkgmod.FIELD_BFLOAT16, 4), (pkgmod.FIELD_BFLOAT16, 1), (-1, 4), (4, 4)):
        refused(pkgmod.field(kind, nbytes))
    refused(pkgmod.field(pkgmod.FIELD_UINT, 4, offset=5))
    refused(pkgmod.field(pkgmod.FIELD_UINT, 4, offset=2 ** 32 - 2))
    # a filter that where refuses: an op outside 0 ... 5, a pair outside the table, a field that ends behind the row
    for op in (-1, 6):
        refused(good, pkgmod.Predicate(0, 4, pkgmod.FIELD_UINT, op))
    for kind, nbytes in ((pkgmod.FIELD_UINT, 3), (pkgmod.FIELD_FLOAT, 1), (pkgmod.FIELD_BFLOAT16, 4), (4, 4)):
        refused(good, pkgmod.Predicate(0, nbytes, kind, pkgmod.WHERE_EQ))
    refused(good, pkgmod.Predicate(7, 2, pkgmod.FIELD_INT, pkgmod.WHERE_EQ))
    # a row size outside 1 ... 65536, also without chunks
    for rb in (0, 65537):
        refused(pkgmod.field(pkgmod.FIELD_UINT, 1), rb=rb)
        refused(pkgmod.field(pkgmod.FIELD_UINT, 1), rb=rb, n=0, s=None, c=None, o=None)
    # a negative count, NULL tables
    refused(good, n=-1)
    assert batch(2, None, 8, C.byref(good), None, *outs) < 0
    assert packed(2, None, 64, off, 8, C.byref(good), None, *outs) < 0 and packed(2, cont, 64, None, 8, C.byref(good), None, *outs) < 0
    # an offset table that decreases, or ends behind the container
    assert packed(2, cont, 64, falls, 8, C.byref(good), None, *outs) < 0 and packed(2, cont, 64, beyond, 8, C.byref(good), None, *outs) < 0
    assert packed(2, cont, 63, off, 8, C.byref(good), None, *outs) < 0
    assert untouched()
    # no chunks: the total of nothing - all zero with both rows -1 - no unread row, nothing else written
    flt = pkgmod.predicate(pkgmod.FIELD_UINT, 2, pkgmod.WHERE_GT, 3, offset=1)
    for call in (lambda: batch(0, None, 8, C.byref(good), None, *outs), lambda: packed(0, None, 0, None, 8, C.byref(good), C.byref(flt), *outs)):
        fill()
        assert call() == 0
        assert (total.rows, total.count, total.nans, total.min_row, total.max_row, bytes(total.min), bytes(total.max), total.sum.u) == \
               (0, 0, 0, -1, -1, bytes(8), bytes(8), 0)
        assert bytes(per_chunk) == b"\xa5" * 128 and (list(rows), list(status), unread.value) == ([-7, -7], [-8, -8], 0)
    assert batch(0, None, 8, C.byref(good), None, None, None, None, None, None, None) == 0
    assert packed(0, None, 0, None, 8, C.byref(good), None, None, None, None, None, None, None) == 0
