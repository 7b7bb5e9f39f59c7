"""CPU: include/blosc_gpu_where.h against the Python loader and the built library - the declared names, the exported symbols, the header as C,
and the whole-call answers that need no device (no chunks, every predicate outside the header's table, a row size outside 1 ... 65536, a
negative count, NULL tables, a capacity without a table, an offset table that decreases or ends behind the container): 0 or a negative
value; a refused call leaves every host output untouched, the call without chunks writes a total of 0 and no table entry."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_where_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_where_packed"), "the library has no where calls"
    return pkgmod.declare_where(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_where.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.WHERE_SYMBOLS) and len(set(declared)) == len(declared) == 2, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS + pkgmod.TAKE_SYMBOLS + pkgmod.PUT_SYMBOLS)
    assert not set(pkgmod.WHERE_SYMBOLS) & set(others)
    for s in pkgmod.WHERE_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_take.h"\n#include "blosc_gpu_where.h"\n'
                   'int (*batch)(int, const void* const*, size_t, const blosc_gpu_predicate*, int64_t*, size_t, size_t*, int*, int*, size_t*, void*)'
                   ' = blosc_gpu_where_batch;\n'
                   'int (*packed)(int, const void*, size_t, const size_t*, size_t, const blosc_gpu_predicate*, int64_t*, size_t, size_t*, int*, int*, size_t*,'
                   ' void*) = blosc_gpu_where_packed;\n'
                   'blosc_gpu_predicate p = {5, 4, BLOSC_GPU_FIELD_FLOAT, BLOSC_GPU_WHERE_GE, {0, 0, 192, 63}};\n'
                   'int sizes[sizeof(blosc_gpu_predicate) == 24 && BLOSC_GPU_WHERE_GE == 5 && BLOSC_GPU_FIELD_BFLOAT16 == 3 ? 1 : -1];\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_the_predicate_builder(pkgmod):
    p = pkgmod.predicate
    assert C.sizeof(pkgmod.Predicate) == 24
    assert bytes(p(pkgmod.FIELD_INT, 2, pkgmod.WHERE_LT, -2, offset=3).value[:2]) == b"\xfe\xff"
    assert bytes(p(pkgmod.FIELD_UINT, 8, 0, 2 ** 64 - 1).value) == b"\xff" * 8
    assert bytes(p(pkgmod.FIELD_FLOAT, 2, 0, 1.5).value[:2]) == b"\x00\x3e" and bytes(p(pkgmod.FIELD_FLOAT, 4, 0, -1.5).value[:4]) == b"\x00\x00\xc0\xbf"
    assert bytes(p(pkgmod.FIELD_FLOAT, 8, 0, float("inf")).value) == b"\x00" * 6 + b"\xf0\x7f"
    assert bytes(p(pkgmod.FIELD_BFLOAT16, 2, 0, 1.5).value[:2]) == b"\xc0\x3f" and bytes(p(pkgmod.FIELD_BFLOAT16, 2, 0, float("nan")).value[:2]) == b"\xc0\x7f"
    assert bytes(p(pkgmod.FIELD_BFLOAT16, 2, 0, 1.00390625).value[:2]) == b"\x80\x3f"      # a tie: to the even neighbour
    q = p(pkgmod.FIELD_UINT, 4, pkgmod.WHERE_GE, b"\x01\x02\x03\x04", offset=7)
    assert (q.offset, q.bytes, q.kind, q.op, bytes(q.value[:4])) == (7, 4, 0, 5, b"\x01\x02\x03\x04")
    with pytest.raises((ValueError, OverflowError)):
        p(pkgmod.FIELD_UINT, 1, 0, 256)


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    falls, beyond = (sz * 3)(0, 40, 32), (sz * 3)(0, 32, 65)
    rows, matches, total, unread = (i * 2)(-7, -7), (i * 2)(-8, -8), sz(77), sz(78)
    outs = (C.byref(total), matches, rows, C.byref(unread), None)
    idx, cont = vp(4096), vp(12288)      # addresses nobody reads: every call below is answered from its arguments
    good = pkgmod.predicate(pkgmod.FIELD_UINT, 4, pkgmod.WHERE_EQ, 1, offset=4)
    batch, packed = L.blosc_gpu_where_batch, L.blosc_gpu_where_packed

    def refused(pred, rb=8, n=2, s=src, c=cont, o=off, table=idx, cap=4, size=64):
        p = C.byref(pred) if pred is not None else None
        assert batch(n, s, rb, p, table, cap, *outs) < 0
        assert packed(n, c, size, o, rb, p, table, cap, *outs) < 0
        assert (list(rows), list(matches), total.value, unread.value) == ([-7, -7], [-8, -8], 77, 78)

    # no predicate; an op outside 0 ... 5; kind / bytes pairs that are not in the table; a field that ends behind the row
    refused(None)
    for op in (-1, 6):
        refused(pkgmod.Predicate(0, 4, pkgmod.FIELD_UINT, op))
    for kind, nbytes in ((pkgmod.FIELD_UINT, 0), (pkgmod.FIELD_UINT, 3), (pkgmod.FIELD_INT, 16), (pkgmod.FIELD_FLOAT, 1), (pkgmod.FIELD_FLOAT, 3),
                         (pkgmod.FIELD_BFLOAT16, 4), (pkgmod.FIELD_BFLOAT16, 1), (-1, 4), (4, 4)):
        refused(pkgmod.Predicate(0, nbytes, kind, pkgmod.WHERE_EQ))
    refused(pkgmod.Predicate(5, 4, pkgmod.FIELD_UINT, pkgmod.WHERE_EQ))
    refused(pkgmod.Predicate(2 ** 32 - 2, 4, pkgmod.FIELD_UINT, pkgmod.WHERE_EQ))
    # a row size outside 1 ... 65536, also without chunks
    for rb in (0, 65537):
        refused(pkgmod.predicate(pkgmod.FIELD_UINT, 1, 0, 0), rb=rb)
        refused(pkgmod.predicate(pkgmod.FIELD_UINT, 1, 0, 0), rb=rb, n=0, s=None, c=None, o=None, table=None, cap=0)
    # a negative count, NULL tables
    refused(good, n=-1)
    assert batch(2, None, 8, C.byref(good), idx, 4, *outs) < 0 and batch(2, None, 8, C.byref(good), None, 0, *outs) < 0
    assert packed(2, None, 64, off, 8, C.byref(good), idx, 4, *outs) < 0 and packed(2, cont, 64, None, 8, C.byref(good), idx, 4, *outs) < 0
    # a capacity without a table
    refused(good, table=None)
    # an offset table that decreases, or ends behind the container
    assert packed(2, cont, 64, falls, 8, C.byref(good), idx, 4, *outs) < 0 and packed(2, cont, 64, beyond, 8, C.byref(good), idx, 4, *outs) < 0
    assert packed(2, cont, 63, off, 8, C.byref(good), None, 0, *outs) < 0
    # a table inside the container
    assert packed(2, cont, 64, off, 8, C.byref(good), vp(12288 + 56), 1, *outs) < 0
    assert (list(rows), list(matches), total.value, unread.value) == ([-7, -7], [-8, -8], 77, 78)
    # no chunks: nothing to read - a total of 0, no unread row, no table entry written
    for call in (lambda: batch(0, None, 8, C.byref(good), None, 0, *outs), lambda: packed(0, None, 0, None, 8, C.byref(good), idx, 4, *outs)):
        total.value, unread.value = 77, 78
        assert call() == 0
        assert (list(rows), list(matches), total.value, unread.value) == ([-7, -7], [-8, -8], 0, 0)
    assert batch(0, None, 8, C.byref(good), None, 0, None, None, None, None, None) == 0
