"""CPU: include/blosc_gpu_take.h against the Python loader and the built library - the declared names, the exported symbols, and the
whole-call answers that need no device (no chunks and no indices, a row size outside 1 ... 65536, a negative count, NULL tables, an offset
table that decreases or ends behind the container): 0 or a negative value, every host output untouched."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_take_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_take_packed"), "the library has no take calls"
    return pkgmod.declare_take(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_take.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.TAKE_SYMBOLS) and len(set(declared)) == len(declared) == 2, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS)
    assert not set(pkgmod.TAKE_SYMBOLS) & set(others)
    for s in pkgmod.TAKE_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_take.h"\n'
                   'int (*batch)(int, const void* const*, size_t, size_t, const int64_t*, void*, int*, int*, size_t*, void*) = blosc_gpu_take_batch;\n'
                   'int (*packed)(int, const void*, size_t, const size_t*, size_t, size_t, const int64_t*, void*, int*, int*, size_t*, void*)'
                   ' = blosc_gpu_take_packed;\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    falls, beyond = (sz * 3)(0, 40, 32), (sz * 3)(0, 32, 65)
    rows, failed = (i * 2)(-7, -7), sz(77)
    fp = C.byref(failed)
    idx, dst, cont = vp(4096), vp(8192), vp(12288)      # addresses nobody reads: every call below is answered from its arguments
    batch, packed = L.blosc_gpu_take_batch, L.blosc_gpu_take_packed
    # no chunks and no indices: nothing to count, nothing to answer
    assert batch(0, None, 8, 0, None, None, None, rows, fp, None) == 0
    assert packed(0, None, 0, None, 8, 0, None, None, None, rows, fp, None) == 0
    # a row size outside 1 ... 65536
    for rb in (0, 65537):
        assert batch(2, src, rb, 1, idx, dst, None, rows, fp, None) < 0
        assert packed(2, cont, 64, off, rb, 1, idx, dst, None, rows, fp, None) < 0
        assert batch(0, None, rb, 0, None, None, None, rows, fp, None) < 0
    # a negative count, NULL tables
    assert batch(-1, src, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert packed(-1, cont, 64, off, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert batch(2, None, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert batch(2, None, 8, 0, None, None, None, rows, fp, None) < 0
    assert packed(2, None, 64, off, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert packed(2, cont, 64, None, 8, 1, idx, dst, None, rows, fp, None) < 0
    # indices without an index table or a destination
    assert batch(2, src, 8, 1, None, dst, None, rows, fp, None) < 0
    assert batch(2, src, 8, 1, idx, None, None, rows, fp, None) < 0
    assert packed(2, cont, 64, off, 8, 1, None, dst, None, rows, fp, None) < 0
    assert packed(2, cont, 64, off, 8, 1, idx, None, None, rows, fp, None) < 0
    # an offset table that decreases, or ends behind the container
    assert packed(2, cont, 64, falls, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert packed(2, cont, 64, beyond, 8, 1, idx, dst, None, rows, fp, None) < 0
    assert packed(2, cont, 63, off, 8, 0, None, None, None, rows, fp, None) < 0
    assert list(rows) == [-7, -7] and failed.value == 77
