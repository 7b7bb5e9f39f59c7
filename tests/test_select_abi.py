"""CPU: include/blosc_gpu_select.h against the Python loader and the built library - the declared names, the exported symbols, and the
whole-call answers that need no device (nchunks == 0, NULL tables, a candidate table that does not start at 0 or decreases, an unusable
align): a negative value, every output untouched."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_compress_packed_select"), "the library has no compress calls with candidates per chunk"
    return pkgmod.declare_select(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_select.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.SELECT_SYMBOLS) and len(set(declared)) == len(declared), declared
    others = pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
    assert not set(pkgmod.SELECT_SYMBOLS) & set(others)
    for s in pkgmod.SELECT_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_select.h"\n'
                   'int (*batch)(int, const int*, const blosc_gpu_cparams*, const void* const*, const size_t*, void* const*, const size_t*, int*, int*, int*, void*)'
                   ' = blosc_gpu_compress_batch_select;\n'
                   'int (*packed)(int, const int*, const blosc_gpu_cparams*, const void* const*, const size_t*, void*, size_t, size_t, size_t*, int*, int*, int*, void*)'
                   ' = blosc_gpu_compress_packed_select;\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    rows = pkgmod.params_table([pkgmod.cparams(8), pkgmod.cparams(8, shuffle=2)])
    src, dst, n2 = (vp * 2)(0, 0), (vp * 2)(0, 0), (sz * 2)(0, 0)
    res, choice, cand, off = (i * 2)(-7, -7), (i * 2)(-8, -8), (i * 2)(-9, -9), (sz * 3)(5, 5, 5)
    good, from_one, falls, beyond = (i * 3)(0, 1, 2), (i * 3)(1, 1, 2), (i * 3)(0, 2, 1), (i * 3)(0, 3, 2)
    batch, packed = L.blosc_gpu_compress_batch_select, L.blosc_gpu_compress_packed_select
    # nchunks == 0: nothing to do, whatever the tables
    assert batch(0, None, None, None, None, None, None, None, None, None, None) == 0
    assert packed(0, None, None, None, None, None, 0, 1, off, None, None, None, None) == 0 and off[0] == 0
    off[0] = 5
    # NULL tables (the candidate answers may be NULL: not an error of its own, so it is not in this list)
    assert batch(2, None, rows, src, n2, dst, n2, res, choice, cand, None) < 0
    assert batch(2, good, None, src, n2, dst, n2, res, choice, cand, None) < 0
    assert batch(2, good, rows, None, n2, dst, n2, res, choice, cand, None) < 0
    assert batch(2, good, rows, src, None, dst, n2, res, choice, cand, None) < 0
    assert batch(2, good, rows, src, n2, None, n2, res, choice, cand, None) < 0
    assert batch(2, good, rows, src, n2, dst, None, res, choice, cand, None) < 0
    assert batch(2, good, rows, src, n2, dst, n2, None, choice, cand, None) < 0
    assert batch(2, good, rows, src, n2, dst, n2, res, None, cand, None) < 0
    assert packed(2, None, rows, src, n2, None, 0, 1, off, res, choice, cand, None) < 0
    assert packed(2, good, None, src, n2, None, 0, 1, off, res, choice, cand, None) < 0
    assert packed(2, good, rows, None, n2, None, 0, 1, off, res, choice, cand, None) < 0
    assert packed(2, good, rows, src, None, None, 0, 1, off, res, choice, cand, None) < 0
    assert packed(2, good, rows, src, n2, None, 0, 1, None, res, choice, cand, None) < 0
    assert packed(2, good, rows, src, n2, None, 0, 1, off, None, choice, cand, None) < 0
    assert packed(2, good, rows, src, n2, None, 0, 1, off, res, None, cand, None) < 0
    # a candidate table that does not start at 0, or decreases
    for first in (from_one, falls, beyond):
        assert batch(2, first, rows, src, n2, dst, n2, res, choice, cand, None) < 0
        assert packed(2, first, rows, src, n2, None, 0, 1, off, res, choice, cand, None) < 0
    # an unusable align, a negative count, a size for no buffer
    assert packed(2, good, rows, src, n2, None, 0, 3, off, res, choice, cand, None) < 0
    assert packed(2, good, rows, src, n2, None, 0, 8192, off, res, choice, cand, None) < 0
    assert packed(-1, good, rows, src, n2, None, 0, 1, off, res, choice, cand, None) < 0
    assert packed(2, good, rows, src, n2, None, 64, 1, off, res, choice, cand, None) < 0
    assert batch(-1, good, rows, src, n2, dst, n2, res, choice, cand, None) == 0
    assert list(res) == [-7, -7] and list(choice) == [-8, -8] and list(cand) == [-9, -9] and list(off) == [5, 5, 5]
