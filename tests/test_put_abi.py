"""CPU: include/blosc_gpu_put.h against the Python loader and the built library - the declared names, the exported symbols, the header as C,
and the whole-call answers that need no device (no chunks and no indices, a row size outside 1 ... 65536, a negative count, NULL tables, more
than UINT32_MAX - 1 indices, an unusable `align`, a NULL dest that claims bytes, an offset table that decreases or ends behind the container, a
dest inside the container): 0 or a negative value, every host output untouched."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_put_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_put_packed"), "the library has no put calls"
    return pkgmod.declare_put(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_put.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.PUT_SYMBOLS) and len(set(declared)) == len(declared) == 2, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS + pkgmod.TAKE_SYMBOLS)
    assert not set(pkgmod.PUT_SYMBOLS) & set(others)
    for s in pkgmod.PUT_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s
    batch, packed = pkgmod.SIGNATURES["blosc_gpu_put_batch"][0], pkgmod.SIGNATURES["blosc_gpu_put_packed"][0]
    assert len(batch) == 17 and len(packed) == 19 and batch[2:] == packed[4:]      # "the same from row_bytes on"


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    tail = ("size_t, size_t, const int64_t*, const void*, const blosc_gpu_cparams*, void*, size_t, size_t, size_t*, int*, int*, int*, int*, size_t*, void*)")
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_put.h"\n'
                   'int (*batch)(int, const void* const*, ' + tail + ' = blosc_gpu_put_batch;\n'
                   'int (*packed)(int, const void*, size_t, const size_t*, ' + tail + ' = blosc_gpu_put_packed;\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    falls, beyond = (sz * 3)(0, 40, 32), (sz * 3)(0, 32, 65)
    par = pkgmod.params_table([pkgmod.cparams(4), pkgmod.cparams(4)])
    out_off, cb, rew, rows, failed = (sz * 3)(7, 7, 7), (i * 2)(-7, -7), (i * 2)(-7, -7), (i * 2)(-7, -7), sz(77)
    fp = C.byref(failed)
    idx, new, cont, dst = vp(4096), vp(8192), vp(12288), vp(1 << 20)      # addresses nobody reads: every call below is answered from its arguments
    batch, packed = L.blosc_gpu_put_batch, L.blosc_gpu_put_packed
    tail = (par, dst, 4096, 16, out_off, cb, rew, None, rows, fp, None)

    def b(nchunks, s, rb, nidx, ix, rw, t=tail): return batch(nchunks, s, rb, nidx, ix, rw, *t)

    def p(nchunks, c, size, o, rb, nidx, ix, rw, t=tail): return packed(nchunks, c, size, o, rb, nidx, ix, rw, *t)

    def untouched(): return list(out_off) == [7, 7, 7] and list(cb) == list(rew) == list(rows) == [-7, -7] and failed.value == 77

    # a row size outside 1 ... 65536
    for rb in (0, 65537):
        assert b(2, src, rb, 1, idx, new) < 0 and p(2, cont, 64, off, rb, 1, idx, new) < 0 and b(0, None, rb, 0, None, None) < 0
    # a negative count, NULL tables
    assert b(-1, src, 8, 1, idx, new) < 0 and p(-1, cont, 64, off, 8, 1, idx, new) < 0
    assert b(2, None, 8, 1, idx, new) < 0 and b(2, None, 8, 0, None, None) < 0
    assert p(2, None, 64, off, 8, 1, idx, new) < 0 and p(2, cont, 64, None, 8, 1, idx, new) < 0
    # indices without an index table or rows; more indices than an owner word can tell apart
    assert b(2, src, 8, 1, None, new) < 0 and b(2, src, 8, 1, idx, None) < 0
    assert p(2, cont, 64, off, 8, 1, None, new) < 0 and p(2, cont, 64, off, 8, 1, idx, None) < 0
    assert b(2, src, 8, 2 ** 32 - 1, idx, new) < 0 and p(2, cont, 64, off, 8, 2 ** 32 - 1, idx, new) < 0
    # no parameters, no table to write, an unusable align, a NULL dest that claims bytes
    for t in ((None,) + tail[1:], tail[:4] + (None,) + tail[5:], tail[:5] + (None,) + tail[6:], tail[:3] + (24,) + tail[4:], tail[:3] + (8192,) + tail[4:],
              (par, None) + tail[2:]):
        assert b(2, src, 8, 1, idx, new, t) < 0 and p(2, cont, 64, off, 8, 1, idx, new, t) < 0, t
    # an offset table that decreases, or ends behind the container; a dest that begins inside the container
    assert p(2, cont, 64, falls, 8, 1, idx, new) < 0 and p(2, cont, 64, beyond, 8, 1, idx, new) < 0 and p(2, cont, 63, off, 8, 0, None, None) < 0
    assert p(2, cont, 64, off, 8, 1, idx, new, (par, vp(12288 + 63)) + tail[2:]) < 0
    assert p(2, cont, 64, off, 8, 1, idx, new, (par, vp(12288 - 4095)) + tail[2:]) < 0
    assert untouched()
    # no chunks and no indices: an empty table, nothing failed
    assert b(0, None, 8, 0, None, None) == 0 and out_off[0] == 0 and failed.value == 0
    out_off[0], failed.value = 7, 77
    assert p(0, None, 0, None, 8, 0, None, None) == 0 and out_off[0] == 0 and failed.value == 0
