"""CPU: include/blosc_gpu_params.h against the Python loader - the declared names, the layout of blosc_gpu_cparams, and the answers that
need no device (nchunks == 0, NULL tables)."""
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


def test_header_names_equal_the_loaders_list(pkgmod):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_params.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.PARAMS_SYMBOLS) and len(set(declared)) == len(declared), declared
    others = pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS
    assert not set(pkgmod.PARAMS_SYMBOLS) & set(others)


def test_struct_layout(pkgmod, tmp_path):
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include "blosc.h"\n#include "blosc_gpu_params.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(blosc_gpu_cparams), offsetof(blosc_gpu_cparams, splitmode), '
                   'offsetof(blosc_gpu_cparams, typesize), offsetof(blosc_gpu_cparams, blocksize)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    P = pkgmod.CParams
    assert got == [C.sizeof(P), P.splitmode.offset, P.typesize.offset, P.blocksize.offset], got
    row = pkgmod.cparams(4, 7, 2, b"zstd", 4096, 2)
    assert (row.clevel, row.doshuffle, row.compcode, row.splitmode, row.typesize, row.blocksize) == (7, 2, 5, 2, 4, 4096)
    assert pkgmod.cparams(8, cname=None).compcode == -1 and pkgmod.cparams(8, cname="lz4hc").compcode == 2 and pkgmod.cparams(8, cname=77).compcode == 77


def test_calls_that_need_no_device(pkgmod):
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    L = C.CDLL(so)
    for s in pkgmod.PARAMS_SYMBOLS:
        assert hasattr(L, s), s
    pkgmod.declare_params(L)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    rows = pkgmod.params_table([pkgmod.cparams(8)])
    src, dst, n1, res, off = (vp * 1)(0), (vp * 1)(0), (sz * 1)(0), (i * 1)(-7), (sz * 2)(5, 5)
    # nchunks == 0: nothing to do, whatever the tables
    assert L.blosc_gpu_compress_batch_params(0, None, None, None, None, None, None, None) == 0
    assert L.blosc_gpu_compress_packed_params(0, None, None, None, None, 0, 1, off, None, None) == 0 and off[0] == 0
    # NULL tables
    assert L.blosc_gpu_compress_batch_params(1, None, src, n1, dst, n1, res, None) < 0
    assert L.blosc_gpu_compress_packed_params(1, None, src, n1, None, 0, 1, off, res, None) < 0
    assert L.blosc_gpu_compress_batch_params(1, rows, None, n1, dst, n1, res, None) < 0
    assert L.blosc_gpu_compress_batch_params(1, rows, src, n1, dst, n1, None, None) < 0
    assert L.blosc_gpu_compress_packed_params(1, rows, None, n1, None, 0, 1, off, res, None) < 0
    assert L.blosc_gpu_compress_packed_params(1, rows, src, n1, None, 0, 1, None, res, None) < 0
    assert L.blosc_gpu_compress_packed_params(1, rows, src, n1, None, 0, 3, off, res, None) < 0      # an unusable align
    assert L.blosc_gpu_compress_packed_params(-1, rows, src, n1, None, 0, 1, off, res, None) < 0
    assert res[0] == -7
