"""CPU: the surface of include/blosc_gpu_getitem.h - every declared name is exported by the product and listed in GETITEM_SYMBOLS, and in
no other list."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_name_is_exported_and_listed(pkg, lib):
    txt = open(os.path.join(ROOT, "include", "blosc_gpu_getitem.h")).read()
    names = sorted(set(re.findall(r"BLOSC_EXPORT[^;(]*?\b(blosc_\w+)\s*\(", txt)))
    assert names == ["blosc_gpu_getitem_batch", "blosc_gpu_getitem_packed"] and names == sorted(pkg.GETITEM_SYMBOLS)
    assert not set(names) & set(pkg.STOCK_SYMBOLS + pkg.GPU_SYMBOLS + pkg.PACKED_SYMBOLS)
    for name in names:
        assert hasattr(lib, name), name


def test_unusable_tables_answer_without_a_device(lib):
    import ctypes as C
    one = (C.c_int * 1)(0)
    assert lib.blosc_gpu_getitem_batch(1, None, 1, one, one, one, None, one, None) < 0
    assert lib.blosc_gpu_getitem_batch(0, None, 0, None, None, None, None, None, None) == 0
    off = (C.c_size_t * 2)(7, 7)
    assert lib.blosc_gpu_getitem_packed(0, None, 0, None, 0, None, None, None, None, 0, off, None, None) == 0 and off[0] == 0
    assert lib.blosc_gpu_getitem_packed(1, None, 0, None, 1, one, one, one, None, 0, None, one, None) < 0
