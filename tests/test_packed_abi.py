"""CPU: the surface of include/blosc_gpu_packed.h - every declared name is exported by the product and listed in PACKED_SYMBOLS - and the
one call of it that needs no device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_name_is_exported_and_listed(pkg, lib):
    txt = open(os.path.join(ROOT, "include", "blosc_gpu_packed.h")).read()
    names = sorted(set(re.findall(r"BLOSC_EXPORT[^;(]*?\b(blosc_\w+)\s*\(", txt)))
    assert len(names) == 4 and names == sorted(pkg.PACKED_SYMBOLS)
    assert not set(names) & set(pkg.STOCK_SYMBOLS + pkg.GPU_SYMBOLS)
    for name in names:
        assert hasattr(lib, name), name


def test_packed_bound_is_its_formula(lib):
    sizes = [0, 1, 15, 16, 100, 4095, 4096, 4097, (1 << 22) + 8, 300001 * 8, (1 << 31) - 17]
    arr = (C.c_size_t * len(sizes))(*sizes)
    for align in (0, 1, 2, 16, 256, 4096):
        a = align or 1
        want = sum((s + 16 + a - 1) // a * a for s in sizes)
        assert lib.blosc_gpu_packed_bound(len(sizes), arr, align) == want, align
        assert lib.blosc_gpu_packed_bound(1, arr, align) == (16 + a - 1) // a * a
    for align in (3, 24, 8192, 1 << 20):                    # not a power of two in 1 ... 4096
        assert lib.blosc_gpu_packed_bound(len(sizes), arr, align) == 0
    assert lib.blosc_gpu_packed_bound(0, arr, 1) == 0
