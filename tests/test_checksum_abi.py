"""CPU: the surface of include/blosc_gpu_checksum.h - every declared name is exported by the product and listed in CHECKSUM_SYMBOLS, and in
no other list."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_declared_name_is_exported_and_listed(pkg, lib):
    txt = open(os.path.join(ROOT, "include", "blosc_gpu_checksum.h")).read()
    names = sorted(set(re.findall(r"BLOSC_EXPORT[^;(]*?\b(blosc_\w+)\s*\(", txt)))
    assert names == ["blosc_gpu_checksum_batch", "blosc_gpu_checksum_packed"] and names == sorted(pkg.CHECKSUM_SYMBOLS)
    assert not set(names) & set(pkg.STOCK_SYMBOLS + pkg.GPU_SYMBOLS + pkg.PACKED_SYMBOLS + pkg.GETITEM_SYMBOLS)
    for name in names:
        assert hasattr(lib, name), name
    assert int(re.search(r"#define\s+BLOSC_GPU_CHECKSUM_ADLER32\s+(\d+)", txt).group(1)) == pkg.CHECKSUM_ADLER32 == 1
    assert int(re.search(r"#define\s+BLOSC_GPU_CHECKSUM_CRC32\s+(\d+)", txt).group(1)) == pkg.CHECKSUM_CRC32 == 2


def test_unusable_arguments_answer_without_a_device(lib):
    import ctypes as C
    dig = (C.c_uint * 2)(7, 7)
    off = (C.c_size_t * 3)(0, 10, 20)
    one = (C.c_size_t * 2)(4, 4)
    ptrs = (C.c_void_p * 2)(0, 0)
    for kind in (0, 3, -1):
        assert lib.blosc_gpu_checksum_batch(kind, 2, ptrs, one, dig, None) < 0
        assert lib.blosc_gpu_checksum_packed(kind, 2, None, 20, off, None, dig, None) < 0
    assert lib.blosc_gpu_checksum_batch(1, 0, None, None, None, None) == 0
    assert lib.blosc_gpu_checksum_packed(2, 0, None, 0, None, None, None, None) == 0
    assert lib.blosc_gpu_checksum_batch(1, 2, None, one, dig, None) < 0
    assert lib.blosc_gpu_checksum_batch(1, 2, ptrs, None, dig, None) < 0
    assert lib.blosc_gpu_checksum_batch(1, 2, ptrs, one, None, None) < 0
    assert lib.blosc_gpu_checksum_packed(1, 2, None, 20, None, None, dig, None) < 0
    down = (C.c_size_t * 3)(0, 10, 9)
    assert lib.blosc_gpu_checksum_packed(1, 2, None, 20, down, None, dig, None) < 0
    assert lib.blosc_gpu_checksum_packed(1, 2, None, 19, off, None, dig, None) < 0
    long = (C.c_size_t * 2)(4, 11)
    assert lib.blosc_gpu_checksum_packed(1, 2, None, 20, off, long, dig, None) < 0
    huge = (C.c_size_t * 2)(4, (1 << 31) + 16)
    assert lib.blosc_gpu_checksum_batch(2, 2, ptrs, huge, dig, None) < 0
    assert list(dig) == [7, 7]
