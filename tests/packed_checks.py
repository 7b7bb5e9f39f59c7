"""What tests/test_gpu_packed.py (device) and tests/test_emu_packed.py (wavefront emulator) both assert about a container written by
blosc_gpu_compress_packed (include/blosc_gpu_packed.h): the expected buffer is built on the host, byte by byte, from the chunks
blosc_gpu_compress_batch wrote for destsize = nbytes + 16 and the layout rule, and compared whole - chunks, zero padding, untouched bytes
of chunks that did not fit, the guard behind destsize."""
import numpy as np

from helpers import DATASETS, orc_decompress, ref_decompress

GUARD = 64
FILL = 0xEE

MIXED_SIZES = [1 << 20, 300001 * 8, 8 * 1000, 0, 100, (1 << 22) + 8, 1 << 16]
MIXED_NAMES = ["bench19", "randwalk", "zeros", "random", "random", "linspace", "random"]
# (compressor, doshuffle, typesize)
SETTINGS = [(b"lz4", 1, 8), (b"blosclz", 1, 8), (b"zstd", 1, 8), (b"lz4", 2, 4), (b"lz4", 0, 1)]
SETTING_IDS = ["lz4-shuffle-T8", "blosclz-shuffle-T8", "zstd-shuffle-T8", "lz4-bitshuffle-T4", "lz4-noshuffle-T1"]


def mixed_batch(sizes=MIXED_SIZES):
    return [DATASETS[nm](n) for nm, n in zip(MIXED_NAMES, sizes)]


def align_up(v, a):
    return (v + a - 1) // a * a


def host_offsets(cbytes, align):
    """offsets[0] = 0, offsets[i + 1] = align_up(offsets[i] + max(cbytes_i, 0), align)"""
    off = [0]
    for c in cbytes:
        off.append(align_up(off[-1] + max(c, 0), align))
    return off


def expected_container(chunks, align, destsize):
    """(offsets, cbytes, buffer of destsize + GUARD bytes) the call must produce on a buffer prefilled with FILL.
    chunks[i]: the bytes blosc_gpu_compress_batch wrote for chunk i with destsize nbytes + 16."""
    full = [int(c.size) for c in chunks]
    off = host_offsets(full, align)
    buf = np.full(destsize + GUARD, FILL, np.uint8)
    cb = []
    for i, c in enumerate(chunks):
        if off[i] + full[i] <= destsize:
            buf[off[i]:off[i] + full[i]] = c
            buf[off[i] + full[i]:min(off[i + 1], destsize)] = 0
            cb.append(full[i])
        else:
            cb.append(0)
    return off, cb, buf


def check_container(buf, offsets, cbytes, chunks, align, destsize, what=""):
    """buf: destsize + GUARD bytes as the call left them (prefilled with FILL)."""
    off, cb, want = expected_container(chunks, align, destsize)
    assert list(offsets) == off, (what, "offsets", list(offsets)[:8], off[:8])
    assert list(cbytes) == cb, (what, "cbytes", list(cbytes)[:8], cb[:8])
    assert np.all(buf[destsize:] == FILL), (what, "bytes at or behind destsize were written")
    if not np.array_equal(buf, want):
        bad = np.flatnonzero(buf != want)
        k = int(np.searchsorted(off, bad[0], side="right")) - 1
        raise AssertionError((what, f"{bad.size} bytes differ, first at {int(bad[0])} (chunk {k} starts at {off[k]}, {cb[k]} bytes): "
                                    f"{int(buf[bad[0]])} for {int(want[bad[0]])}"))


def check_chunks_decode(chunks, hosts, oracle, ref):
    for c, h in zip(chunks, hosts):
        r, out = orc_decompress(oracle, c, h.size)
        assert r == h.size and np.array_equal(out, h), "the oracle cannot read it"
        if ref is not None:
            r, out = ref_decompress(ref, c, h.size)
            assert r == h.size and np.array_equal(out, h), "stock c-blosc cannot read it"


def capacity_cases(chunks, align):
    """(name, destsize) of the capacity test for a batch whose full container is host_offsets(...)[-1] bytes"""
    full = [int(c.size) for c in chunks]
    off = host_offsets(full, align)
    return [("the need", off[-1]), ("need - 1", off[-1] - 1), ("a cut in the middle of chunk 3", off[3] + full[3] // 2), ("nothing", 0)]
