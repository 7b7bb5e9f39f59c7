"""What tests/test_gpu_checksum.py (device) and tests/test_emu_checksum.py (wavefront emulator) both ask of include/blosc_gpu_checksum.h:
the cases are laid out in ONE host buffer per case with the runs as (offset, length) pairs, the test puts that buffer where its library
reads ("device memory": a torch tensor, or the host array itself on the emulator), and the digests are compared with Python's zlib."""
import zlib

import numpy as np

ZLIB = {1: zlib.adler32, 2: zlib.crc32}
KINDS = [1, 2]
KIND_IDS = ["adler32", "crc32"]
BASE_LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65, 5552, 5553, 65520, 65521, 65522]
CONTENTS = ["ff", "zeros", "random", "one-first", "one-last"]
FILL = 0xA5


def lengths(tile):
    return BASE_LENGTHS + [tile - 1, tile, tile + 1, 3 * tile + 7]


def content(name, n, rng):
    if name == "ff":
        return np.full(n, 0xFF, np.uint8)          # adler32: the sums overflow 32 bits long before a tile ends
    if name == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    a = np.zeros(n, np.uint8)                       # crc32 of zeros depends on the length alone: a wrong combine exponent shows
    if n and name == "one-first": a[0] = 1
    if n and name == "one-last": a[-1] = 1
    return a


def lay_out(arrays, gap=0, shifts=None):
    """(buffer, runs): the arrays one after the other in a buffer of FILL bytes, run i at a multiple of 16 plus shifts[i] (default 0),
    at least `gap` FILL bytes between two runs"""
    runs, pos = [], 16
    for i, a in enumerate(arrays):
        pos = (pos + gap + 15) // 16 * 16 + (shifts[i] if shifts else 0)
        runs.append((pos, a.size)); pos += a.size
    buf = np.full(pos + 16 + gap, FILL, np.uint8)
    for (o, n), a in zip(runs, arrays):
        buf[o:o + n] = a
    return buf, runs


def expected(kind, buf, runs):
    return [ZLIB[kind](buf[o:o + n].tobytes()) & 0xffffffff for o, n in runs]


def grid_case(tile, seed=11):
    rng = np.random.default_rng(seed)
    return lay_out([content(c, n, rng) for n in lengths(tile) for c in CONTENTS])


def alignment_case(seed=12):
    """runs of 1000 + k random bytes that start k bytes behind a 16-byte boundary, k = 0 .. 15, FILL all around them"""
    rng = np.random.default_rng(seed)
    return lay_out([rng.integers(0, 256, 1000 + k, dtype=np.uint8) for k in range(16)], gap=40, shifts=list(range(16)))


LONG_COUNTS = (4096, 4097, 5000)      # k_checksum.hip's ck_find_run probes 64 places a round: two rounds reach 64^2 = 4096 runs, more take a third


def long_search_case(nruns, seed=18):
    """runs of 0 ... 200 random bytes at random shifts; the first and the last run empty, runs 100 ... 169 empty - 70 in a row, more than
    one round's 64 probes - and, with 5000 runs, runs 400 ... 4499 as well: 4100 in a row, more than two rounds' 4096"""
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(0, 201, nruns)]
    sizes[0] = sizes[-1] = 0
    sizes[100:170] = [0] * 70
    if nruns >= 5000:
        sizes[400:4500] = [0] * 4100
    assert sizes[99] and sizes[170] and (nruns < 5000 or (sizes[399] and sizes[4500]))
    return lay_out([rng.integers(0, 256, n, dtype=np.uint8) for n in sizes], shifts=[int(s) for s in rng.integers(0, 16, nruns)])


def many_runs_case(seed=13, nruns=300, longest=3000):
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.integers(0, longest + 1, nruns)]
    for k in (0, 5, 77, nruns - 1):
        sizes[k] = 0
    return lay_out([rng.integers(0, 256, n, dtype=np.uint8) for n in sizes], shifts=[int(s) for s in rng.integers(0, 16, nruns)])


def aligned_copy(buf):
    """the same bytes in a host array whose first byte lies on a 16-byte boundary (the emulator reads host memory)"""
    raw = np.empty(buf.size + 16, np.uint8)
    o = (-raw.ctypes.data) % 16
    out = raw[o:o + buf.size]
    out[:] = buf
    return out


def check_runs(pkg, lib, kind, base_ptr, buf, runs, what=""):
    """base_ptr: where buf lies in the memory the library reads.  Both calls: a pointer per run, and the runs by offset table with their
    lengths (the runs of lay_out rise)."""
    want = expected(kind, buf, runs)
    got = pkg.checksums(kind, [base_ptr + o for o, _ in runs], [n for _, n in runs], lib=lib)
    bad = [(i, runs[i], hex(got[i]), hex(want[i])) for i in range(len(runs)) if got[i] != want[i]]
    assert not bad, (what, KIND_IDS[kind - 1], "batch", len(bad), bad[:5])
    got = pkg.checksums_packed(kind, base_ptr, buf.size, [o for o, _ in runs] + [buf.size], [n for _, n in runs], lib=lib)
    bad = [(i, runs[i], hex(got[i]), hex(want[i])) for i in range(len(runs)) if got[i] != want[i]]
    assert not bad, (what, KIND_IDS[kind - 1], "packed", len(bad), bad[:5])
