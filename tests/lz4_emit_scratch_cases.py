"""The inputs of tests/test_emu_lz4_emit_scratch.py and its device twin tests/test_gpu_lz4_emit_scratch.py: one LZ4 stream per chunk
(no filter, typesize 1, the block size forced to the input's size) at the two strides of the parallel LZ4 step (enc_lz4p.h: clevel 5 probes
every other position, SS = 1; clevel 9 every position, SS = 0), sized around the 64- and 128-position steps, with contents that fill, empty
or straddle what the step hands from its rank lanes to its byte lanes.

tests/golden/lz4_emit_scratch_parent.json holds size and crc32 of every case's chunk as the encoder wrote it BEFORE the hand-over moved from
one word per position to one word per pair of positions: the parse, and with it every emitted byte, is not supposed to change.  That file is the
emulator build's; ..._parent_gpu.json is the same commit's product on the device.  The two differ in four cases (the dictionary tokens at 4097 and
65549 bytes, clevel 5): when several lanes of one step enter the same table slot, the device keeps one lane's entry and the emulator, which runs
the lanes as fibers, another's - either is a valid table, and each platform is compared with itself.
    python tests/lz4_emit_scratch_cases.py LIBRARY OUT.json      records such a file from a build of the library (emulated or device)."""
import ctypes as C
import sys
import zlib

import numpy as np

SIZES = (13, 16, 127, 128, 129, 255, 256, 257, 4097, 65549)
CLEVELS = (5, 9)               # SS = 1 / SS = 0
KINDS = ("tokens", "random", "zeros", "tokens_shifted", "match_to_step_end", "match_to_mlimit", "match_at_last_start")


def _tokens(n, clevel, seed):
    """tokens of a 16-entry dictionary, 8 bytes each (4 at clevel 9): nearly every token starts a sequence - the rank lanes are full"""
    rng = np.random.default_rng(seed)
    w = 4 if clevel >= 9 else 8
    words = rng.integers(0, 256, (16, w), dtype=np.uint8)
    return words[rng.integers(0, 16, n // w + 2)].reshape(-1)


def make_case(kind, clevel, n):
    seed = 7 * n + clevel
    rng = np.random.default_rng(1000 + seed)
    if kind == "tokens":
        return _tokens(n, clevel, seed)[:n].copy()
    if kind == "tokens_shifted":                      # matches begin on odd positions: found one byte late, the backward extension brings the byte back
        return _tokens(n, clevel, seed)[1:n + 1].copy()
    if kind == "random":                              # literal-only steps, pending literals beyond 64
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "zeros":                               # one match across the steps
        return np.zeros(n, np.uint8)
    # random head (the first step and a little more) | zeros | random tail of 40 bytes: the planted matches lie in the random parts, the zeros
    # make the stream small enough to be kept (a stream that does not shrink is stored raw, and its chunk as a plain copy)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    span = 64 if clevel >= 9 else 128                 # positions of one step
    head, tail = (span + 16, 40) if n > 2 * span + 64 else (n // 3, n // 3)
    if n - tail - head >= 16:
        a[head:n - tail] = 0
    if kind == "match_to_step_end":                   # a copy of the first bytes that ends where the second step begins, a different byte behind it
        if n > span + 1:
            L = min(28, span // 2)
            a[span - L:span] = a[:L]
            a[span] = a[L] ^ 0x55
    elif kind == "match_to_mlimit":                   # a copy that runs to the end of the input: the match has to stop at n - 5
        L = min(24, (n - 1) // 2)
        if L >= 4:
            a[n - L:] = a[:L]
    elif kind == "match_at_last_start":               # a copy that begins at n - 12, the last position a match may start at
        if n >= 32:
            a[n - 12:n - 4] = a[4:12]
    else:
        raise ValueError(kind)
    return a


def all_cases():
    for clevel in CLEVELS:
        for kind in KINDS:
            for n in SIZES:
                yield clevel, kind, n


def case_key(clevel, kind, n):
    return f"clevel{clevel}-{kind}-{n}"


def compress_host(L, data, clevel):
    """one chunk through blosc_compress_ctx of library L: (return value, the chunk)"""
    data = np.ascontiguousarray(data)
    out = np.full(data.size + 16 + 64, 0xEE, np.uint8)
    r = L.blosc_compress_ctx(clevel, 0, 1, data.size, data.ctypes.data, out.ctypes.data, data.size + 16, b"lz4", data.size, 1)
    assert np.all(out[data.size + 16:] == 0xEE)
    return r, out[:max(r, 0)].copy()


def declare(L):
    sz, i, vp = C.c_size_t, C.c_int, C.c_void_p
    L.blosc_compress_ctx.argtypes = [i, i, sz, sz, vp, vp, sz, C.c_char_p, sz, i]
    L.blosc_decompress_ctx.argtypes = [vp, vp, sz, i]
    return L


def fingerprint(chunk):
    return [int(chunk.size), int(zlib.crc32(chunk.tobytes()) & 0xFFFFFFFF)]


def same_bytes(chunk, recorded):
    """the chunk against a recorded [size, crc32], whatever bit 4 of the header's flags says ("this chunk's blocks are not split", blosc.c:1230-1237):
    the split mode is process-wide, has no getter, an earlier test may have left it anywhere and a later one may count on where it is - at typesize 1
    no block is split under any mode, so the bit is all the mode changes here, and the recorded files were written under the default mode"""
    if chunk.size < 16:
        return fingerprint(chunk) == recorded
    a, b = chunk.copy(), chunk.copy()
    a[2] &= 0xEF; b[2] |= 0x10
    return recorded in (fingerprint(a), fingerprint(b))


if __name__ == "__main__":
    lib = declare(C.CDLL(sys.argv[1]))
    table = {}
    for clevel, kind, n in all_cases():
        r, chunk = compress_host(lib, make_case(kind, clevel, n), clevel)
        assert r > 0, (clevel, kind, n, r)
        table[case_key(clevel, kind, n)] = fingerprint(chunk)
    with open(sys.argv[2], "w") as fh:
        fh.write("{\n" + ",\n".join(f' "{k}": [{v[0]}, {v[1]}]' for k, v in sorted(table.items())) + "\n}\n")
