"""What the CPU tests (oracle, zstd_serial.h, the emulated library) and tests/test_gpu_zstd_features.py (device) share about the fixture
tests/golden/ref_zstd_features.npz: Zstd frames the reference's own encoder wrote through its advanced API, chosen so that every optional
feature of the format (RFC 8878 3.1.1) occurs in several of them - tests/golden/make_ref_zstd_features.py is the recipe.

  census(frame)      which features a frame carries, read from its headers alone (no entropy decoding)
  make_input(...)    the input generators the fixture's recipe strings name: the plain bytes are remade, not stored
  fixture()          the frames with recipe, plain bytes and census
  check_*            the checks both sides run; `dec` is how a side reaches its decoder (EmuSide / DeviceSide below)

Yardsticks: the recorded plain bytes and the oracle's orc_decompress on the same chunk, never the library under test."""
import ctypes as C

import numpy as np

from batch_bounds_checks import GUARD, check_written, guarded_slots
from getitem_ranges_checks import SENTINEL
from helpers import DATASETS, golden_npz, orc_decompress, ptr, wrap_planes_as_chunk, wrap_stream_as_chunk

FIXTURE = "ref_zstd_features.npz"
ZSTD_FMT = 4                      # the format id of blosc's header flags (blosc.h: BLOSC_ZSTD_FORMAT)
BODY_BYTES = 24                   # damaged headers: bit flips in the first 24 bytes of a block body
DAMAGE_SEED = 20261018            # the draw of damaged-header cases: the CPU tests and the device test take the same ones
EMU_MAX = 64 << 10                # the emulated library takes the frames that decode to at most this

# ---- the census: every class the CPU census test wants in >= 3 frames (tests/golden/README.md has the counts) ----
REQUIRED = (["window_descriptor", "fcs_flag0", "fcs_flag1", "fcs_flag2", "block_raw", "block_rle", "block_compressed", "multi_block",
             "lit_raw_sf0", "lit_raw_sf1", "lit_raw_sf3", "lit_rle", "lit_huf_sf0", "lit_huf_sf1", "lit_huf_sf2", "lit_huf_sf3", "lit_treeless",
             "hufweights_fse", "hufweights_direct", "nseq_0", "nseq_1byte", "nseq_2byte"]
            + [f"{t}_{m}" for t in ("ll", "of", "ml") for m in ("predefined", "rle", "fse", "repeat")]
            + ["two_phase_lit_raw", "two_phase_lit_rle", "two_phase_lit_huf1", "two_phase_lit_huf4", "seq_overflow"])
OPTIONAL = ["nseq_3byte"]         # reached through ZSTD_compressSequences; counted, not demanded in three frames
MIN_FRAMES = 3


def walk(frame, out_size=None):
    """The headers of one frame (RFC 8878 3.1.1): frame header, block headers, and of every compressed block the literals section header,
    the first byte of a Huffman tree description, the sequence count and the modes byte.  Nothing is entropy-decoded.
    -> dict(classes, blocks=[dict(type, body, size, nseq, lit)], fcs, nseq) ; out_size (the decoded size) is needed for seq_overflow
    where the frame header carries no content size."""
    f = np.asarray(frame, np.uint8)
    cls = set()
    assert f.size >= 6 and bytes(f[:4]) == b"\x28\xb5\x2f\xfd", "not a Zstd frame"
    fhd = int(f[4])
    flag, single, checksum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
    assert not fhd & 0x08, "reserved bit"
    ip = 5
    cls.add("single_segment" if single else "window_descriptor")
    if not single:
        ip += 1
    ip += (0, 1, 2, 4)[did]
    if did: cls.add("dictionary_id")
    if checksum: cls.add("checksum")
    nb = (single, 2, 4, 8)[flag]
    fcs = int.from_bytes(bytes(f[ip:ip + nb]), "little") + (256 if nb == 2 else 0) if nb else None
    ip += nb
    cls.add(f"fcs_flag{flag}")
    if out_size is None:
        out_size = fcs
    blocks = []
    while True:
        bh = int(f[ip]) | (int(f[ip + 1]) << 8) | (int(f[ip + 2]) << 16)
        ip += 3
        last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
        assert btype != 3, "reserved block type"
        blk = dict(type=btype, body=ip, size=1 if btype == 1 else bsize, nseq=0, lit=None, last=last)
        cls.add(("block_raw", "block_rle", "block_compressed")[btype])
        if btype == 2:
            b = f[ip:ip + bsize]
            lt, sf = int(b[0]) & 3, (int(b[0]) >> 2) & 3
            if lt < 2:
                # raw / RLE literals: Size_Format ?0 is ONE class (bit 3 of the byte already belongs to the size)
                if sf in (0, 2): hdr, regen, sfc = 1, int(b[0]) >> 3, 0
                elif sf == 1: hdr, regen, sfc = 2, (int(b[0]) >> 4) | (int(b[1]) << 4), 1
                else: hdr, regen, sfc = 3, (int(b[0]) >> 4) | (int(b[1]) << 4) | (int(b[2]) << 12), 3
                p = hdr + (regen if lt == 0 else 1)
                if lt == 0: cls.add(f"lit_raw_sf{sfc}"); blk["lit"] = "raw"
                else: cls.add("lit_rle"); cls.add(f"lit_rle_sf{sfc}"); blk["lit"] = "rle"
            else:
                v = int.from_bytes(bytes(b[:5]), "little")
                if sf < 2: hdr, csize = 3, (v >> 14) & 0x3ff
                elif sf == 2: hdr, csize = 4, (v >> 18) & 0x3fff
                else: hdr, csize = 5, (v >> 22) & 0x3ffff
                if lt == 2:
                    cls.add(f"lit_huf_sf{sf}")
                    cls.add("hufweights_fse" if int(b[hdr]) < 128 else "hufweights_direct")
                    blk["lit"] = "huf1" if sf == 0 else "huf4"
                else:
                    cls.add("lit_treeless"); cls.add(f"lit_treeless_sf{sf}"); blk["lit"] = "treeless"
                p = hdr + csize
            n0 = int(b[p])
            if n0 == 0: nseq, used = 0, 1
            elif n0 < 128: nseq, used = n0, 1
            elif n0 < 255: nseq, used = ((n0 - 128) << 8) + int(b[p + 1]), 2
            else: nseq, used = int(b[p + 1]) + (int(b[p + 2]) << 8) + 0x7f00, 3
            cls.add("nseq_0" if nseq == 0 else f"nseq_{used}byte")
            blk["nseq"] = nseq
            if nseq:
                modes = int(b[p + used])
                for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
                    cls.add(f"{name}_" + ("predefined", "rle", "fse", "repeat")[(modes >> sh) & 3])
        blocks.append(blk)
        ip += blk["size"]
        if last:
            break
    assert ip + 4 * checksum == f.size, "bytes behind the frame"
    if len(blocks) > 1: cls.add("multi_block")
    b0 = blocks[0]
    # the shape k_zstd_entropy keeps for itself (k_zstd2.hip): one last compressed block, its literals not treeless, no checksum
    if len(blocks) == 1 and b0["type"] == 2 and b0["lit"] != "treeless" and not checksum:
        cls.add("two_phase_shape"); cls.add("two_phase_lit_" + b0["lit"])
        if out_size is not None and b0["nseq"] > out_size // 8:
            cls.add("seq_overflow")
    return dict(classes=cls, blocks=blocks, fcs=fcs, nseq=[b["nseq"] for b in blocks])


def census(frame, out_size=None):
    return walk(frame, out_size)["classes"]


def seq_kernel_frames(classes, nseq):
    """does k_zstd_seq decode this frame's sequences?  The two-phase shape, not handed back for its sequence count - and with sequences at
    all: a block without any is finished by k_zstd_entropy and k_zstd_exec alone (k_zstd2.hip: ZM_READY, never ZM_SEQ)."""
    return "two_phase_shape" in classes and "seq_overflow" not in classes and nseq[0] > 0


# ---- the inputs the recipes name ----
def _bits(nbits):
    return lambda n, seed: np.random.default_rng(seed).integers(0, 1 << nbits, n, dtype=np.uint8)


def _text(n, seed):
    """short random text: words of 2 - 9 letters out of a small vocabulary"""
    rng = np.random.default_rng(seed)
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(rng.integers(2, 10)))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += (words[int(rng.integers(0, 40))] + " ").encode()
    return np.frombuffer(bytes(out[:n]), np.uint8).copy()


def _tokens(n, seed):
    """a few 3- and 4-byte tokens in random order: matches of the minimum length, a sequence every few bytes"""
    rng = np.random.default_rng(seed)
    toks = [rng.integers(0, 256, int(rng.integers(3, 5)), dtype=np.uint8) for _ in range(6)]
    out = np.concatenate([toks[int(k)] for k in rng.integers(0, 6, n // 3 + 1)])
    return out[:n].copy()


def _sparse(n, seed):
    """noise with, every `seed % 64 + 5` bytes or so, four bytes seen 16 bytes earlier: the sequence count follows the gap (the search
    for frames on both sides of the two-phase path's sequence limit walks the seed)"""
    rng = np.random.default_rng(1000 + seed)
    out = rng.integers(0, 256, n, dtype=np.uint8)
    gap = seed % 64 + 5
    for p in range(32, n - 4, gap):
        out[p:p + 4] = out[p - 16:p - 12]
    return out


def _period3(n, seed):
    """three bytes over and over: whatever the match length, the source is three bytes back (the input of the explicit-sequences frames)"""
    return np.resize(np.random.default_rng(seed).integers(0, 256, 3, dtype=np.uint8), n).copy()


def _rlelit(n, seed):
    """the first half noise without the byte 0xAA; the second half 12-byte pieces of the first, a single 0xAA behind each: cut into two
    blocks in the middle, the second block's literals are that one byte, many times"""
    rng = np.random.default_rng(seed)
    h = n // 2
    out = np.empty(n, np.uint8)
    out[:h] = rng.integers(0, 128, h, dtype=np.uint8)
    p = h
    while p < n:
        o = int(rng.integers(0, h - 12)); m = min(12, n - p)
        out[p:p + m] = out[o:o + m]; p += m
        if p < n: out[p] = 0xAA; p += 1
    return out


GENERATORS = {
    "bench19": lambda n, seed: DATASETS["bench19"](n), "linspace": lambda n, seed: DATASETS["linspace"](n),
    "smallints": lambda n, seed: DATASETS["smallints"](n, seed=seed), "randwalk": lambda n, seed: DATASETS["randwalk"](n, seed=seed),
    "bits1": _bits(1), "bits2": _bits(2), "const": lambda n, seed: np.full(n, seed & 255, np.uint8), "text": _text, "tokens": _tokens,
    "sparse": _sparse, "period3": _period3, "rlelit": _rlelit,
}


def make_input(gen, n, seed):
    d = GENERATORS[gen](int(n), int(seed))
    assert d.dtype == np.uint8 and d.size == int(n)
    return d


class Entry:
    def __init__(self, k, frame, recipe, plain):
        self.k, self.frame, self.recipe, self.plain, self.n = k, frame, recipe, plain, plain.size
        w = walk(frame, plain.size)
        self.classes, self.blocks, self.nseq = w["classes"], w["blocks"], w["nseq"]
        self.seq_kernel = seq_kernel_frames(self.classes, self.nseq)

    def __repr__(self):
        return f"frame {self.k} ({self.recipe}; {self.frame.size} -> {self.n} bytes)"


_CACHE = []


def fixture():
    """[Entry] in fixture order, read (and its inputs remade) once per process; nobody writes into the arrays"""
    if not _CACHE:
        z = golden_npz(FIXTURE)
        for k, recipe in enumerate(z["recipes"]):
            gen, n, seed = str(recipe).split(",")[:3]
            plain = z[f"p{k}"] if f"p{k}" in z else make_input(gen, n, seed)
            plain.setflags(write=False); z[f"f{k}"].setflags(write=False)
            _CACHE.append(Entry(k, z[f"f{k}"], str(recipe), plain))
    return _CACHE


def wrap_frame(frame, n):
    """one unsplit block of typesize 1 around one frame"""
    return wrap_stream_as_chunk(frame, n, ZSTD_FMT)


def wrap_planes(frames, neblock):
    """one split, byte-shuffled block whose len(frames) planes are these frames (each decodes to neblock bytes)"""
    return wrap_planes_as_chunk(frames, neblock, ZSTD_FMT)


def planes_plain(plains):
    """what a block of these planes unshuffles to: byte i of plane j is byte j of element i"""
    return np.ascontiguousarray(np.stack(plains, 1)).reshape(-1)


def plane_groups(entries, T):
    """chunks of T planes out of frames of equal decoded size, both shapes mixed wherever a size has both: the frames of a size sorted
    so that two-phase and general-path frames alternate, cut into runs of T, the last run filled up from the front
    -> [(entries of the T planes)]"""
    by_n = {}
    for e in entries:
        by_n.setdefault(e.n, []).append(e)
    groups = []
    for n, es in sorted(by_n.items()):
        if len(es) < T:
            continue
        a, b = [e for e in es if e.seq_kernel], [e for e in es if not e.seq_kernel]
        mixed = [x for pair in zip(a, b) for x in pair] + a[len(b):] + b[len(a):]
        for i in range(0, len(mixed), T):
            run = mixed[i:i + T]
            groups.append(run + mixed[:T - len(run)])
    return groups


# ---- the two sides ----
class EmuSide:
    """the emulated library (tests/tools/libblosc_amd_emu.so): "device" memory is the host's"""
    def __init__(self, L, mem):
        self.L, self.mem = L, mem

    def decompress(self, chunk, n):
        chunk = np.ascontiguousarray(chunk)
        out = np.full(n + 64, 0xEE, np.uint8)
        r = self.L.blosc_decompress_ctx(ptr(chunk), ptr(out), n, 1)
        assert np.all(out[n:] == 0xEE), "wrote behind the destination"
        return r, out[:n]

    def getitem(self, chunk, start, nitems, got):
        return self.L.blosc_getitem(ptr(chunk), start, nitems, ptr(got))

    def batch(self, src, srcsize, dst, dstsize):
        n = len(src)
        res = (C.c_int * n)(*[-777] * n)
        r = self.L.blosc_gpu_decompress_batch(n, (C.c_void_p * n)(*src), (C.c_size_t * n)(*srcsize), (C.c_void_p * n)(*dst), (C.c_size_t * n)(*dstsize), res, None)
        assert r == 0, r
        return list(res)


class DeviceSide:
    """the product on the device: pkg.decompress / blosc_getitem of the C ABI, pkg.DeviceBatch for the batched call"""
    def __init__(self, pkg, lib, mem):
        self.pkg, self.lib, self.mem = pkg, lib, mem

    def decompress(self, chunk, n):
        r, out = self.pkg.decompress(chunk, n)
        return r, out

    def getitem(self, chunk, start, nitems, got):
        return self.lib.blosc_getitem(ptr(np.ascontiguousarray(chunk)), start, nitems, ptr(got))

    def batch(self, src, srcsize, dst, dstsize):
        b = self.pkg.DeviceBatch(src, srcsize, dst, dstsize)
        assert b.decompress() == 0
        return b.results()


# ---- the checks ----
def oracle_says(oracle, chunk, n, plain, what):
    r, out = orc_decompress(oracle, chunk, n)
    assert r == n and np.array_equal(out, plain), (what, "the oracle does not decode the chunk to the recorded bytes", r)


def check_single(dec, oracle, entries):
    """every frame wrapped alone, one call each"""
    for e in entries:
        chunk = wrap_frame(e.frame, e.n)
        oracle_says(oracle, chunk, e.n, e.plain, e)
        r, out = dec.decompress(chunk, e.n)
        assert r == e.n, (e, sorted(e.classes), r)
        assert np.array_equal(out[:e.n], e.plain), (e, sorted(e.classes), "first differing byte", int(np.flatnonzero(out[:e.n] != e.plain)[0]))


def check_batch(dec, oracle, chunks, plains, order, what):
    """ONE batched call over chunks[k] for k in `order`: all chunks inside one buffer, every destination with GUARD sentinel bytes in front
    of it and behind it, the destination buffer compared whole with its image"""
    cs, ps = [chunks[k] for k in order], [plains[k] for k in order]
    c_at, c_total = guarded_slots([c.size for c in cs])
    c_img = np.full(c_total, SENTINEL, np.uint8)
    for a, c in zip(c_at, cs):
        c_img[a:a + c.size] = c
    c_h, c_base = dec.mem.put(c_img)
    d_at, d_total = guarded_slots([p.size for p in ps])
    d_h, d_base = dec.mem.filled(d_total, SENTINEL)
    res = dec.batch([c_base + a for a in c_at], [c.size for c in cs], [d_base + a for a in d_at], [p.size for p in ps])
    want = [p.size for p in ps]
    assert res == want, (what, [(order[k], g, w) for k, (g, w) in enumerate(zip(res, want)) if g != w][:8])
    check_written(dec.mem.get(d_h)[:d_total], d_at, ps, what, want)
    assert np.array_equal(dec.mem.get(c_h)[:c_total], c_img), (what, "the chunks were written")


def check_planes(dec, oracle, entries, T):
    """split blocks of T planes, every plane another frame: decoded, unshuffled, and equal to the interleaved plain bytes -> chunks run"""
    groups = plane_groups(entries, T)
    for g in groups:
        chunk = wrap_planes([e.frame for e in g], g[0].n)
        want = planes_plain([e.plain for e in g])
        oracle_says(oracle, chunk, want.size, want, ("planes", T, [e.k for e in g]))
        r, out = dec.decompress(chunk, want.size)
        assert r == want.size and np.array_equal(out[:want.size], want), ("planes", T, [e.k for e in g], r)
    return groups


def check_getitem(dec, entries):
    """blosc_getitem on every wrapped frame: the first item, the last 7 items, a middle range (typesize 1: an item is a byte)"""
    for e in entries:
        chunk = wrap_frame(e.frame, e.n)
        for start, nitems in ((0, 1), (e.n - 7, 7), (e.n // 3, min(5000, e.n - e.n // 3))):
            got = np.full(nitems + 16, SENTINEL, np.uint8)
            r = dec.getitem(chunk, start, nitems, got)
            assert r == nitems and np.array_equal(got[:nitems], e.plain[start:start + nitems]) and np.all(got[nitems:] == SENTINEL), (e, start, nitems, r)


def damage_cases(entries, seed, limit=400):
    """Damaged headers: for ONE frame per census class (the smallest that has it), single-bit flips inside the first BODY_BYTES bytes of
    each block body - literals header, Huffman description, sequence count, modes byte, table descriptions.  A seeded draw of at most
    `limit` cases -> [(entry, byte offset in the frame, bit)] in a fixed order."""
    rng = np.random.default_rng(seed)
    chosen = {}
    for c in sorted(set().union(*[e.classes for e in entries])):
        best = min((e for e in entries if c in e.classes), key=lambda e: (e.n > EMU_MAX, e.frame.size, e.k))
        chosen[best.k] = best
    frames = [chosen[k] for k in sorted(chosen)]
    per = max(1, limit // len(frames))
    cases = []
    for e in frames:
        spots = [(b["body"] + i, bit) for b in e.blocks for i in range(min(BODY_BYTES, b["size"])) for bit in range(8)]
        for j in rng.permutation(len(spots))[:per]:
            cases.append((e, spots[int(j)][0], spots[int(j)][1]))
    return cases[:limit]


def damaged_chunk(e, pos, bit):
    f = e.frame.copy()
    f[pos] ^= 1 << bit
    return wrap_frame(f, e.n)


def check_verdict(decompress, oracle, case):
    """the decoder gives the oracle's verdict on a damaged chunk, and the oracle's bytes when the frame is accepted -> accepted?"""
    e, pos, bit = case
    c = damaged_chunk(e, pos, bit)
    ro, oo = orc_decompress(oracle, c, e.n)
    rg, og = decompress(c, e.n)
    if ro == e.n:
        assert rg == e.n and np.array_equal(og[:e.n], oo), (e, pos, bit, "accepted by the oracle", rg)
    else:
        assert rg < 0, (e, pos, bit, "rejected by the oracle", ro, rg)
    return ro == e.n
