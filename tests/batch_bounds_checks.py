"""What tests/test_gpu_batch_bounds.py (device) and tests/test_emu_batch_bounds.py (wavefront emulator) both assert about
blosc_gpu_compress_batch / blosc_gpu_decompress_batch (include/blosc_gpu.h) on "device" memory: what a chunk's own destsize decides, every
byte around a destination, and caller addresses of every residue modulo 16.  Every buffer a call writes into is compared WHOLE with an
image built on the host (sentinels, the bytes that must be there, the few bytes that are left open).  Yardsticks: the oracle and, where
oracle/_ref is built, the reference itself.  `mem` is getitem_ranges_checks.py's way to reach "device" memory."""
import ctypes as C

import numpy as np

from getitem_ranges_checks import BIG, BLOCKSIZE, SENTINEL, SMALL, odd_slots, plain
from helpers import header, orc_compress, orc_decompress, ptr, ref_decompress

GUARD = 256
TYPESIZES = [1, 2, 4, 8, 16, 3, 17]          # fused filters, stand-alone filters, the generic filter
SHUFFLES = [0, 1, 2]
DETERMINISTIC = [("lz4", 5), ("blosclz", 5), ("zstd", 5)]      # include/blosc.h: the same input and arguments give the same chunk
OTHERS = [("lz4hc", 7), ("zlib", 7), ("zstd", 7)]              # two calls may differ in size and bytes: validity and canaries only
ORACLE_WRITES = ("lz4", "blosclz")


def declare(L):
    """argtypes of the two batch calls on a library handle (the product's loader has them; the emulator build gets them here)"""
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.blosc_gpu_compress_batch.argtypes = [i, i, sz, C.c_char_p, sz, i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i), vp]
    L.blosc_gpu_decompress_batch.argtypes = [i, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(i), vp]
    return L


def is_split(cname, T):
    """blosc.c:929-959 with the forward-compatible split mode at the forced blocksize: a split block is then widened to 64 KiB"""
    return cname != "zstd" and T <= 16 and BLOCKSIZE // T >= 128


def specials():
    """100 bytes (MEMCPYED on the host), nbytes 0, 9000 random bytes (MEMCPYED by the scan)"""
    return [plain(100, seed=3), plain(0), np.random.default_rng(3).integers(0, 256, 9000, dtype=np.uint8)]


def mixed_hosts(n, seed=0, light=False):
    """8 chunks: five that compress (those of n - 1 bytes are no multiple of an even typesize, n is none of 3, 16, 17) and the specials;
    light (the emulator compresses some 45 KB a second): two that compress, the specials twice"""
    s = specials()
    if light:
        return [plain(n, 20 + seed), s[0], s[1], s[2], plain(n - 1, 21 + seed), s[0], s[1], s[2]]
    return [plain(n, 20 + seed), plain(n - 1, 21 + seed), s[0], s[1], s[2], plain(n, 22 + seed), plain(n - 1, 23 + seed), plain(n, 24 + seed)]


def guarded_slots(rooms, residues=None):
    """every room's place inside one buffer: GUARD bytes in front of it and behind it; with residues, room k at an offset congruent to
    residues[k] modulo 16 -> (offsets, size of the buffer)"""
    at, off = [], 0
    for k, w in enumerate(rooms):
        off += GUARD
        if residues is not None: off += (residues[k] - off) % 16
        at.append(off)
        off += w
    return at, off + GUARD


def check_written(image, at, spans, what, caps):
    """image: a buffer of SENTINEL bytes as a call left it.  spans[i] says what may be at at[i]: None - nothing; an array - exactly
    these bytes; an int - that many bytes are left open.  Every other byte of the buffer must still be the sentinel."""
    exp = np.full(image.size, SENTINEL, np.uint8)
    live = np.ones(image.size, bool)
    for a, s in zip(at, spans):
        if s is None: continue
        if isinstance(s, (int, np.integer)): live[a:a + int(s)] = False
        else: exp[a:a + s.size] = s
    bad = np.flatnonzero((image != exp) & live)
    if bad.size:
        b = int(bad[0])
        k = max((j for j, a in enumerate(at) if a <= b), default=-1)
        raise AssertionError((what, f"{bad.size} bytes differ, first at {b}: {int(image[b])} for {int(exp[b])}", "chunk", k,
                              "dest + %d" % (b - at[k]) if k >= 0 else "in front of the first dest", "destsize", caps[k] if k >= 0 else None,
                              "address residue", at[k] % 16 if k >= 0 else None))


def reads(oracle, ref, chunk, host, what):
    r, out = orc_decompress(oracle, chunk, host.size)
    assert r == host.size and np.array_equal(out, host), (what, "the oracle cannot read it", r)
    if ref is not None:
        r, out = ref_decompress(ref, chunk, host.size)
        assert r == host.size and np.array_equal(out, host), (what, "stock c-blosc cannot read it", r)


def compress_call(lib, mem, src, sizes, caps, setting, dest_at=None):
    """one blosc_gpu_compress_batch into one sentinel-filled buffer; chunk i at dest_at[i] (default: guarded slots wide enough for the
    whole chunk, whatever caps[i]) -> (results, image, offsets)"""
    cname, clevel, T, shuffle = setting
    n = len(src)
    if dest_at is None:
        dest_at = guarded_slots([max(c, s + 16) for c, s in zip(caps, sizes)])
    at, total = dest_at
    h, base = mem.filled(total, SENTINEL)
    res = (C.c_int * n)(*[-777] * n)
    r = lib.blosc_gpu_compress_batch(clevel, shuffle, T, cname.encode(), BLOCKSIZE, n, (C.c_void_p * n)(*src), (C.c_size_t * n)(*sizes),
                                     (C.c_void_p * n)(*[base + a for a in at]), (C.c_size_t * n)(*caps), res, None)
    assert r == 0, (setting, r)
    return list(res), mem.get(h)[:total], [base + a for a in at]


def first_call(lib, mem, oracle, ref, hosts, src, setting, deterministic, plain_idx, dest_at=None):
    """destsize = nbytes + 16: every chunk fits, decodes with everybody, writes nothing beyond its cbytes; the chunks that compress are
    regular ones where the writer is deterministic -> the chunks"""
    sizes = [h.size for h in hosts]
    caps = [s + 16 for s in sizes]
    res, image, addr = compress_call(lib, mem, src, sizes, caps, setting, dest_at)
    at = dest_at[0] if dest_at is not None else guarded_slots(caps)[0]
    assert all(0 < r <= c for r, c in zip(res, caps)), (setting, res, caps)
    check_written(image, at, res, (setting, "destsize nbytes + 16"), caps)
    chunks = [image[a:a + r].copy() for a, r in zip(at, res)]
    for k, (c, hst) in enumerate(zip(chunks, hosts)):
        assert header(c)["cbytes"] == res[k] and header(c)["nbytes"] == hst.size, (setting, k, header(c), res[k])
        reads(oracle, ref, c, hst, (setting, "chunk", k))
        if deterministic and k in plain_idx:
            assert not header(c)["flags"] & 2, (setting, "chunk", k, "is MEMCPYED: C - 1 would be the nbytes + 15 case", res[k], hst.size)
    return chunks, addr


def capacity_cases(c, nbytes, nblocks):
    """(name, destsize, fits) for a regular chunk of c bytes"""
    return [("C", c, True), ("C + 1", c + 1, True), ("nbytes + 16", nbytes + 16, True), ("nbytes + 1000", nbytes + 1000, True),
            ("C - 1", c - 1, False), ("header + bstarts - 1", 16 + 4 * nblocks - 1, False), ("16", 16, False), ("15", 15, False), ("0", 0, False)]


def check_capacity(lib, mem, oracle, ref, setting, n, deterministic, min_blocks=1, rotations=(0, 4)):
    """Case 1 of the issue: nine chunks that compress and the three specials in one batch, every chunk with a capacity of its own; with
    the second rotation of the assignment every chunk meets a capacity that fits and one that does not."""
    hosts = [plain(n - (k % 2), seed=30 + k) for k in range(9)] + specials()
    sizes = [h.size for h in hosts]
    src = [mem.put(h) for h in hosts]
    sp = [p for _, p in src]
    chunks, _ = first_call(lib, mem, oracle, ref, hosts, sp, setting, deterministic, range(9))
    for k in range(9):
        hd = header(chunks[k])
        assert -(-hd["nbytes"] // hd["blocksize"]) >= min_blocks and (min_blocks == 1 or hd["nbytes"] % hd["blocksize"]), (setting, hd)
    assert header(chunks[9])["flags"] & 2 and header(chunks[11])["flags"] & 2 and chunks[10].size == 16, setting
    for rot in rotations:
        names, caps, fits = [], [], []
        for k in range(9):
            hd = header(chunks[k])
            nm, cap, ok = capacity_cases(chunks[k].size, sizes[k], -(-hd["nbytes"] // hd["blocksize"]))[(k + rot) % 9]
            names.append(nm); caps.append(cap); fits.append(ok)
        for k in (9, 10, 11):              # the specials: what they need, or one byte less
            names.append("nbytes + 16" if rot == 0 else "nbytes + 15"); caps.append(sizes[k] + (16 if rot == 0 else 15)); fits.append(rot == 0)
        res, image, _ = compress_call(lib, mem, sp, sizes, caps, setting)
        at = guarded_slots([max(c, s + 16) for c, s in zip(caps, sizes)])[0]
        what = (setting, "rotation", rot, list(zip(names, caps)))
        spans = []
        for k, (r, cap) in enumerate(zip(res, caps)):
            if deterministic or k >= 9:
                want = chunks[k].size if fits[k] else 0
                assert r == want, (what, "chunk", k, names[k], "destsize", cap, "answered", r, "for", want)
                spans.append(chunks[k] if fits[k] else (cap if cap >= 16 else None))
            else:
                assert r == 0 or 0 < r <= cap, (what, "chunk", k, names[k], cap, r)
                assert r > 0 or cap < sizes[k] + 16, (what, "chunk", k, "destsize nbytes + 16 or more answered 0", cap)
                assert r == 0 or cap >= 16, (what, "chunk", k, cap, r)
                if r > 0:
                    c = image[at[k]:at[k] + r]
                    assert header(c)["cbytes"] == r, (what, k, header(c), r)
                    reads(oracle, ref, c, hosts[k], (what, "chunk", k, names[k]))
                spans.append(r if r > 0 else (cap if cap >= 16 else None))
        check_written(image, at, spans, what, caps)
    for (hnd, _), hst in zip(src, hosts):
        assert np.array_equal(mem.get(hnd)[:hst.size], hst), (setting, "a source was written")


def stock_compress(oracle, ref, data, cname, clevel, T, shuffle, destsize):
    """blosc_compress_ctx of the reference at this destsize (the oracle's restatement where the reference is not built) -> (result, chunk)"""
    data = np.ascontiguousarray(data) if data.size else np.zeros(1, np.uint8)[:0]
    out = np.zeros(max(destsize, 16) + 64, np.uint8)
    if ref is not None:
        r = ref.blosc_compress_ctx(clevel, shuffle, T, data.size, ptr(data), ptr(out), destsize, cname.encode(), BLOCKSIZE, 1)
        return r, out[:max(r, 0)].copy()
    r, c = orc_compress(oracle, data, T, clevel, shuffle, cname, blocksize=BLOCKSIZE, destsize=destsize)
    return r, (c if r > 0 else out[:0])


def check_policy(lib, mem, oracle, ref, cname, T, shuffle):
    """The outcomes no encoder has a say in, with the reference's return value at the same destsize: on success the reference's header and
    a MEMCPYED chunk (header + the input, so the reference's whole chunk)."""
    s100, s0, rnd = specials()
    pl = plain(SMALL)
    for clevel, batch in ((5, [(s100, 115), (s100, 116), (s0, 15), (s0, 16), (rnd, 9015), (rnd, 9016), (pl, 7)]),
                          (0, [(pl, SMALL + 15), (pl, SMALL + 16), (s100, 116), (s0, 16), (rnd, 9016), (pl, 15)])):
        setting = (cname, clevel, T, shuffle)
        hosts, caps = [h for h, _ in batch], [c for _, c in batch]
        sizes = [h.size for h in hosts]
        src = [mem.put(h) for h in hosts]
        res, image, _ = compress_call(lib, mem, [p for _, p in src], sizes, caps, setting)
        at = guarded_slots([max(c, s + 16) for c, s in zip(caps, sizes)])[0]
        spans = []
        for k, (hst, cap) in enumerate(zip(hosts, caps)):
            want, stock = stock_compress(oracle, ref, hst, cname, clevel, T, shuffle, cap)
            assert res[k] == want, (setting, "chunk", k, "nbytes", hst.size, "destsize", cap, "answered", res[k], "the reference", want)
            if want > 0:
                assert want == hst.size + 16 and header(stock)["flags"] & 2 and np.array_equal(stock[16:], hst), (setting, k, header(stock))
                got = image[at[k]:at[k] + 16]
                assert np.array_equal(got, stock[:16]), (setting, "chunk", k, "header", bytes(got).hex(), "the reference's", bytes(stock[:16]).hex())
            spans.append(stock if want > 0 else (cap if cap >= 16 else None))
        check_written(image, at, spans, (setting, "policy", caps), caps)


def odd_dest(widths):
    """odd_slots behind a guard"""
    at, total = odd_slots(widths)
    return [GUARD + a for a in at], GUARD + total + GUARD


def check_odd_compress(lib, mem, oracle, ref, setting, n, deterministic, light=False):
    """Case 2, compress: sixteen sources inside one buffer, one at every residue modulo 16, destinations at odd addresses, two calls of eight
    chunks.  Deterministic writers: the bytes of the same chunks compressed from and to memory of their own (aligned)."""
    hosts = mixed_hosts(n, 0, light) + mixed_hosts(n, 10, light)
    sizes = [h.size for h in hosts]
    s_at, s_total = guarded_slots(sizes, residues=list(range(16)))
    s_img = np.full(s_total, SENTINEL, np.uint8)
    for a, hst in zip(s_at, hosts):
        s_img[a:a + hst.size] = hst
    s_h, s_base = mem.put(s_img)
    assert sorted((s_base + a) % 16 for a in s_at) == list(range(16))
    out = []
    for half in (0, 1):
        idx = list(range(8 * half, 8 * half + 8))
        hs, sz = [hosts[k] for k in idx], [sizes[k] for k in idx]
        plain_idx = [k for k, v in enumerate(sz) if v >= n - 1]
        if deterministic:
            own = [mem.put(hst) for hst in hs]
            assert all(p % 8 == 0 for _, p in own)
            aligned, _ = first_call(lib, mem, oracle, ref, hs, [p for _, p in own], setting, True, plain_idx)
        d_at = odd_dest([s + 16 for s in sz])
        chunks, addr = first_call(lib, mem, oracle, ref, hs, [s_base + s_at[k] for k in idx], setting, deterministic, plain_idx, d_at)
        assert all(a % 2 == 1 for a in addr), addr
        if deterministic:
            for k, (c, w) in enumerate(zip(chunks, aligned)):
                if not np.array_equal(c, w):
                    m = min(c.size, w.size)
                    bad = int(np.flatnonzero(c[:m] != w[:m])[0]) if np.any(c[:m] != w[:m]) else m
                    raise AssertionError((setting, "chunk", idx[k], "source residue", (s_base + s_at[idx[k]]) % 16, "dest residue", addr[k] % 16,
                                          "sizes", c.size, w.size, "first differing byte", bad))
        out += chunks
    assert np.array_equal(mem.get(s_h)[:s_total], s_img), (setting, "the source buffer was written")
    return hosts, out


def decompress_call(lib, src, srcsize, dst, destsize):
    n = len(src)
    res = (C.c_int * n)(*[-777] * n)
    r = lib.blosc_gpu_decompress_batch(n, (C.c_void_p * n)(*src), (C.c_size_t * n)(*srcsize) if srcsize is not None else None,
                                       (C.c_void_p * n)(*dst), (C.c_size_t * n)(*destsize), res, None)
    assert r == 0, r
    return list(res)


def check_odd_decompress(lib, mem, hosts, chunks, what):
    """Case 2, decompress: sixteen chunks at odd addresses of one buffer, their destinations inside another, one at every residue modulo 16,
    two calls of eight chunks (the second without srcsize); destsize nbytes, nbytes + 37, and nbytes - 1 for three chunks of each call.
    Every mode runs twice in a row on a fresh buffer."""
    assert len(chunks) == 16
    sizes = [h.size for h in hosts]
    c_at, c_total = odd_slots([c.size for c in chunks])
    c_img = np.full(c_total, SENTINEL, np.uint8)
    for a, c in zip(c_at, chunks):
        c_img[a:a + c.size] = c
    c_h, c_base = mem.put(c_img)
    assert c_base % 2 == 0
    d_at, d_total = guarded_slots([s + 37 for s in sizes], residues=list(range(16)))
    victims = [k for half in (0, 8) for k in [j for j in range(half, half + 8) if sizes[j] > 0][::2][:3]]      # three of each call; five neighbours
    assert len(victims) == 6 and any(header(chunks[k])["flags"] & 2 for k in victims) and not all(header(chunks[k])["flags"] & 2 for k in victims)
    for mode in ("nbytes", "nbytes + 37", "nbytes - 1"):
        caps = [s + 37 if mode == "nbytes + 37" else (s - 1 if mode == "nbytes - 1" and k in victims else s) for k, s in enumerate(sizes)]
        want = [-1 if c < s else s for c, s in zip(caps, sizes)]
        spans = [None if (w <= 0) else h for w, h in zip(want, hosts)]
        for rep in range(2):
            d_h, d_base = mem.filled(d_total, SENTINEL)
            assert sorted((d_base + a) % 16 for a in d_at) == list(range(16))
            got = []
            for half in (0, 1):
                idx = range(8 * half, 8 * half + 8)
                got += decompress_call(lib, [c_base + c_at[k] for k in idx], [chunks[k].size for k in idx] if half == 0 else None,
                                       [d_base + d_at[k] for k in idx], [caps[k] for k in idx])
            assert got == want, (what, mode, "call", rep, [(k, g, w) for k, (g, w) in enumerate(zip(got, want)) if g != w])
            check_written(mem.get(d_h)[:d_total], d_at, spans, (what, "destsize", mode, "call", rep), caps)
    assert np.array_equal(mem.get(c_h)[:c_total], c_img), (what, "the chunks were written")


def stock_chunks(oracle, ref, hosts, setting):
    """the chunks as the reference writes them (the oracle for LZ4 and BloscLZ where the reference is not built, else None)"""
    cname, clevel, T, shuffle = setting
    if ref is None and cname not in ORACLE_WRITES:
        return None
    out = []
    for hst in hosts:
        r, c = stock_compress(oracle, ref, hst, cname, clevel, T, shuffle, hst.size + 16)
        assert r > 0
        out.append(c)
    return out
