"""What tests/test_gpu_params.py (device) and tests/test_emu_params.py (wavefront emulator) both assert about the compress calls with
parameters per chunk (include/blosc_gpu_params.h).  The yardstick of a chunk is what the EXISTING call - blosc_gpu_compress_batch with
destsize nbytes + 16, one parameter set for the batch - writes for it with the chunk's own parameters; of a container,
packed_checks.expected_container built from those chunks; of a chunk's content, the oracle and (where oracle/_ref is built) the reference.
`mem` is getitem_ranges_checks.py's way to reach "device" memory."""
import ctypes as C

import numpy as np

from batch_bounds_checks import check_written, declare, guarded_slots
from getitem_ranges_checks import SENTINEL
from helpers import header
from packed_checks import (FILL, GUARD, capacity_cases, check_chunks_decode, check_container, host_offsets)

NEVER_SPLIT, FORWARD_COMPAT_SPLIT = 2, 4      # include/blosc.h


class Setting:
    """one chunk's parameters; blocksize None: the suite's own (the emulator forces 8192, the device leaves it automatic)"""

    def __init__(self, cname, shuffle, T, clevel, splitmode=0, blocksize=None):
        self.cname, self.shuffle, self.T, self.clevel, self.splitmode, self.blocksize = cname, shuffle, T, clevel, splitmode, blocksize

    def __repr__(self):
        return f"{self.cname.decode()}-{('noshuffle', 'shuffle', 'bitshuffle')[self.shuffle]}-T{self.T}-c{self.clevel}" + \
            (f"-split{self.splitmode}" if self.splitmode else "") + (f"-bs{self.blocksize}" if self.blocksize else "")


def deterministic_settings(forced_blocksize):
    """include/blosc_gpu_params.h: blosclz, lz4, and zstd up to clevel 5 write the same bytes for the same input and parameters.
    Clevels 1, 5 and 9, one split mode of its own, one blocksize of its own (on a codec whose blocks are not split: a split block is
    widened to at least 64 KiB whatever the caller forces, blosc.c:1049-1057)."""
    return [Setting(b"lz4", 1, 8, 5), Setting(b"blosclz", 1, 8, 9), Setting(b"zstd", 1, 8, 3), Setting(b"lz4", 2, 4, 1), Setting(b"lz4", 0, 1, 5),
            Setting(b"lz4", 1, 2, 9), Setting(b"lz4", 1, 16, 1), Setting(b"lz4", 1, 8, 5, splitmode=NEVER_SPLIT),
            Setting(b"zstd", 1, 4, 5, blocksize=forced_blocksize)]


# two calls may differ in size and bytes: header, validity and cbytes only.  With the deterministic ones these are five variants of the
# encode kernel in one call: LZ (lz4, blosclz), Zstd with per-block tables (clevel 3), LZ4HC, zlib, Zstd behind the LZ4HC-grade search (clevel 7)
OTHER_SETTINGS = [Setting(b"lz4hc", 1, 8, 5), Setting(b"zlib", 1, 8, 5), Setting(b"zstd", 1, 8, 7)]
# the kernel names blosc_gpu_profile counts (unchanged by the per-chunk calls) and the launches ONE call of all twelve settings makes:
# one per variant - the two Zstd variants share a name
VARIANT_LAUNCHES = {"k_encode_streams": 1, "k_lz4hc_encode": 1, "k_zlib_encode": 1, "k_zstd_encode": 2}


def interleave(hosts, settings):
    """the batch of `hosts` repeated once per setting, neighbours never sharing a setting: chunk d * S + s = data set d with setting s
    -> [(d, s)]"""
    assert len(settings) > 1
    return [(d, s) for d in range(len(hosts)) for s in range(len(settings))]


class Calls:
    """the old and the new calls on one library handle over `mem`; sources are uploaded once and kept"""

    def __init__(self, pkgmod, lib, mem, blocksize):
        self.pkg, self.lib, self.mem, self.blocksize = pkgmod, declare(lib), mem, blocksize
        pkgmod.declare_packed(lib)
        pkgmod.declare_params(lib)
        lib.blosc_set_splitmode.argtypes = [C.c_int]
        lib.blosc_set_splitmode.restype = None
        # the global split mode has no getter and an earlier test may have left it anywhere (BLOSC_SPLITMODE is read into it by
        # blosc_compress): both the existing calls and a row with splitmode 0 read it, so it starts at the library's default, which is
        # also where old_batch puts it back
        lib.blosc_set_splitmode(FORWARD_COMPAT_SPLIT)
        self.kept = {}

    def src(self, hosts):
        for h in hosts:
            if id(h) not in self.kept: self.kept[id(h)] = (h, self.mem.put(h))
        return [self.kept[id(h)][1][1] for h in hosts]

    def bs(self, s):
        return self.blocksize if s.blocksize is None else s.blocksize

    def row(self, s):
        return self.pkg.cparams(s.T, s.clevel, s.shuffle, s.cname, self.bs(s), s.splitmode)

    # ---- the existing calls: one setting for the batch (a split mode of its own through the global, put back afterwards) ----
    def old_batch(self, hosts, s):
        """the chunks blosc_gpu_compress_batch writes with destsize nbytes + 16, as host arrays"""
        n, sizes = len(hosts), [h.size for h in hosts]
        at, total = guarded_slots([z + 16 for z in sizes])
        h, base = self.mem.filled(total, SENTINEL)
        res = (C.c_int * n)()
        if s.splitmode: self.lib.blosc_set_splitmode(s.splitmode)
        try:
            r = self.lib.blosc_gpu_compress_batch(s.clevel, s.shuffle, s.T, s.cname, self.bs(s), n, (C.c_void_p * n)(*self.src(hosts)), (C.c_size_t * n)(*sizes),
                                                  (C.c_void_p * n)(*[base + a for a in at]), (C.c_size_t * n)(*[z + 16 for z in sizes]), res, None)
        finally:
            if s.splitmode: self.lib.blosc_set_splitmode(FORWARD_COMPAT_SPLIT)
        assert r == 0 and all(c > 0 for c in res), (s, r, list(res))
        image = self.mem.get(h)
        return [image[a:a + c].copy() for a, c in zip(at, res)]

    def old_packed(self, hosts, s, align, destsize):
        b = self.pkg.PackedBatch(len(hosts), lib=self.lib)
        h, base = self.mem.filled(destsize + GUARD, FILL)
        assert b.compress(self.src(hosts), [x.size for x in hosts], base, destsize, s.T, s.clevel, s.shuffle, s.cname, self.bs(s), align) == 0
        return b.offsets(), b.results(), self.mem.get(h)[:destsize + GUARD]

    # ---- the calls with parameters per chunk ----
    def new_batch(self, hosts, rows, caps=None, dest_at=None, src=None, stream=None):
        """one blosc_gpu_compress_batch_params into one sentinel-filled buffer, chunk i at dest_at[0][i] (default: guarded slots wide
        enough for the whole chunk whatever caps[i]) -> (results, image, offsets of the destinations)"""
        n, sizes = len(hosts), [h.size for h in hosts]
        caps = [z + 16 for z in sizes] if caps is None else caps
        at, total = dest_at if dest_at is not None else guarded_slots([max(c, z + 16) for c, z in zip(caps, sizes)])
        h, base = self.mem.filled(total, SENTINEL)
        b = self.pkg.DeviceBatch(src if src is not None else self.src(hosts), sizes, [base + a for a in at], caps)
        for k in range(n): b.res[k] = -777
        assert b.compress_params(rows, stream=stream, lib=self.lib) == 0
        return b.results(), self.mem.get(h)[:total], at

    def new_packed(self, hosts, rows, align, destsize, stream=None):
        b = self.pkg.PackedBatch(len(hosts), lib=self.lib)
        h, base = self.mem.filled(destsize + GUARD, FILL)
        assert b.compress_params(self.src(hosts), [x.size for x in hosts], rows, base if destsize else None, destsize, align, stream=stream) == 0
        return b.offsets(), b.results(), self.mem.get(h)[:destsize + GUARD]

    def unpack(self, buf, off, total, stream=None):
        """the container through the existing blosc_gpu_decompress_packed -> (results, plain bytes)"""
        n = len(off) - 1
        b = self.pkg.PackedBatch(n, lib=self.lib)
        hc, pc = self.mem.put(buf)
        ho, po = self.mem.filled(total + GUARD, FILL)
        assert b.decompress(pc, buf.size, off, po, total, stream=stream) == 0
        out = self.mem.get(ho)
        assert np.all(out[total:total + GUARD] == FILL)
        return b.results(), out[:total]


def reference_chunks(calls, hosts, settings):
    """ref[s][d]: data set d through the existing call with setting s"""
    return [calls.old_batch(hosts, s) for s in settings]


# ---- case 1 ----
def check_one_setting(calls, hosts, s, align=16):
    """the same parameters in every slot: bytes, offsets and cbytes of the existing calls, every buffer compared whole"""
    old = calls.old_batch(hosts, s)
    rows = [calls.row(s)] * len(hosts)
    res, image, at = calls.new_batch(hosts, rows)
    assert res == [c.size for c in old], (s, res, [c.size for c in old])
    check_written(image, at, old, (s, "batch form"), [h.size + 16 for h in hosts])
    need = host_offsets([c.size for c in old], align)[-1]
    off, cb, buf = calls.new_packed(hosts, rows, align, need)
    check_container(buf, off, cb, old, align, need, (s, "packed form"))
    off0, cb0, buf0 = calls.old_packed(hosts, s, align, need)
    assert off == off0 and cb == cb0 and np.array_equal(buf, buf0), (s, "the two packed calls differ")


# ---- case 2 ----
def check_every_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref, aligns=(1, 16, 4096), stream=None, keep=None):
    """stream: the caller's stream of the new calls (default the NULL stream); keep: a dict that receives what they gave"""
    order = interleave(hosts, settings)
    batch = [hosts[d] for d, _ in order]
    rows = [calls.row(settings[s]) for _, s in order]
    want = [ref_chunks[s][d] for d, s in order]
    assert all(settings[order[i][1]] is not settings[order[i + 1][1]] for i in range(len(order) - 1))
    res, image, at = calls.new_batch(batch, rows, stream=stream)
    if keep is not None:
        keep.update(batch_cbytes=np.array(res, np.int64), batch_image=image)
    assert res == [c.size for c in want], ("cbytes", [(i, r, c.size) for i, (r, c) in enumerate(zip(res, want)) if r != c.size][:6])
    check_written(image, at, want, "every deterministic setting, batch form", [h.size + 16 for h in batch])
    total = sum(h.size for h in batch)
    for align in aligns:
        need = host_offsets([c.size for c in want], align)[-1]
        off, cb, buf = calls.new_packed(batch, rows, align, need, stream=stream)
        if keep is not None:
            keep.update({f"packed_offsets_align{align}": np.array(off, np.int64), f"packed_cbytes_align{align}": np.array(cb, np.int64), f"packed_container_align{align}": buf})
        check_container(buf, off, cb, want, align, need, ("every deterministic setting", align))
        assert off == host_offsets(cb, align)
        if align == aligns[0]:
            chunks = [buf[off[i]:off[i] + cb[i]] for i in range(len(batch))]
            for c, (d, s) in zip(chunks, order):
                assert header(c)["typesize"] == settings[s].T
            check_chunks_decode(chunks, batch, oracle, ref)
            r, out = calls.unpack(buf[:need], off, total, stream=stream)
            assert r == [h.size for h in batch] and np.array_equal(out, np.concatenate(batch)), "blosc_gpu_decompress_packed cannot read it back"


# ---- case 3 ----
def check_all_variants(calls, hosts, settings, ref_chunks, others, oracle, ref, align=16):
    """`settings` (deterministic, ref_chunks theirs) plus `others` in one call -> the container's offsets and cbytes"""
    every = list(settings) + list(others)
    other_chunks = reference_chunks(calls, hosts, others)
    order = interleave(hosts, every)
    batch = [hosts[d] for d, _ in order]
    rows = [calls.row(every[s]) for _, s in order]
    nd = len(settings)
    old = [ref_chunks[s][d] if s < nd else other_chunks[s - nd][d] for d, s in order]

    def check(chunks, res, what):
        for i, (c, (d, s)) in enumerate(zip(chunks, order)):
            if s < nd:
                assert np.array_equal(c, old[i]), (what, i, every[s], "differs from the existing call's chunk")
            else:
                assert np.array_equal(c[:12], old[i][:12]), (what, i, every[s], "header bytes 0 ... 11", list(c[:12]), list(old[i][:12]))
                assert res[i] == header(c)["cbytes"] == c.size, (what, i, every[s], res[i], header(c))
        check_chunks_decode(chunks, batch, oracle, ref)

    res, image, at = calls.new_batch(batch, rows)
    assert all(0 < r <= h.size + 16 for r, h in zip(res, batch)), res
    check_written(image, at, [int(r) for r in res], "all variants, batch form: bytes around the chunks", [h.size + 16 for h in batch])
    check([image[a:a + r] for a, r in zip(at, res)], res, "batch form")
    need = sum((h.size + 16 + align - 1) // align * align for h in batch)
    off, cb, buf = calls.new_packed(batch, rows, align, need)
    assert off == host_offsets(cb, align) and all(c > 0 for c in cb) and np.all(buf[need:] == FILL)
    check([buf[off[i]:off[i] + cb[i]] for i in range(len(batch))], cb, "packed form")
    for i in range(len(batch)):      # zero padding up to the next chunk, FILL behind the container
        assert not buf[off[i] + cb[i]:off[i + 1]].any(), i
    assert np.all(buf[off[-1]:] == FILL)
    r, out = calls.unpack(buf[:off[-1]], off, sum(h.size for h in batch))
    assert r == [h.size for h in batch] and np.array_equal(out, np.concatenate(batch))


# ---- case 4 ----
def bad_rows(calls):
    """(row, code): what blosc_compress_ctx rejects (-10), codes that are not built (-5), a split mode that does not exist (-10)"""
    p = calls.pkg.cparams
    bs = calls.blocksize
    return [(p(8, 10, 1, b"lz4", bs), -10), (p(8, 5, 3, b"lz4", bs), -10), (p(0, 5, 1, b"lz4", bs), -10), (p(8, 5, 1, 3, bs), -5), (p(8, 5, 1, 77, bs), -5),
            (p(8, 5, 1, b"lz4", bs, 9), -10)]


def check_errors_stay_with_their_chunk(calls, hosts, settings, align=16):
    """good chunks (setting k % S for the k-th) with the six bad slots between them: the codes, no room, not a byte, and the good chunks
    as in the same call without the bad slots"""
    good_rows = [calls.row(settings[k % len(settings)]) for k in range(len(hosts))]
    bad = bad_rows(calls)
    batch, rows, is_bad, codes = [], [], [], []
    for k, h in enumerate(hosts):
        batch.append(h); rows.append(good_rows[k]); is_bad.append(False); codes.append(None)
        if k < len(bad):
            batch.append(hosts[(k + 1) % len(hosts)] if k % 2 else h); rows.append(bad[k][0]); is_bad.append(True); codes.append(bad[k][1])
    assert sum(is_bad) == len(bad) and not is_bad[0]
    # the batch form
    res0, image0, at0 = calls.new_batch(hosts, good_rows)
    good = [image0[a:a + r].copy() for a, r in zip(at0, res0)]
    assert all(r > 0 for r in res0)
    res, image, at = calls.new_batch(batch, rows)
    it = iter(good)
    spans = [None if b else next(it) for b in is_bad]
    assert res == [codes[i] if is_bad[i] else spans[i].size for i in range(len(batch))], res
    check_written(image, at, spans, "errors, batch form", [h.size + 16 for h in batch])
    # the packed form: a failed chunk takes 0 bytes
    need = host_offsets([c.size for c in good], align)[-1]
    off0, cb0, buf0 = calls.new_packed(hosts, good_rows, align, need)
    check_container(buf0, off0, cb0, good, align, need, "the good chunks alone")
    off, cb, buf = calls.new_packed(batch, rows, align, need)
    assert cb == [codes[i] if is_bad[i] else spans[i].size for i in range(len(batch))], cb
    assert off == host_offsets(cb, align) and off[-1] == need
    assert np.array_equal(buf, buf0), "the container differs from the one without the bad slots"
    assert [off[i] for i in range(len(batch)) if not is_bad[i]] == off0[:-1]


# ---- case 5 ----
def check_capacity(calls, hosts, settings, ref_chunks, align):
    """packed_checks.capacity_cases on a container whose chunk d has setting d % S"""
    S = len(settings)
    rows = [calls.row(settings[d % S]) for d in range(len(hosts))]
    want = [ref_chunks[d % S][d] for d in range(len(hosts))]
    need = host_offsets([c.size for c in want], align)[-1]
    for name, destsize in capacity_cases(want, align):
        off, cb, buf = calls.new_packed(hosts, rows, align, destsize)
        assert off[-1] == need, (name, off[-1], need)
        check_container(buf, off, cb, want, align, destsize, (name, align))
        if name == "the need": assert all(c > 0 for c in cb)
        if name.startswith("a cut"): assert all(c > 0 for c in cb[:3]) and not any(cb[3:])
        if name == "nothing": assert not any(cb)


def check_destsize_and_addresses(calls, hosts, settings, ref_chunks):
    """the batch form, chunk d with setting d % S: a destsize below the chunk answers 0, below 16 nothing is written at all, and
    sources and destinations at odd addresses of every residue give the same chunks; sentinels around every destination"""
    S, n = len(settings), len(hosts)
    rows = [calls.row(settings[d % S]) for d in range(n)]
    want = [ref_chunks[d % S][d] for d in range(n)]
    sizes = [h.size for h in hosts]
    full = [z + 16 for z in sizes]
    # (a) every other chunk one byte short of what it needs, the next one below a header
    caps = [(want[d].size - 1 if d % 4 == 0 else (15 if d % 4 == 2 else full[d])) for d in range(n)]
    res, image, at = calls.new_batch(hosts, rows, caps=caps)
    spans = []
    for d in range(n):
        if caps[d] >= want[d].size:
            assert res[d] == want[d].size, (d, res[d]); spans.append(want[d])
        elif caps[d] < 16:
            assert res[d] == 0, (d, res[d]); spans.append(None)
        else:
            assert res[d] == 0, (d, res[d]); spans.append(caps[d])      # (what a chunk that does not fit leaves inside its destsize is open)
    check_written(image, at, spans, "destsize per chunk", caps)
    # (b) odd residues: source k at residue 2 k + 1, destination k at residue 15 - 2 k (mod 16)
    residues = [(2 * k + 1) % 16 for k in range(n)]
    s_at, s_total = guarded_slots([max(z, 1) for z in sizes], residues)
    img = np.full(s_total, SENTINEL, np.uint8)
    for a, h in zip(s_at, hosts): img[a:a + h.size] = h
    hs, ps = calls.mem.put(img)
    dest_at = guarded_slots(full, [(15 - 2 * k) % 16 for k in range(n)])
    res, image, at = calls.new_batch(hosts, rows, dest_at=dest_at, src=[ps + a for a in s_at])
    assert res == [c.size for c in want], res
    check_written(image, at, want, "odd addresses", full)
    assert np.array_equal(calls.mem.get(hs)[:s_total], img), "a source was written"
