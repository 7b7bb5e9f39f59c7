"""blosc_gpu_compress_batch / blosc_gpu_decompress_batch on the device the way no other test calls them (include/blosc_gpu.h): a destsize
of its own per chunk, from 0 to ample; sentinels in front of and behind every destination; caller addresses of every residue modulo 16 on
both sides - and the packed, take, put, per-chunk-parameter, select, getitem-ranges, checksum and cbuffer-sizes calls on a stream of their
own.  The checkers are
tests/batch_bounds_checks.py's (tests/test_emu_batch_bounds.py runs them on the emulated library); shapes: 40 KiB + 24 bytes where the
setting's blocks are not split, 5 x 64 KiB + 24 where they are, blocksize 8192 forced."""
import ctypes as C

import numpy as np
import pytest

import checksum_checks as cs
import concurrent_checks as cc
import params_checks as pc
import select_checks as sc
from batch_bounds_checks import (DETERMINISTIC, OTHERS, SHUFFLES, TYPESIZES, check_capacity, check_odd_compress, check_odd_decompress, check_policy,
                                 compress_call, guarded_slots, is_split, mixed_hosts, stock_chunks)
from getitem_ranges_checks import BIG, BLOCKSIZE, SENTINEL, SMALL, TorchMem, chunk_ranges, expected, odd_slots, plain, prefix, slot_widths
from helpers import orc_compress, ptr
from packed_checks import FILL, check_container, host_offsets
from put_checks import check_put
from take_checks import check_take

pytestmark = pytest.mark.gpu
ROWS = [(c, l, True) for c, l in DETERMINISTIC] + [(c, l, False) for c, l in OTHERS]
ROW_IDS = [f"{c}-clevel{l}" for c, l, _ in ROWS]


@pytest.fixture(scope="module")
def mem(pkg):
    return TorchMem()


def size_for(cname, T):
    return BIG if is_split(cname, T) else SMALL


@pytest.mark.parametrize("T", TYPESIZES)
@pytest.mark.parametrize("cname,clevel,deterministic", ROWS, ids=ROW_IDS)
def test_compress_capacity(lib, mem, oracle, ref, cname, clevel, deterministic, T):
    """every chunk's outcome is that of its own destsize: C, C + 1, nbytes + 16, nbytes + 1000 give the chunk, C - 1, a destsize that ends
    inside bstarts and 16 give 0, 15 and 0 give 0 with nothing written; not a byte outside [dest, dest + destsize) or behind cbytes"""
    for shuffle in SHUFFLES:
        check_capacity(lib, mem, oracle, ref, (cname, clevel, T, shuffle), size_for(cname, T), deterministic, min_blocks=3)


@pytest.mark.parametrize("cname,clevel,deterministic", ROWS, ids=ROW_IDS)
def test_policy_outcomes_are_the_references(lib, mem, oracle, ref, cname, clevel, deterministic):
    if ref is None and cname not in ("lz4", "blosclz"):
        cname = "lz4"                   # (the oracle writes LZ4 and BloscLZ only)
    for T in TYPESIZES:
        for shuffle in SHUFFLES:
            check_policy(lib, mem, oracle, ref, cname, T, shuffle)


@pytest.mark.parametrize("T", TYPESIZES)
@pytest.mark.parametrize("cname,clevel,deterministic", ROWS, ids=ROW_IDS)
def test_every_address_residue(lib, mem, oracle, ref, cname, clevel, deterministic, T):
    """sources at every residue modulo 16 and destinations at odd addresses for compress, chunks (the reference's and this library's) at odd
    addresses and destinations at every residue for decompress, destsize nbytes, nbytes + 37 and nbytes - 1"""
    n = size_for(cname, T)
    for shuffle in SHUFFLES:
        setting = (cname, clevel, T, shuffle)
        hosts, own = check_odd_compress(lib, mem, oracle, ref, setting, n, deterministic)
        stock = stock_chunks(oracle, ref, mixed_hosts(n, 0), setting)
        check_odd_decompress(lib, mem, hosts, (stock if stock is not None else own[:8]) + own[8:], setting)


# ---- the newer entry points on a stream of their own ----
# None of these tests can prove ordering: each fails only if work of the call lands on another stream than the one it was given AND loses the
# race against the producer enqueued there (some tens of milliseconds of matrix products, then the copy that brings the call's input).
def side_feed(dev_buf, host):
    """a new stream with, enqueued and not waited for, unrelated work and then the copy of `host` from pinned memory into dev_buf, which
    holds zeros until then -> (stream, what must stay alive)"""
    import torch
    dev_buf.zero_()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    pinned = torch.from_numpy(host).pin_memory()
    with torch.cuda.stream(s):
        a = torch.ones((4096, 4096), device=dev_buf.device)
        for _ in range(40):
            a = (a @ a) * (1.0 / 4096)
        dev_buf[:host.size].copy_(pinned, non_blocking=True)
    return s, (pinned, a)


def device_zeros(n):
    import torch
    return torch.zeros(n, dtype=torch.uint8, device=torch.device("cuda:0"))


def container_of(chunks):
    off = host_offsets([c.size for c in chunks], 1)
    return np.concatenate(chunks), off


def stock_container(oracle):
    rng = np.random.default_rng(3)
    chunks = [orc_compress(oracle, plain(BIG), 8, 5, 1, "lz4", blocksize=BLOCKSIZE)[1], orc_compress(oracle, plain(SMALL), 17, 5, 1, "blosclz", blocksize=BLOCKSIZE)[1],
              orc_compress(oracle, plain(SMALL, seed=5), 4, 5, 2, "lz4", blocksize=BLOCKSIZE)[1], orc_compress(oracle, rng.integers(0, 256, 9000, dtype=np.uint8), 4, 5, 1, "lz4")[1],
              orc_compress(oracle, plain(100), 4, 5, 1, "lz4")[1], orc_compress(oracle, plain(0), 4, 5, 1, "lz4")[1]]
    return chunks, container_of(chunks)


class SideMem:
    """the checkers' `mem` for a call on a side stream: everything happens on that stream and nothing waits for it.  put() enqueues the copy
    from pinned memory into a zeroed buffer, filled() the fill; behind side_feed's producer both are still on their way when the call is
    made.  get() waits for the stream and reads the device - except the first get() of a buffer that was put() and never read: that one
    answers the bytes on their way (put_checks.run_put looks at its sources before the call), and the next one reads the device"""
    def __init__(self, stream):
        import torch
        self.torch, self.s, self.dev, self.pinned, self.on_their_way = torch, stream, torch.device("cuda:0"), [], {}

    def put(self, a):
        a = np.ascontiguousarray(a).copy()
        with self.torch.cuda.stream(self.s):
            t = self.torch.zeros(max(a.size, 1), dtype=self.torch.uint8, device=self.dev)
            if a.size:
                self.pinned.append(self.torch.from_numpy(a).pin_memory())
                t[:a.size].copy_(self.pinned[-1], non_blocking=True)
        self.on_their_way[id(t)] = (t, a if a.size else np.zeros(1, np.uint8))      # (holding t: its id stays its own)
        return t, t.data_ptr()

    def filled(self, n, value):
        with self.torch.cuda.stream(self.s):
            t = self.torch.full((max(n, 1),), value, dtype=self.torch.uint8, device=self.dev)
        return t, t.data_ptr()

    def get(self, h):
        if id(h) in self.on_their_way:
            return self.on_their_way.pop(id(h))[1]
        with self.torch.cuda.stream(self.s):
            return h.cpu().numpy()


def busy_side_mem():
    """a SideMem on a new stream that side_feed has given some tens of milliseconds of unrelated work -> (stream, mem, what must stay alive)"""
    s, keep = side_feed(device_zeros(64), np.zeros(64, np.uint8))
    return s, SideMem(s), keep


@pytest.fixture(scope="module")
def env(pkg, lib, mem, oracle, ref):
    """concurrent_checks' environment of the row tables: the writers of their chunks"""
    made = cc.Env(pkg, cc.Recorder(lib), mem, oracle, ref)
    yield made
    made.close()      # (the global split mode, as it was found)


ROW_TABLES = [(("blosclz", 17, 2), 17), (("lz4", 8, 1), 4080)]      # (codec, typesize, filter) and row size: lanes share a row; rows cross blocks


def test_take_calls_on_a_side_stream(pkg, lib, env):
    """blosc_gpu_take_batch / blosc_gpu_take_packed with a non-NULL stream; the chunks or the container, the index table and the sentinels of
    dest and status are still on their way on that stream when the call is made.  The answers are take_checks.check_take's.  Cannot prove
    ordering (see above); the first run of these calls on a stream of the caller's at all."""
    for k, (setting, row_bytes) in enumerate(ROW_TABLES):
        t = cc.RowTable(env, setting, row_bytes, turn=k)
        for form in ("batch", "packed"):
            s, side, keep = busy_side_mem()
            source = cc.both_sources(side, t.chunks)[form]
            check_take(pkg, lib, side, source, t.chunks, t.rows_plain, row_bytes, t.index, offset=5, what=(t.name, form, "side stream"), stream=s.cuda_stream)
            s.synchronize()


def test_put_calls_on_a_side_stream(pkg, lib, mem, oracle, env):
    """blosc_gpu_put_batch / blosc_gpu_put_packed with a non-NULL stream; the chunks or the container, the index table and the new rows are
    still on their way on that stream when the call is made.  The answers are put_checks.check_put's, and the container is the NULL
    stream's byte for byte.  Cannot prove ordering (see above); the first run of these calls on a stream of the caller's at all."""
    for k, (setting, row_bytes) in enumerate(ROW_TABLES):
        t = cc.RowTable(env, setting, row_bytes, turn=k)
        for form in ("batch", "packed"):
            null, _, _ = check_put(pkg, lib, mem, oracle, t.sources[form], t.chunks, row_bytes, t.index, t.params, 256, 3, True, what=(t.name, form, "NULL stream"))
            s, side, keep = busy_side_mem()
            source = cc.both_sources(side, t.chunks)[form]
            got, _, _ = check_put(pkg, lib, side, oracle, source, t.chunks, row_bytes, t.index, t.params, 256, 3, True, what=(t.name, form, "side stream"),
                                  stream=s.cuda_stream)
            s.synchronize()
            assert np.array_equal(got, null), (t.name, form, "the side stream's container differs from the NULL stream's")


def test_params_and_select_calls_on_a_side_stream(pkg, lib, mem, oracle, ref, env):
    """blosc_gpu_compress_batch_params / _packed_params / _batch_select / _packed_select with a non-NULL stream, their sources still on their
    way on that stream when they are called.  The answers are params_checks.check_every_setting_in_one_batch's and
    select_checks.check_deterministic's, their yardstick the existing call on the NULL stream.  Cannot prove ordering (see above); the first
    run of these calls on a stream of the caller's at all."""
    hosts = mixed_hosts(SMALL)[:5]
    yard_calls = sc.Calls(pkg, lib, mem, BLOCKSIZE)
    settings, candidates = pc.deterministic_settings(2 * BLOCKSIZE), sc.candidates()
    ref_chunks, yard = pc.reference_chunks(yard_calls, hosts, settings), sc.yardstick(yard_calls, hosts, candidates)
    s, side, keep = busy_side_mem()
    calls = sc.Calls(pkg, lib, side, BLOCKSIZE)
    calls.src(hosts)
    pc.check_every_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref, aligns=(1, 256), stream=s.cuda_stream)
    s.synchronize()
    s, side, keep = busy_side_mem()
    calls = sc.Calls(pkg, lib, side, BLOCKSIZE)
    calls.src(hosts)
    sc.check_deterministic(calls, hosts, candidates, yard, oracle, ref, aligns=(1, 256), stream=s.cuda_stream)
    s.synchronize()


def test_packed_calls_on_a_side_stream(pkg, lib, mem, oracle, ref):
    """blosc_gpu_compress_packed / blosc_gpu_decompress_packed with a non-NULL stream, their input still on its way on that stream when
    they are called.  Cannot prove ordering (see above); the first run of these calls on a stream of the caller's at all."""
    import torch
    hosts = mixed_hosts(BIG)
    sizes, n = [h.size for h in hosts], len(hosts)
    s_off = host_offsets([h.size + 3 for h in hosts], 1)
    img = np.zeros(s_off[-1], np.uint8)
    for o, h in zip(s_off, hosts):
        img[o:o + h.size] = h
    for cname, shuffle, T, align in (("lz4", 1, 8, 16), ("zstd", 2, 4, 1)):
        ready, base = mem.put(img)
        res, image, _ = compress_call(lib, mem, [base + o for o in s_off[:-1]], sizes, [s + 16 for s in sizes], (cname, 5, T, shuffle))
        at = guarded_slots([s + 16 for s in sizes])[0]
        chunks = [image[a:a + r].copy() for a, r in zip(at, res)]
        destsize = host_offsets(res, align)[-1]
        pb = pkg.PackedBatch(n)
        buf0 = torch.full((destsize + 64,), FILL, dtype=torch.uint8, device=ready.device)
        assert pb.compress([base + o for o in s_off[:-1]], sizes, buf0.data_ptr(), destsize, T, 5, shuffle, cname.encode(), BLOCKSIZE, align) == 0
        off0, cb0 = pb.offsets(), pb.results()
        dev = device_zeros(img.size)
        buf = torch.full((destsize + 64,), FILL, dtype=torch.uint8, device=ready.device)
        s, keep = side_feed(dev, img)
        assert pb.compress([dev.data_ptr() + o for o in s_off[:-1]], sizes, buf.data_ptr(), destsize, T, 5, shuffle, cname.encode(), BLOCKSIZE, align, stream=s.cuda_stream) == 0
        off, cb = pb.offsets(), pb.results()
        assert off == off0 and cb == cb0 and cb == res, (cname, cb, cb0, res)
        got = buf.cpu().numpy()
        check_container(got, off, cb, chunks, align, destsize, (cname, "side stream"))
        assert np.array_equal(got, buf0.cpu().numpy())
        # ... and back: the container arrives on the stream
        total = sum(sizes)
        out0 = torch.full((total + 64,), FILL, dtype=torch.uint8, device=ready.device)
        assert pb.decompress(buf0.data_ptr(), destsize, off, out0.data_ptr(), total) == 0
        r0, o0 = pb.results(), pb.offsets()
        cont = device_zeros(destsize)
        out = torch.full((total + 64,), FILL, dtype=torch.uint8, device=ready.device)
        s, keep = side_feed(cont, got[:destsize])
        assert pb.decompress(cont.data_ptr(), destsize, off, out.data_ptr(), total, stream=s.cuda_stream) == 0
        assert pb.results() == r0 == sizes and pb.offsets() == o0 == host_offsets(sizes, 1), (cname, pb.results())
        back = out.cpu().numpy()
        assert np.array_equal(back[:total], np.concatenate(hosts)) and np.all(back[total:] == FILL) and np.array_equal(back, out0.cpu().numpy()), cname


def test_getitem_calls_on_a_side_stream(pkg, lib, mem, oracle):
    """blosc_gpu_getitem_batch / blosc_gpu_getitem_packed with a non-NULL stream, the chunks still on their way on that stream when they
    are called; results and bytes are the oracle's, range by range.  Cannot prove ordering (see above); their first run on a caller's stream."""
    chunks, (img, off) = stock_container(oracle)
    ranges = [(ci, s, k) for ci, c in enumerate(chunks) for s, k in chunk_ranges(c)] + [(len(chunks), 0, 1)]
    want = expected(oracle, chunks, ranges)
    res = [r for r, _ in want]
    at, total = odd_slots(slot_widths(chunks, ranges))
    exp = np.full(total, SENTINEL, np.uint8)
    for a, (r, data) in zip(at, want):
        if r > 0: exp[a:a + r] = data
    dev = device_zeros(img.size)
    b = pkg.ItemRanges(ranges)
    images = []
    for side in (True, False):
        out, obase = mem.filled(total, SENTINEL)
        if side:
            s, keep = side_feed(dev, img)
        assert b.batch([dev.data_ptr() + o for o in off[:-1]], [obase + a for a in at], stream=s.cuda_stream if side else None) == 0
        assert b.results() == res, (side, [(k, ranges[k], g, w) for k, (g, w) in enumerate(zip(b.results(), res)) if g != w][:8])
        images.append(mem.get(out)[:total])
        assert np.array_equal(images[-1], exp), (side, int(np.flatnonzero(images[-1] != exp)[0]))
    flat = np.concatenate([d for r, d in want if r > 0])
    for side in (True, False):
        out, obase = mem.filled(flat.size + 64, SENTINEL)
        if side:
            s, keep = side_feed(dev, img)
        assert b.packed(dev.data_ptr(), img.size, off, obase, flat.size, stream=s.cuda_stream if side else None) == 0
        assert b.results() == res and b.offsets() == prefix(res), side
        got = mem.get(out)
        assert np.array_equal(got[:flat.size], flat) and np.all(got[flat.size:] == SENTINEL), side


@pytest.mark.parametrize("kind", cs.KINDS, ids=cs.KIND_IDS)
def test_checksum_calls_on_a_side_stream(pkg, lib, kind):
    """blosc_gpu_checksum_batch / blosc_gpu_checksum_packed with a non-NULL stream, the bytes still on their way on that stream when they
    are called; the digests are zlib's.  Cannot prove ordering (see above); their first run on a caller's stream."""
    for buf, runs in (cs.alignment_case(), cs.many_runs_case()):
        want = cs.expected(kind, buf, runs)
        dev = device_zeros(buf.size)
        base = dev.data_ptr()
        s, keep = side_feed(dev, buf)
        got = pkg.checksums(kind, [base + o for o, _ in runs], [n for _, n in runs], lib=lib, stream=s.cuda_stream)
        assert got == want, [(i, runs[i]) for i in range(len(runs)) if got[i] != want[i]][:5]
        s, keep = side_feed(dev, buf)
        got = pkg.checksums_packed(kind, base, buf.size, [o for o, _ in runs] + [buf.size], [n for _, n in runs], lib=lib, stream=s.cuda_stream)
        assert got == want, [(i, runs[i]) for i in range(len(runs)) if got[i] != want[i]][:5]
        cs.check_runs(pkg, lib, kind, base, buf, runs, "default stream")


def test_cbuffer_sizes_batch_on_a_side_stream(pkg, lib, oracle):
    """blosc_gpu_cbuffer_sizes_batch with a non-NULL stream, the headers still on their way on that stream when it is called.  Cannot prove
    ordering (see above); its first run on a caller's stream."""
    chunks, (img, off) = stock_container(oracle)
    dev = device_zeros(img.size)
    pb = pkg.PackedBatch(len(chunks))
    s, keep = side_feed(dev, img)
    got = pb.sizes([dev.data_ptr() + o for o in off[:-1]], stream=s.cuda_stream)
    for k, c in enumerate(chunks):
        one = [C.c_size_t() for _ in range(3)]
        lib.blosc_cbuffer_sizes(ptr(c), *[C.byref(x) for x in one])
        assert [g[k] for g in got] == [x.value for x in one], k
    assert pb.sizes([dev.data_ptr() + o for o in off[:-1]]) == got
