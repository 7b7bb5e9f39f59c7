"""The packed batch calls on the device (include/blosc_gpu_packed.h): a whole batch compressed into, and decompressed from, ONE device
buffer.  Yardsticks: blosc_gpu_compress_batch's bytes for destsize = nbytes + 16, the layout rule restated on the host
(tests/packed_checks.py), the oracle and the reference."""
import ctypes as C

import numpy as np
import pytest

from helpers import DATASETS, ptr, ref_compress
from packed_checks import (FILL, GUARD, SETTINGS, SETTING_IDS, capacity_cases, check_chunks_decode, check_container, host_offsets,
                           mixed_batch)

pytestmark = pytest.mark.gpu


def to_dev(hosts):
    import torch
    dev = torch.device("cuda:0")
    return [torch.from_numpy(h).to(dev) if h.size else torch.empty(0, dtype=torch.uint8, device=dev) for h in hosts]


def batch_chunks(pkg, src, sizes, T, shuffle, cname):
    """what blosc_gpu_compress_batch writes with destsize nbytes + 16 for every chunk, as host arrays"""
    import torch
    dst = [torch.full((n + 16,), FILL, dtype=torch.uint8, device=src[0].device) for n in sizes]
    b = pkg.DeviceBatch([t.data_ptr() for t in src], sizes, [t.data_ptr() for t in dst], [n + 16 for n in sizes])
    assert b.compress(T, 5, shuffle, cname) == 0
    cb = b.results()
    assert all(c > 0 for c in cb), cb
    return [d[:c].cpu().numpy() for d, c in zip(dst, cb)]


def packed(pkg, src, sizes, T, shuffle, cname, align, destsize):
    import torch
    b = pkg.PackedBatch(len(sizes))
    buf = torch.full((destsize + GUARD,), FILL, dtype=torch.uint8, device=src[0].device)
    assert b.compress([t.data_ptr() for t in src], sizes, buf.data_ptr(), destsize, T, 5, shuffle, cname, 0, align) == 0
    return b.offsets(), b.results(), buf.cpu().numpy()


@pytest.fixture(scope="module")
def mixed():
    hosts = mixed_batch()
    return hosts, to_dev(hosts), [h.size for h in hosts]


@pytest.fixture(scope="module")
def mixed_lz4_chunks(pkg, mixed):
    hosts, src, sizes = mixed
    return batch_chunks(pkg, src, sizes, 8, 1, b"lz4")


@pytest.mark.parametrize("cname,shuffle,T", SETTINGS, ids=SETTING_IDS)
def test_mixed_batch_every_fallback(pkg, oracle, ref, mixed, cname, shuffle, T):
    hosts, src, sizes = mixed
    chunks = batch_chunks(pkg, src, sizes, T, shuffle, cname)
    flags = [int(c[2]) for c in chunks]
    assert flags[4] & 2 and flags[6] & 2 and not flags[2] & 2, flags            # MEMCPYED: below 128 bytes (host), random bytes (scan); not the zeros
    bs = int(chunks[1][8:12].view("<i4")[0])
    assert bs < sizes[1] and sizes[1] % bs                                       # full blocks and a leftover block
    for align in (1, 16, 4096):
        need = host_offsets([c.size for c in chunks], align)[-1]
        assert need <= pkg.PackedBatch(len(sizes)).bound(sizes, align)
        off, cb, buf = packed(pkg, src, sizes, T, shuffle, cname, align, need)
        assert off == host_offsets(cb, align)
        check_container(buf, off, cb, chunks, align, need, (cname, align))
        if align == 16:
            check_chunks_decode([buf[off[i]:off[i] + cb[i]] for i in range(len(sizes))], hosts, oracle, ref)


def test_more_chunks_than_one_workgroup_is_wide(pkg, oracle, ref):
    rng = np.random.default_rng(700)
    sizes = [int(s) * 8 for s in rng.integers((4 << 10) // 8, (12 << 10) // 8 + 1, 700)]
    hosts = [DATASETS["bench19" if k % 3 else "random"](n) for k, n in enumerate(sizes)]
    src = to_dev(hosts)
    chunks = batch_chunks(pkg, src, sizes, 8, 1, b"lz4")
    for align in (1, 256):
        need = host_offsets([c.size for c in chunks], align)[-1]
        off, cb, buf = packed(pkg, src, sizes, 8, 1, b"lz4", align, need)
        assert off == host_offsets(cb, align)
        check_container(buf, off, cb, chunks, align, need, align)
        check_chunks_decode([buf[off[i]:off[i] + cb[i]] for i in range(len(sizes))], hosts, oracle, ref)


def test_capacity(pkg, mixed, mixed_lz4_chunks):
    hosts, src, sizes = mixed
    chunks, n = mixed_lz4_chunks, len(sizes)
    need = host_offsets([c.size for c in chunks], 1)[-1]
    for align in (1, 16):
        need = host_offsets([c.size for c in chunks], align)[-1]
        for name, destsize in capacity_cases(chunks, align):
            off, cb, buf = packed(pkg, src, sizes, 8, 1, b"lz4", align, destsize)
            assert off[n] == need, (name, off[n], need)
            # whole-buffer comparison: written chunks, zero padding below destsize, FILL in the room of unwritten chunks and behind destsize
            check_container(buf, off, cb, chunks, align, destsize, (name, align))
            if name == "the need": assert all(c > 0 for c in cb)
            if name == "need - 1" and align == 1: assert all(c > 0 for c in cb[:-1]) and cb[-1] == 0
            if name.startswith("a cut"): assert all(c > 0 for c in cb[:3]) and not any(cb[3:])
            if name == "nothing": assert not any(cb)


def test_offsets_past_4_gib(pkg):
    """70 chunks of 64 MiB of random bytes: every chunk is MEMCPYED, the container is 4.38 GiB - the smallest shape at which a layout
    scan in 32 bits goes wrong."""
    import torch
    dev = torch.device("cuda:0")
    n, size = 70, 64 << 20
    g = torch.Generator(device=dev); g.manual_seed(4)
    data = torch.randint(0, 256, (n * size,), dtype=torch.uint8, device=dev, generator=g)
    b = pkg.PackedBatch(n)
    need = b.bound([size] * n, 1)
    cont = torch.empty(need, dtype=torch.uint8, device=dev)
    assert b.compress([data.data_ptr() + k * size for k in range(n)], [size] * n, cont.data_ptr(), need, 8, 5, 1, b"lz4", 0, 1) == 0
    off, cb = b.offsets(), b.results()
    assert cb == [size + 16] * n and off == host_offsets(cb, 1) and off[-1] > 2 ** 32
    out = torch.full((n * size,), FILL, dtype=torch.uint8, device=dev)
    assert b.decompress(cont.data_ptr(), need, off, out.data_ptr(), n * size) == 0
    assert b.results() == [size] * n and b.offsets() == [k * size for k in range(n + 1)]
    for k in range(n):
        assert torch.equal(out[k * size:(k + 1) * size], data[k * size:(k + 1) * size]), k


@pytest.fixture(scope="module")
def ref_container(ref, mixed):
    """reference-written chunks of the mixed batch with 0 ... 15 bytes of junk between them"""
    hosts, _, sizes = mixed
    assert ref is not None
    rng = np.random.default_rng(5)
    chunks = [ref_compress(ref, h, 8, 5, 1, b"lz4")[1] for h in hosts]
    parts, offs = [], [0]
    for k, c in enumerate(chunks):
        junk = rng.integers(0, 256, k * 5 % 16, dtype=np.uint8)
        parts += [c, junk]
        offs.append(offs[-1] + c.size + junk.size)
    return chunks, np.concatenate(parts), offs


def test_decompress_packed(pkg, mixed, ref_container):
    import torch
    hosts, _, sizes = mixed
    chunks, cont, offs = ref_container
    n, total = len(sizes), sum(sizes)
    dev = torch.device("cuda:0")
    d_cont = torch.from_numpy(cont).to(dev)
    b = pkg.PackedBatch(n)
    # the size query
    assert b.decompress(d_cont.data_ptr(), cont.size, offs, None, 0) == 0
    assert b.results() == sizes and b.offsets() == host_offsets(sizes, 1)
    # the real call
    out = torch.full((total + GUARD,), FILL, dtype=torch.uint8, device=dev)
    assert b.decompress(d_cont.data_ptr(), cont.size, offs, out.data_ptr(), total) == 0
    assert b.results() == sizes and b.offsets() == host_offsets(sizes, 1)
    got = out.cpu().numpy()
    for k, h in enumerate(hosts):
        assert np.array_equal(got[b.offsets()[k]:b.offsets()[k + 1]], h), k
    assert np.all(got[total:] == FILL)
    # a damaged version byte: that chunk fails alone, with width 0
    bad = cont.copy(); bad[offs[1]] = 9
    d_bad = torch.from_numpy(bad).to(dev)
    out.fill_(FILL)
    assert b.decompress(d_bad.data_ptr(), bad.size, offs, out.data_ptr(), total) == 0
    assert b.results() == [s if k != 1 else -1 for k, s in enumerate(sizes)]
    assert b.offsets() == host_offsets([s if k != 1 else 0 for k, s in enumerate(sizes)], 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[:total - sizes[1]], np.concatenate([h for k, h in enumerate(hosts) if k != 1])) and np.all(got[total - sizes[1]:] == FILL)
    # a destination that cuts the last chunk: -1 for it, its slot untouched
    out.fill_(FILL)
    assert b.decompress(d_cont.data_ptr(), cont.size, offs, out.data_ptr(), total - 1) == 0
    assert b.results() == sizes[:-1] + [-1] and b.offsets() == host_offsets(sizes, 1)
    got = out.cpu().numpy()
    assert np.array_equal(got[:total - sizes[-1]], np.concatenate(hosts[:-1])) and np.all(got[total - sizes[-1]:] == FILL)
    # tables that are unusable as a whole
    out.fill_(FILL)
    down = list(offs); down[2] = down[1] - 1
    assert b.decompress(d_cont.data_ptr(), cont.size, down, out.data_ptr(), total) < 0
    assert b.decompress(d_cont.data_ptr(), cont.size - 1, offs, out.data_ptr(), total) < 0
    assert np.all(out.cpu().numpy() == FILL)


def test_cbuffer_sizes_batch(pkg, lib, mixed, ref_container):
    import torch
    chunks, cont, offs = ref_container
    d_cont = torch.from_numpy(cont).to(torch.device("cuda:0"))
    got = pkg.PackedBatch(len(chunks)).sizes([d_cont.data_ptr() + o for o in offs[:-1]])
    for k, c in enumerate(chunks):
        one = [C.c_size_t() for _ in range(3)]
        lib.blosc_cbuffer_sizes(ptr(c), *[C.byref(x) for x in one])
        assert [g[k] for g in got] == [x.value for x in one], k
