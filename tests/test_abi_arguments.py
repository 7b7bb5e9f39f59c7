"""CPU: what every exported batch entry point answers to unusable and edge arguments, pinned.

Every batch call of include/blosc_gpu.h, blosc_gpu_packed.h, blosc_gpu_params.h, blosc_gpu_getitem.h and blosc_gpu_checksum.h is called on the
emulated library with a fixed list of arguments; the whole-call return value, the per-item result array and the offset table (where the call
has one) are compared with tests/golden/abi_arguments.json, which tests/golden/make_abi_arguments.py wrote once (tests/golden/README.md names
the commit).  Outputs start filled with a sentinel; an entry the call left alone is recorded as "untouched".  The same file pins the sha256 of
the files blpk.pack writes for three small inputs, and that blpk.pack_device writes the same bytes.

The sources of the compress calls are random bytes: every chunk is stored (MEMCPYED), so cbytes = nbytes + 16 whatever the encoders do, and
the recorded numbers depend on the argument handling alone.  For chunks that reach a destination the first 12 header bytes are recorded too
(typesize, filter and codec flags, block size: what a mix-up of the parameters would change).

Left out, because the call reads through the pointer without a check (the headers say "no checks" for these; nothing here is meant to crash):
  * blosc_gpu_compress_batch, blosc_gpu_compress_batch_host, blosc_gpu_compress_batch_multi with nchunks > 0: src, nbytes, dest, destsize or
    cbytes_out NULL
  * blosc_gpu_decompress_batch, blosc_gpu_decompress_batch_host, blosc_gpu_decompress_batch_multi with nchunks > 0: src, dest, destsize or
    nbytes_out NULL (srcsize NULL is a documented value and is in the list)
  * blosc_gpu_compress_batch_multi / blosc_gpu_decompress_batch_multi: devices NULL is a documented value (device r for range r) and is in
    the list
  * a run longer than INT32_MAX + 16 is only given as a size with a NULL pointer, never with memory behind it
"""
import ctypes as C
import hashlib
import importlib.util
import io
import json
import os

import numpy as np
import pytest

from helpers import DATASETS
from test_emu_blpk_device import NumpyMem
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_arguments.json")
SIZES = [2048, 4096, 3000]            # three chunks of 2 - 4 KiB, typesize 8
T, BS = 8, 512                        # the forced block size keeps the emulator at a few blocks per chunk
I_SENT, Z_SENT, U_SENT = -77, 0xEEEEEEEEEEEEEEEE, 0xDEADBEEF
HUGE = (1 << 31) - 1 + 16 + 1         # one byte beyond the longest run a checksum call takes
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int


def _module(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _seen(arr, sentinel):
    return None if arr is None else ["untouched" if v == sentinel else int(v) for v in arr]


def iarr(n):
    return (ci * max(n, 1))(*[I_SENT] * max(n, 1))


def zsent(n):
    return (sz * max(n, 1))(*[Z_SENT] * max(n, 1))


def usent(n):
    return (C.c_uint * max(n, 1))(*[U_SENT] * max(n, 1))


def zarr(vals):
    return (sz * max(len(vals), 1))(*vals)


def parr(vals):
    return (vp * max(len(vals), 1))(*vals)


def intarr(vals):
    return (ci * max(len(vals), 1))(*vals)


class World:
    """The valid inputs, and one function per entry point that calls it with the valid arguments except for what the case names."""

    def __init__(self, L, pkgmod):
        self.L, self.pkg = L, pkgmod
        for f in (pkgmod.declare_packed, pkgmod.declare_params, pkgmod.declare_getitem, pkgmod.declare_checksum):
            f(L)
        L.blosc_get_compressor.restype = C.c_char_p
        L.blosc_set_compressor.argtypes = [C.c_char_p]
        L.blosc_set_blocksize.argtypes = [sz]
        L.blosc_set_blocksize.restype = None
        L.blosc_compress_ctx.argtypes = [ci, ci, sz, sz, vp, vp, sz, C.c_char_p, sz, ci]
        rnd = DATASETS["random"](sum(SIZES))
        cuts = np.cumsum([0] + SIZES)
        self.plain = [rnd[a:b].copy() for a, b in zip(cuts[:-1], cuts[1:])]          # sources of the compress calls: stored, never compressed
        self.soft = [DATASETS["bench19"](n) for n in SIZES]                           # what the chunks of the reading calls hold
        self.chunks = []
        for s in self.soft:
            out = np.zeros(s.size + 16, np.uint8)
            r = L.blosc_compress_ctx(5, 1, T, s.size, s.ctypes.data, out.ctypes.data, out.size, b"lz4", BS, 1)
            assert 16 < r < s.size
            self.chunks.append(out[:r].copy())
        self.runs = np.arange(64, dtype=np.uint8)                                      # plain bytes for the checksum calls

    def container(self, gaps=(0, 0, 0), chunks=None):
        """the chunks one behind the other with gaps[i] bytes of 0xA5 behind chunk i; returns (buffer, offsets[n + 1])"""
        chunks = self.chunks if chunks is None else chunks
        parts, off = [], [0]
        for c, g in zip(chunks, gaps):
            parts += [c, np.full(g, 0xA5, np.uint8)]
            off.append(off[-1] + c.size + g)
        return np.concatenate(parts), off

    # ---- include/blosc_gpu.h ----
    def compress_batch(self, host=False, n=3, clevel=5, cname=b"lz4", room=16):
        m = max(n, 0)
        dst = [np.full(s.size + room, 0xEE, np.uint8) for s in self.plain[:m]]
        out = iarr(m)
        args = [ci(clevel), ci(1), sz(T), C.c_char_p(cname), sz(BS), ci(n), parr([s.ctypes.data for s in self.plain[:m]]), zarr(SIZES[:m]),
                parr([d.ctypes.data for d in dst]), zarr([d.size for d in dst]), out]
        r = self.L.blosc_gpu_compress_batch_host(*args) if host else self.L.blosc_gpu_compress_batch(*args, vp(None))
        return dict(ret=r, results=_seen(out, I_SENT), headers=[bytes(d[:12]).hex() if c > 0 else None for d, c in zip(dst, out)])

    def decompress_batch(self, host=False, n=3, srcsize=True, short=0):
        m = max(n, 0)
        dst = [np.full(s.size, 0xEE, np.uint8) for s in self.soft[:m]]
        out = iarr(m)
        args = [ci(n), parr([c.ctypes.data for c in self.chunks[:m]]), zarr([c.size - short for c in self.chunks[:m]]) if srcsize else None,
                parr([d.ctypes.data for d in dst]), zarr([d.size for d in dst]), out]
        r = self.L.blosc_gpu_decompress_batch_host(*args) if host else self.L.blosc_gpu_decompress_batch(*args, vp(None))
        for d, s, c in zip(dst, self.soft, out):
            assert c != s.size or np.array_equal(d, s)
        return dict(ret=r, results=_seen(out, I_SENT))

    def multi(self, compress, ndev=1, devices=None, n=3, cname=b"lz4"):
        m = max(n, 0)
        src = self.plain[:m] if compress else self.chunks[:m]
        dst = [np.full(s.size + 16, 0xEE, np.uint8) for s in self.soft[:m]]
        out = iarr(m)
        tail = [ci(n), parr([s.ctypes.data for s in src]), zarr([s.size for s in src]), parr([d.ctypes.data for d in dst]), zarr([d.size for d in dst]), out]
        head = [ci(ndev), intarr(devices) if devices is not None else None]
        if compress:
            r = self.L.blosc_gpu_compress_batch_multi(*head, ci(5), ci(1), sz(T), C.c_char_p(cname), sz(BS), *tail)
        else:
            r = self.L.blosc_gpu_decompress_batch_multi(*head, *tail)
        return dict(ret=r, results=_seen(out, I_SENT))

    # ---- include/blosc_gpu_packed.h, include/blosc_gpu_params.h ----
    def bound(self, n=3, nbytes=True, align=1):
        return dict(ret=int(self.L.blosc_gpu_packed_bound(n, zarr(SIZES[:max(n, 0)]) if nbytes else None, align)))

    def compress_packed(self, params=None, n=3, null=(), destsize=None, align=1, clevel=5, cname=b"lz4"):
        """params: None - blosc_gpu_compress_packed; a list of rows - blosc_gpu_compress_packed_params"""
        m = max(n, 0)
        room = sum(SIZES) + 16 * 3 + 3 * 8192
        buf = np.full(room, 0xEE, np.uint8)
        off, out = zsent(m + 1), iarr(m)
        a = dict(src=parr([s.ctypes.data for s in self.plain[:m]]), nbytes=zarr(SIZES[:m]), dest=buf.ctypes.data, offsets_out=off, cbytes_out=out,
                 params=self.pkg.params_table(params) if params is not None else None)
        for name in null:
            a[name] = None
        destsize = (room if a["dest"] is not None else 0) if destsize is None else destsize
        if params is None:
            r = self.L.blosc_gpu_compress_packed(clevel, 1, T, cname, BS, n, a["src"], a["nbytes"], a["dest"], destsize, align, a["offsets_out"], a["cbytes_out"], None)
        else:
            r = self.L.blosc_gpu_compress_packed_params(n, a["params"], a["src"], a["nbytes"], a["dest"], destsize, align, a["offsets_out"], a["cbytes_out"], None)
        heads = [bytes(buf[o:o + 12]).hex() if c > 0 and o != Z_SENT else None for o, c in zip(off, out)] if a["dest"] is not None else None
        return dict(ret=r, results=_seen(out, I_SENT), offsets=_seen(off, Z_SENT), headers=heads, touched=bool(np.any(buf != 0xEE)))

    def compress_batch_params(self, params, n=3, null=()):
        m = max(n, 0)
        dst = [np.full(s.size + 16, 0xEE, np.uint8) for s in self.plain[:m]]
        out = iarr(m)
        a = dict(params=self.pkg.params_table(params), src=parr([s.ctypes.data for s in self.plain[:m]]), nbytes=zarr(SIZES[:m]),
                 dest=parr([d.ctypes.data for d in dst]), destsize=zarr([d.size for d in dst]), cbytes_out=out)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_compress_batch_params(n, a["params"], a["src"], a["nbytes"], a["dest"], a["destsize"], a["cbytes_out"], None)
        return dict(ret=r, results=_seen(out, I_SENT), headers=[bytes(d[:12]).hex() if c > 0 else None for d, c in zip(dst, out)])

    def decompress_packed(self, n=3, null=(), cont=None, containersize=None, destsize=None):
        buf, off = self.container() if cont is None else cont
        m = max(n, 0)
        total = sum(SIZES)
        dst = np.full(total, 0xEE, np.uint8)
        doff, out = zsent(m + 1), iarr(m)
        a = dict(container=buf.ctypes.data if buf is not None else None, offsets=zarr(off), dest=dst.ctypes.data, dest_offsets_out=doff, nbytes_out=out)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_decompress_packed(n, a["container"], (buf.size if buf is not None else 0) if containersize is None else containersize, a["offsets"],
                                               a["dest"], total if destsize is None else destsize, a["dest_offsets_out"], a["nbytes_out"], None)
        return dict(ret=r, results=_seen(out, I_SENT), offsets=_seen(doff, Z_SENT), touched=bool(np.any(dst != 0xEE)))

    def sizes_batch(self, n=3, null=(), chunks=None):
        m = max(n, 0)
        chunks = self.chunks if chunks is None else chunks
        a = dict(src=parr([c.ctypes.data for c in chunks[:m]]), nbytes=zsent(m), cbytes=zsent(m), blocksize=zsent(m))
        outs = dict(a)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_cbuffer_sizes_batch(n, a["src"], a["nbytes"], a["cbytes"], a["blocksize"], None)
        return dict(ret=r, nbytes=_seen(outs["nbytes"], Z_SENT), blocksize=_seen(outs["blocksize"], Z_SENT),
                    cbytes_is_the_chunks=[int(v) == c.size for v, c in zip(outs["cbytes"], chunks[:m])])

    # ---- include/blosc_gpu_getitem.h ----
    RANGES = [(0, 0, 10), (2, 100, 50), (1, 500, 12), (3, 0, 1), (-1, 0, 1), (1, 512, 1), (1, -1, 2), (0, 250, 6), (0, 256, 0)]

    def getitem_batch(self, nchunks=3, nranges=None, null=(), ranges=None):
        ranges = self.RANGES if ranges is None else ranges
        nr = len(ranges) if nranges is None else nranges
        dst = [np.full(max(r[2], 0) * T + 8, 0xEE, np.uint8) for r in ranges]
        out = iarr(len(ranges))
        a = dict(src=parr([c.ctypes.data for c in self.chunks[:max(nchunks, 0)]]), chunk=intarr([r[0] for r in ranges]), start=intarr([r[1] for r in ranges]),
                 nitems=intarr([r[2] for r in ranges]), dest=parr([d.ctypes.data for d in dst]), result_out=out)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_getitem_batch(nchunks, a["src"], nr, a["chunk"], a["start"], a["nitems"], a["dest"], a["result_out"], None)
        for (c, s, k), d, got in zip(ranges, dst, out):
            assert got <= 0 or (got == k * T and np.array_equal(d[:got], self.soft[c][s * T:(s + k) * T]) and np.all(d[got:] == 0xEE))
        return dict(ret=r, results=_seen(out, I_SENT))

    def getitem_packed(self, nchunks=3, nranges=None, null=(), ranges=None, cont=None, containersize=None, destsize=None):
        ranges = self.RANGES if ranges is None else ranges
        nr = len(ranges) if nranges is None else nranges
        buf, off = self.container() if cont is None else cont
        room = sum(max(r[2], 0) for r in ranges) * T + 8
        dst = np.full(room, 0xEE, np.uint8)
        doff, out = zsent(len(ranges) + 1), iarr(len(ranges))
        a = dict(container=buf.ctypes.data if buf is not None else None, offsets=zarr(off), chunk=intarr([r[0] for r in ranges]), start=intarr([r[1] for r in ranges]),
                 nitems=intarr([r[2] for r in ranges]), dest=dst.ctypes.data, dest_offsets_out=doff, result_out=out)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_getitem_packed(nchunks, a["container"], (buf.size if buf is not None else 0) if containersize is None else containersize, a["offsets"], nr,
                                            a["chunk"], a["start"], a["nitems"], a["dest"], room if destsize is None else destsize, a["dest_offsets_out"], a["result_out"], None)
        return dict(ret=r, results=_seen(out, I_SENT), offsets=_seen(doff, Z_SENT), touched=bool(np.any(dst != 0xEE)))

    # ---- include/blosc_gpu_checksum.h ----
    def checksum_batch(self, kind=1, n=3, null=(), ptrs=None, sizes=(10, 0, 20)):
        base = self.runs.ctypes.data
        dig = usent(max(n, 0))
        a = dict(src=parr([base, base + 10, base + 10] if ptrs is None else ptrs), nbytes=zarr(list(sizes)), digest_out=dig)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_checksum_batch(kind, n, a["src"], a["nbytes"], a["digest_out"], None)
        return dict(ret=r, results=_seen(dig, U_SENT))

    def checksum_packed(self, kind=1, n=3, null=(), offsets=(0, 10, 10, 30), length=None, containersize=None, container=True):
        dig = usent(max(n, 0))
        a = dict(container=self.runs.ctypes.data if container else None, offsets=zarr(list(offsets)), length=zarr(list(length)) if length is not None else None,
                 digest_out=dig)
        for name in null:
            a[name] = None
        r = self.L.blosc_gpu_checksum_packed(kind, n, a["container"], self.runs.size if containersize is None else containersize, a["offsets"], a["length"],
                                             a["digest_out"], None)
        return dict(ret=r, results=_seen(dig, U_SENT))


def row(pkg, **kw):
    a = dict(typesize=T, clevel=5, shuffle=1, cname=b"lz4", blocksize=BS, splitmode=0)
    a.update(kw)
    return pkg.cparams(**a)


def collect(L, pkgmod):
    """{case name: what the call answered}, in a fixed order.  The global compressor is LZ4 and the global block size 0 while this runs."""
    w = World(L, pkgmod)
    was = L.blosc_get_compressor(), L.blosc_get_blocksize()
    L.blosc_set_compressor(b"lz4"); L.blosc_set_blocksize(0)
    R = {}
    try:
        # ---- blosc_gpu_compress_batch[_host], blosc_gpu_decompress_batch[_host], the multi-GPU pair ----
        for host in (False, True):
            tag = "compress_batch_host" if host else "compress_batch"
            R[f"{tag}: valid"] = w.compress_batch(host)
            for n in (-1, 0):
                R[f"{tag}: n {n}"] = w.compress_batch(host, n=n)
            for name, cname in (("snappy (not built)", b"snappy"), ("unknown name", b"nosuch"), ("null name", None)):
                R[f"{tag}: {name}"] = w.compress_batch(host, cname=cname)
            R[f"{tag}: clevel 11"] = w.compress_batch(host, clevel=11)
            R[f"{tag}: destsize nbytes + 15"] = w.compress_batch(host, room=15)
            tag = "decompress_batch_host" if host else "decompress_batch"
            R[f"{tag}: valid"] = w.decompress_batch(host)
            for n in (-1, 0):
                R[f"{tag}: n {n}"] = w.decompress_batch(host, n=n)
            R[f"{tag}: srcsize null"] = w.decompress_batch(host, srcsize=False)
            R[f"{tag}: srcsize one short"] = w.decompress_batch(host, short=1)
        for compress in (True, False):
            tag = "compress_batch_multi" if compress else "decompress_batch_multi"
            R[f"{tag}: valid, devices null"] = w.multi(compress)
            R[f"{tag}: valid, device 0"] = w.multi(compress, devices=[0])
            for n in (-1, 0):
                R[f"{tag}: n {n}"] = w.multi(compress, n=n)
            for ndev in (0, -1, 65):
                R[f"{tag}: ndev {ndev}"] = w.multi(compress, ndev=ndev)
            R[f"{tag}: a device the node does not have"] = w.multi(compress, devices=[7])
            R[f"{tag}: n 0 before ndev 0"] = w.multi(compress, ndev=0, n=0)
        R["compress_batch_multi: snappy (not built)"] = w.multi(True, cname=b"snappy")
        R["compress_batch_multi: null name"] = w.multi(True, cname=None)

        # ---- blosc_gpu_packed_bound ----
        for n in (-1, 0):
            R[f"packed_bound: n {n}"] = w.bound(n=n)
        R["packed_bound: nbytes null"] = w.bound(nbytes=False)
        for align in (0, 1, 3, 16, 4096, 8192):
            R[f"packed_bound: align {align}"] = w.bound(align=align)

        # ---- blosc_gpu_compress_packed, blosc_gpu_compress_packed_params, blosc_gpu_compress_batch_params ----
        plain_rows = [row(pkgmod)] * 3
        edge_rows = {
            "compcode -1, 3, 6": [row(pkgmod, cname=None), row(pkgmod, cname=3), row(pkgmod, cname=6)],
            "compcode -2, 5, 1": [row(pkgmod, cname=-2), row(pkgmod, cname=5), row(pkgmod, cname=1)],
            "splitmode -1, 0, 5": [row(pkgmod, splitmode=-1), row(pkgmod, splitmode=0), row(pkgmod, splitmode=5)],
            "splitmode 1, 2, 4": [row(pkgmod, splitmode=1), row(pkgmod, splitmode=2), row(pkgmod, splitmode=4)],
            "clevel 11, -1, 0": [row(pkgmod, clevel=11), row(pkgmod, clevel=-1), row(pkgmod, clevel=0)],
            "shuffle 3, typesize 0, blocksize 0": [row(pkgmod, shuffle=3), row(pkgmod, typesize=0), row(pkgmod, blocksize=0)],
            "shuffle 0, 2, typesize 4": [row(pkgmod, shuffle=0), row(pkgmod, shuffle=2), row(pkgmod, typesize=4)],
        }
        for tag, rows in (("compress_packed", None), ("compress_packed_params", plain_rows)):
            R[f"{tag}: valid"] = w.compress_packed(rows)
            R[f"{tag}: n -1"] = w.compress_packed(rows, n=-1)
            R[f"{tag}: n -1, offsets_out null"] = w.compress_packed(rows, n=-1, null=("offsets_out",))
            R[f"{tag}: n 0"] = w.compress_packed(rows, n=0)
            R[f"{tag}: n 0, offsets_out null"] = w.compress_packed(rows, n=0, null=("offsets_out",))
            R[f"{tag}: n 0, everything else null"] = w.compress_packed(rows, n=0, null=("src", "nbytes", "dest", "cbytes_out") + (("params",) if rows else ()))
            for name in ("src", "nbytes", "offsets_out", "cbytes_out") + (("params",) if rows else ()):
                R[f"{tag}: {name} null"] = w.compress_packed(rows, n=2, null=(name,))
            R[f"{tag}: dest null, destsize 0 (the sizing call)"] = w.compress_packed(rows, n=2, null=("dest",))
            R[f"{tag}: dest null, a destsize (a size without a buffer)"] = w.compress_packed(rows, n=2, null=("dest",), destsize=4096)
            R[f"{tag}: a buffer, destsize 0"] = w.compress_packed(rows, n=2, destsize=0)
            for align in (0, 3, 16, 4096, 8192):
                R[f"{tag}: align {align}"] = w.compress_packed(rows, align=align)
            R[f"{tag}: align 3, n 0"] = w.compress_packed(rows, n=0, align=3)
        for name, cname in (("snappy (not built)", b"snappy"), ("unknown name", b"nosuch"), ("null name", None)):
            R[f"compress_packed: {name}"] = w.compress_packed(cname=cname)
        R["compress_packed: snappy, dest null"] = w.compress_packed(cname=b"snappy", null=("dest",))
        R["compress_packed: snappy, cbytes_out null"] = w.compress_packed(cname=b"snappy", null=("cbytes_out",))
        R["compress_packed: clevel 11"] = w.compress_packed(clevel=11)
        R["compress_batch_params: valid"] = w.compress_batch_params(plain_rows)
        for n in (-1, 0):
            R[f"compress_batch_params: n {n}"] = w.compress_batch_params(plain_rows, n=n)
        R["compress_batch_params: n 0, everything null"] = w.compress_batch_params(plain_rows, n=0, null=("params", "src", "nbytes", "dest", "destsize", "cbytes_out"))
        for name in ("params", "src", "nbytes", "dest", "destsize", "cbytes_out"):
            R[f"compress_batch_params: {name} null"] = w.compress_batch_params(plain_rows, n=2, null=(name,))
        for name, rows in edge_rows.items():
            R[f"compress_batch_params: {name}"] = w.compress_batch_params(rows)
            R[f"compress_packed_params: {name}"] = w.compress_packed(rows)

        # ---- blosc_gpu_decompress_packed, blosc_gpu_cbuffer_sizes_batch ----
        buf, off = w.container()
        gapped = w.container(gaps=(3, 0, 7))
        cases = {
            "valid": {}, "valid, junk between the chunks": dict(cont=gapped), "n -1": dict(n=-1), "n -1, dest_offsets_out null": dict(n=-1, null=("dest_offsets_out",)),
            "n 0": dict(n=0), "n 0, dest_offsets_out null": dict(n=0, null=("dest_offsets_out",)),
            "n 0, everything else null": dict(n=0, null=("container", "offsets", "dest", "nbytes_out")),
            "container null": dict(n=2, null=("container",)), "offsets null": dict(n=2, null=("offsets",)), "dest_offsets_out null": dict(n=2, null=("dest_offsets_out",)),
            "nbytes_out null": dict(n=2, null=("nbytes_out",)), "dest null, destsize 0 (the size query)": dict(n=2, null=("dest",), destsize=0),
            "dest null, a destsize (a size without a buffer)": dict(n=2, null=("dest",)), "a buffer, destsize 0": dict(n=2, destsize=0),
            "destsize one short": dict(destsize=sum(SIZES) - 1),
            "a table that falls": dict(cont=(buf, [off[0], off[2], off[1], off[3]])),
            "a table that falls at its end": dict(cont=(buf, [off[0], off[1], off[2], off[2] - 1])),
            "last offset beyond containersize": dict(containersize=buf.size - 1),
            "last offset is containersize": dict(cont=gapped, containersize=gapped[1][3]),
            "a span of 0 between two chunks": dict(cont=(buf, [off[0], off[1], off[1], off[2]])),
            "a span of 15 between two chunks": dict(cont=(w.container(gaps=(15, 0, 0))[0], [off[0], off[1], off[1] + 15, off[2] + 15])),
            "a span of 16 between two chunks": dict(cont=(w.container(gaps=(16, 0, 0))[0], [off[0], off[1], off[1] + 16, off[2] + 16])),
            "a span one short of its chunk": dict(n=2, cont=(buf, [off[0], off[1], off[2] - 1])),
            "an empty container with a null base": dict(n=2, cont=(None, [0, 0, 0])),
        }
        for name, kw in cases.items():
            R[f"decompress_packed: {name}"] = w.decompress_packed(**kw)
        other = w.chunks[1].copy(); other[0] = 9
        R["cbuffer_sizes_batch: valid"] = w.sizes_batch()
        R["cbuffer_sizes_batch: another format version"] = w.sizes_batch(chunks=[w.chunks[0], other, w.chunks[2]])
        for n in (-1, 0):
            R[f"cbuffer_sizes_batch: n {n}"] = w.sizes_batch(n=n)
        R["cbuffer_sizes_batch: n 0, src null"] = w.sizes_batch(n=0, null=("src",))
        for name in ("src", "nbytes", "cbytes", "blocksize"):
            R[f"cbuffer_sizes_batch: {name} null"] = w.sizes_batch(n=2, null=(name,))
        R["cbuffer_sizes_batch: every output null"] = w.sizes_batch(n=2, null=("nbytes", "cbytes", "blocksize"))

        # ---- blosc_gpu_getitem_batch, blosc_gpu_getitem_packed ----
        two = [(0, 0, 4), (1, 8, 4)]
        R["getitem_batch: valid"] = w.getitem_batch()
        R["getitem_batch: nchunks -1"] = w.getitem_batch(nchunks=-1)
        R["getitem_batch: nranges -1"] = w.getitem_batch(nranges=-1)
        R["getitem_batch: nranges 0"] = w.getitem_batch(nranges=0)
        R["getitem_batch: nranges 0, everything null"] = w.getitem_batch(nranges=0, null=("src", "chunk", "start", "nitems", "dest", "result_out"))
        R["getitem_batch: nchunks 0"] = w.getitem_batch(nchunks=0, ranges=two)
        R["getitem_batch: nchunks 0, src null"] = w.getitem_batch(nchunks=0, ranges=two, null=("src",))
        for name in ("src", "chunk", "start", "nitems", "dest", "result_out"):
            R[f"getitem_batch: {name} null"] = w.getitem_batch(nchunks=2, ranges=two, null=(name,))
        cases = {
            "valid": {}, "valid, junk between the chunks": dict(cont=gapped), "nchunks -1": dict(nchunks=-1), "nranges -1": dict(nranges=-1),
            "nranges -1, dest_offsets_out null": dict(nranges=-1, null=("dest_offsets_out",)), "nranges 0": dict(nranges=0),
            "nranges 0, dest_offsets_out null": dict(nranges=0, null=("dest_offsets_out",)),
            "nranges 0, everything else null": dict(nranges=0, null=("container", "offsets", "chunk", "start", "nitems", "dest", "result_out")),
            "nranges 0, a table that falls": dict(nranges=0, cont=(buf, [off[0], off[2], off[1], off[3]])),
            "nchunks 0": dict(nchunks=0, ranges=two), "nchunks 0, an empty container with a null base": dict(nchunks=0, ranges=two, cont=(None, [0])),
            "nchunks 0, offsets null": dict(nchunks=0, ranges=two, null=("offsets",)),
            "an empty container with a null base": dict(nchunks=2, ranges=two, cont=(None, [0, 0, 0])),
            "dest null, destsize 0 (the size query)": dict(null=("dest",), destsize=0), "dest null, a destsize (a size without a buffer)": dict(null=("dest",)),
            "a buffer, destsize 0": dict(destsize=0), "destsize one short": dict(destsize=sum(max(r[2], 0) for r in World.RANGES) * T - 1),
            "a table that falls": dict(cont=(buf, [off[0], off[2], off[1], off[3]])),
            "last offset beyond containersize": dict(containersize=buf.size - 1),
            "a span of 0 between two chunks": dict(cont=(buf, [off[0], off[1], off[1], off[2]])),
            "a span of 15 between two chunks": dict(cont=(w.container(gaps=(15, 0, 0))[0], [off[0], off[1], off[1] + 15, off[2] + 15])),
            "a span of 16 between two chunks": dict(cont=(w.container(gaps=(16, 0, 0))[0], [off[0], off[1], off[1] + 16, off[2] + 16])),
            "a span one short of its chunk": dict(nchunks=2, ranges=two, cont=(buf, [off[0], off[1], off[2] - 1])),
        }
        for name in ("container", "offsets", "chunk", "start", "nitems", "dest_offsets_out", "result_out"):
            cases[f"{name} null"] = dict(nchunks=2, ranges=two, null=(name,))
        for name, kw in cases.items():
            R[f"getitem_packed: {name}"] = w.getitem_packed(**kw)

        # ---- blosc_gpu_checksum_batch, blosc_gpu_checksum_packed ----
        base = w.runs.ctypes.data
        for kind in (1, 2):
            R[f"checksum_batch: kind {kind}"] = w.checksum_batch(kind)
            R[f"checksum_packed: kind {kind}, spans of 10, 0 and 20"] = w.checksum_packed(kind)
            R[f"checksum_packed: kind {kind}, spans of 0 and 15"] = w.checksum_packed(kind, offsets=(5, 5, 20, 64))
            R[f"checksum_packed: kind {kind}, lengths"] = w.checksum_packed(kind, length=(10, 0, 7))
        for kind in (0, 3, -1):
            R[f"checksum_batch: kind {kind}"] = w.checksum_batch(kind)
            R[f"checksum_batch: kind {kind}, n 0"] = w.checksum_batch(kind, n=0)                  # kind is checked first
            R[f"checksum_batch: kind {kind}, n -1"] = w.checksum_batch(kind, n=-1)
            R[f"checksum_packed: kind {kind}"] = w.checksum_packed(kind)
            R[f"checksum_packed: kind {kind}, n 0"] = w.checksum_packed(kind, n=0)
            R[f"checksum_packed: kind {kind}, n -1"] = w.checksum_packed(kind, n=-1)
        for n in (-1, 0):
            R[f"checksum_batch: n {n}"] = w.checksum_batch(n=n)
            R[f"checksum_packed: n {n}"] = w.checksum_packed(n=n)
        R["checksum_batch: n 0, everything null"] = w.checksum_batch(n=0, null=("src", "nbytes", "digest_out"))
        R["checksum_packed: n 0, everything null"] = w.checksum_packed(n=0, null=("container", "offsets", "length", "digest_out"))
        for name in ("src", "nbytes", "digest_out"):
            R[f"checksum_batch: {name} null"] = w.checksum_batch(n=2, null=(name,))
        R["checksum_batch: an empty run with a null pointer"] = w.checksum_batch(ptrs=[base, None, base + 10])
        R["checksum_batch: a run with a null pointer"] = w.checksum_batch(ptrs=[base, base, None])
        R["checksum_batch: a run beyond INT32_MAX + 16, pointer null"] = w.checksum_batch(ptrs=[base, None, base], sizes=(10, HUGE, 20))
        R["checksum_batch: a run of INT32_MAX + 16, pointer null"] = w.checksum_batch(ptrs=[base, None, base], sizes=(10, HUGE - 1, 20))
        for name in ("container", "offsets", "digest_out"):
            R[f"checksum_packed: {name} null"] = w.checksum_packed(n=2, null=(name,), offsets=(0, 10, 30))
        R["checksum_packed: a table that falls"] = w.checksum_packed(offsets=(0, 10, 9, 30))
        R["checksum_packed: last offset beyond containersize"] = w.checksum_packed(containersize=29)
        R["checksum_packed: last offset is containersize"] = w.checksum_packed(containersize=30)
        R["checksum_packed: a length beyond its span"] = w.checksum_packed(length=(10, 1, 20))
        R["checksum_packed: a length beyond its span, table falls too"] = w.checksum_packed(offsets=(0, 10, 9, 30), length=(11, 0, 0))
        R["checksum_packed: an empty container with a null base"] = w.checksum_packed(n=2, container=False, containersize=0, offsets=(0, 0, 0))
        R["checksum_packed: empty runs in a null base of some size"] = w.checksum_packed(n=2, container=False, containersize=64, offsets=(7, 7, 7))
        R["checksum_packed: zero lengths in a null base"] = w.checksum_packed(n=2, container=False, containersize=64, offsets=(0, 10, 30), length=(0, 0))
        R["checksum_packed: a run beyond INT32_MAX + 16, base null"] = w.checksum_packed(n=1, container=False, containersize=HUGE, offsets=(0, HUGE))
        R["checksum_packed: a length beyond INT32_MAX + 16, base null"] = w.checksum_packed(n=1, container=False, containersize=HUGE + 5, offsets=(0, HUGE + 5), length=(HUGE,))
    finally:
        L.blosc_set_compressor(was[0]); L.blosc_set_blocksize(was[1])
    return R


BLPK_INPUTS = {"empty": (0, 4096), "one chunk": (3000, 4096), "five chunks, a short last one": (4 * 2048 + 1000, 2048)}      # (bytes, chunk_size)


def collect_blpk(L, pkgmod, blpk):
    """sha256 of the file blpk.pack writes (random bytes: stored chunks), and whether pack_device wrote the same file"""
    pkgmod.declare_packed(L); pkgmod.declare_checksum(L)
    L.blosc_gpu_compress_batch_host.argtypes = [ci, ci, sz, C.c_char_p, sz, ci, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz), C.POINTER(ci)]
    L.blosc_set_blocksize.argtypes = [sz]
    L.blosc_set_blocksize.restype = None
    was = L.blosc_get_blocksize()
    L.blosc_set_blocksize(0)
    R = {}
    try:
        for name, (n, chunk_size) in BLPK_INPUTS.items():
            data = DATASETS["random"](n)
            for checksum in (0, 1):
                a, b = io.BytesIO(), io.BytesIO()
                ra = blpk.pack(L, data, a, chunk_size=chunk_size, typesize=T, cname=b"lz4", checksum=checksum)
                rb = blpk.pack_device(L, data.ctypes.data, n, b, chunk_size=chunk_size, typesize=T, cname=b"lz4", checksum=checksum, mem=NumpyMem())
                R[f"{name}, checksum {checksum}"] = dict(nchunks=ra[0], written=ra[1], sha256=hashlib.sha256(a.getvalue()).hexdigest(),
                                                         pack_device_writes_the_same=(rb == ra and b.getvalue() == a.getvalue()))
    finally:
        L.blosc_set_blocksize(was)
    return R


def collect_all(L):
    pkgmod = _module("c_blosc_amd_for_abi", "c-blosc_amd", "__init__.py")
    blpk = _module("blpk_for_abi", "c-blosc_amd", "blpk.py")
    return json.loads(json.dumps({"calls": collect(L, pkgmod), "blpk": collect_blpk(L, pkgmod, blpk)}))      # (through JSON: tuples become lists)


def test_every_batch_entry_point_answers_as_recorded(emulib):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    got = collect_all(emulib)
    assert list(got["calls"]) == list(want["calls"]) and list(got["blpk"]) == list(want["blpk"]), "the list of cases changed: regenerate on purpose only"
    wrong = {k: (got[part][k], want[part][k]) for part in ("calls", "blpk") for k in want[part] if got[part][k] != want[part][k]}
    assert not wrong, f"{len(wrong)} answers changed (got, recorded): {wrong}"
    entry_points = {k.split(":")[0] for k in want["calls"]}
    assert entry_points == {"compress_batch", "compress_batch_host", "decompress_batch", "decompress_batch_host", "compress_batch_multi", "decompress_batch_multi",
                            "packed_bound", "compress_packed", "decompress_packed", "cbuffer_sizes_batch", "compress_batch_params", "compress_packed_params",
                            "getitem_batch", "getitem_packed", "checksum_batch", "checksum_packed"}
    assert all(v["pack_device_writes_the_same"] for v in want["blpk"].values())
