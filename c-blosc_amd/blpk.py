"""blpk.py — a many-chunk container in Bloscpack's file layout, streamed through the BATCHED GPU calls.

c-blosc compresses one buffer of at most 2 GiB per call; files are handled by callers such as Bloscpack (`README.md:173-177`
of the reference points there), which cut the data into chunks, run `blosc_compress` on each and store the chunks behind a
small header with an offset table.  This module is that caller for libblosc_amd: the chunks of a file go through
`blosc_gpu_compress_batch_host` / `blosc_gpu_decompress_batch_host` several hundred at a time instead of one call per chunk, so a file
is a handful of launches.

File layout (Bloscpack format version 3, written from its published format description; **parity unpinned**: Bloscpack is
a separate project, neither in the reference tree nor in this image, so no byte-for-byte comparison with its own files was
possible - what IS pinned: every chunk inside is an ordinary c-blosc chunk, read by the reference and the oracle in the tests):

    bytes 0-3   magic "blpk"          4  format version (3)        5  options (bit 0: offsets, bit 1: metadata)
    6  checksum (0 none, 1 adler32, 2 crc32)      7  typesize      8-11  chunk_size (int32)    12-15  last_chunk (int32)
    16-23  nchunks (int64)            24-31  max_app_chunks (int64)
    [offsets: (nchunks + max_app_chunks) x int64, from the start of the file, -1 = unused]
    chunk 0 [+ 4-byte checksum of the compressed chunk, little endian], chunk 1 ...

`pack_device` / `unpack_device` are the same file from and to DEVICE memory: the plain data never crosses to the host.  A batch is
compressed into one packed container (include/blosc_gpu_packed.h), its chunks are digested where they lie
(include/blosc_gpu_checksum.h), and only the compressed bytes come down, in one copy; the reader uploads the file image once,
verifies the digests on the device and decodes the image as a packed container straight into the caller's buffer.

Only what the path needs: no metadata section is written (a file that has one is read past it), checksums none / adler32 /
crc32.  There is no CPU implementation here: without the library and a GPU the calls fail.
"""
import ctypes as C
import os
import struct
import zlib

import numpy as np

MAGIC = b"blpk"
FORMAT_VERSION = 3
HEADER_LENGTH = 32
METADATA_HEADER_LENGTH = 32
CHECKSUMS = ("None", "adler32", "crc32")
_OPT_OFFSETS, _OPT_METADATA = 1, 2


class BlpkError(ValueError):
    pass


def _digest(kind, data):
    if kind == 1:
        return struct.pack("<I", zlib.adler32(data) & 0xffffffff)
    if kind == 2:
        return struct.pack("<I", zlib.crc32(data) & 0xffffffff)
    return b""


def pack_header(nchunks, chunk_size, last_chunk, typesize, checksum=1, offsets=True, max_app_chunks=0):
    if not 0 <= checksum < len(CHECKSUMS):
        raise BlpkError("unknown checksum")
    return MAGIC + struct.pack("<BBBBiiqq", FORMAT_VERSION, _OPT_OFFSETS if offsets else 0, checksum, typesize & 0xff,
                               chunk_size, last_chunk, nchunks, max_app_chunks)


def unpack_header(buf):
    if len(buf) < HEADER_LENGTH:
        raise BlpkError("file shorter than a bloscpack header")
    if buf[:4] != MAGIC:
        raise BlpkError("not a bloscpack file (magic)")
    version, options, checksum, typesize, chunk_size, last_chunk, nchunks, max_app = struct.unpack("<BBBBiiqq", buf[4:HEADER_LENGTH])
    if version != FORMAT_VERSION:
        raise BlpkError(f"format version {version} (this reader knows {FORMAT_VERSION})")
    if checksum >= len(CHECKSUMS):
        raise BlpkError(f"checksum kind {checksum} not supported")
    if nchunks < 0 or max_app < 0 or chunk_size == 0:
        raise BlpkError("header needs nchunks and chunk_size")
    return dict(options=options, checksum=checksum, typesize=typesize, chunk_size=chunk_size, last_chunk=last_chunk,
                nchunks=nchunks, max_app_chunks=max_app, offsets=bool(options & _OPT_OFFSETS), metadata=bool(options & _OPT_METADATA))


def _ptr_array(arrs):
    return (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])


def _failed(what, rc, res):
    return BlpkError(f"{what} failed (rc {rc}, results {list(res)[:4]}...)")


class _Writer:
    """The file of `pack` and `pack_device`: the header and a placeholder offset table at once, then chunk() for every chunk in order
    (its bytes, its digest - empty for checksum 0), then close(), which writes the table back and returns (nchunks, bytes written).
    batches() cuts the `n` plain bytes into the calls' batches: (index of the first chunk, the plain sizes of its chunks)."""

    def __init__(self, fh, n, chunk_size, typesize, checksum, batch_bytes):
        if chunk_size <= 0 or chunk_size > (1 << 31) - 17:
            raise BlpkError("chunk_size out of range")
        self.fh, self.n, self.chunk_size = fh, n, chunk_size
        self.nchunks = (n + chunk_size - 1) // chunk_size if n else 0
        self.per_batch = max(1, batch_bytes // chunk_size)
        header = pack_header(self.nchunks, chunk_size, n - (self.nchunks - 1) * chunk_size if self.nchunks else 0, typesize, checksum)
        self.start = fh.tell()
        fh.write(header)
        self.offsets, self.written = np.full(self.nchunks, -1, "<i8"), 0
        fh.write(self.offsets.tobytes())

    def batches(self):
        for b0 in range(0, self.nchunks, self.per_batch):
            yield b0, [min(self.n, (k + 1) * self.chunk_size) - k * self.chunk_size for k in range(b0, min(self.nchunks, b0 + self.per_batch))]

    def chunk(self, data, digest):
        self.offsets[self.written] = self.fh.tell() - self.start
        self.written += 1
        self.fh.write(data); self.fh.write(digest)

    def close(self):
        end = self.fh.tell()
        self.fh.seek(self.start + HEADER_LENGTH); self.fh.write(self.offsets.tobytes()); self.fh.seek(end)
        return self.nchunks, end - self.start


_META_DIGEST_LENGTH = {0: 0, 1: 4, 2: 4, 3: 16, 4: 20, 5: 28, 6: 32, 7: 48, 8: 64}      # metadata section: checksum kind -> bytes of its digest


def _read_layout(raw):
    """Where the chunks of the file image `raw` lie: (header dict, offsets, plain sizes, compressed sizes, bytes of a chunk's digest), one
    list entry per chunk.  A metadata section is skipped; without an offset table the chunks are found one behind the other.  Every chunk's
    16-byte header and, with its digest, its compressed bytes lie inside the image; nothing else is promised about the offsets."""
    h = unpack_header(raw)
    pos = HEADER_LENGTH
    if h["metadata"]:                                  # skip: magic_format(8) options checksum codec level meta_size max_meta_size meta_comp_size user_codec(8)
        if len(raw) < pos + METADATA_HEADER_LENGTH:
            raise BlpkError("truncated metadata header")
        max_meta = struct.unpack_from("<I", raw, pos + 16)[0]
        dlen = _META_DIGEST_LENGTH.get(raw[pos + 9])
        if dlen is None:
            raise BlpkError("metadata checksum kind")
        pos += METADATA_HEADER_LENGTH + max_meta + dlen
    nch = h["nchunks"]
    dlen = 4 if h["checksum"] else 0
    table = None
    if h["offsets"]:
        tot = nch + h["max_app_chunks"]
        if len(raw) < pos + 8 * tot:
            raise BlpkError("truncated offset table")
        table = np.frombuffer(raw, "<i8", tot, pos)[:nch]
        pos += 8 * tot
    offs, sizes, cbytes = [], [], []
    for k in range(nch):
        o = int(table[k]) if table is not None else pos
        if o < 0 or o + 16 > len(raw):
            raise BlpkError(f"chunk {k}: offset outside the file")
        nb, _bs, cb = struct.unpack_from("<iii", raw, o + 4)
        if cb < 16 or o + cb + dlen > len(raw) or nb < 0:
            raise BlpkError(f"chunk {k}: header sizes outside the file")
        offs.append(o); sizes.append(nb); cbytes.append(cb)
        pos = o + cb + dlen
    return h, offs, sizes, cbytes, dlen


def pack(lib, data, fh, chunk_size=1 << 20, typesize=8, clevel=5, shuffle=1, cname=b"lz4", checksum=1, batch_bytes=1 << 30):
    """Compress `data` (numpy, any dtype) into the open binary file `fh`.  Chunks go to the GPU `batch_bytes` at a time
    through blosc_gpu_compress_batch_host.  Returns (nchunks, bytes written)."""
    a = np.ascontiguousarray(data).view(np.uint8).ravel()
    w = _Writer(fh, a.size, chunk_size, typesize, checksum, batch_bytes)
    for b0, sizes in w.batches():
        m = len(sizes)
        srcs = [a[(b0 + k) * chunk_size:(b0 + k) * chunk_size + s] for k, s in enumerate(sizes)]
        dsts = [np.empty(s + 16, np.uint8) for s in sizes]
        res = (C.c_int * m)()
        rc = lib.blosc_gpu_compress_batch_host(clevel, shuffle, typesize, cname, 0, m, _ptr_array(srcs), (C.c_size_t * m)(*sizes), _ptr_array(dsts),
                                               (C.c_size_t * m)(*[d.size for d in dsts]), res)
        if rc != 0 or any(r <= 0 for r in res):
            raise _failed("compression", rc, res)
        for d, r in zip(dsts, res):
            chunk = d[:r].tobytes()
            w.chunk(chunk, _digest(checksum, chunk))
    return w.close()


def unpack(lib, fh, batch_bytes=1 << 30, verify=True):
    """Read a bloscpack file from the open binary file `fh`; returns the plain bytes as a numpy uint8 array.  Chunks go to the
    GPU `batch_bytes` at a time through blosc_gpu_decompress_batch_host."""
    blob = fh.read()
    h, offs, sizes, cbytes, dlen = _read_layout(blob)
    nch = len(offs)
    chunks = [np.frombuffer(blob, np.uint8, cb, o) for o, cb in zip(offs, cbytes)]
    for k, (c, o) in enumerate(zip(chunks, offs)):
        if verify and dlen and _digest(h["checksum"], c.tobytes()) != blob[o + c.size:o + c.size + dlen]:
            raise BlpkError(f"chunk {k}: checksum mismatch")
    total = int(sum(sizes))
    out = np.empty(total, np.uint8)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    k0 = 0
    while k0 < nch:
        k1 = k0; acc = 0
        while k1 < nch and (k1 == k0 or acc + sizes[k1] <= batch_bytes):
            acc += sizes[k1]; k1 += 1
        m = k1 - k0
        srcs = [np.ascontiguousarray(chunks[k]) for k in range(k0, k1)]
        dsts = [out[starts[k]:starts[k + 1]] for k in range(k0, k1)]
        ssz = (C.c_size_t * m)(*[s.size for s in srcs]); dsz = (C.c_size_t * m)(*[d.size for d in dsts])
        res = (C.c_int * m)()
        rc = lib.blosc_gpu_decompress_batch_host(m, _ptr_array(srcs), ssz, _ptr_array(dsts), dsz, res)
        if rc != 0 or any(r != d.size for r, d in zip(res, dsts)):
            raise _failed("decompression", rc, res)
        k0 = k1
    return out


# ---- files from and to device memory ---------------------------------------------------------------------------------------------
class TorchMem:
    """Device memory and copies for pack_device / unpack_device out of torch (uint8 tensors on the current device).
    alloc(n) -> (ptr, keepalive); to_host(ptr, n) -> numpy uint8 (ptr inside a buffer of alloc / to_device that is still alive);
    to_device(numpy uint8) -> (ptr, keepalive).  Anything with these three methods serves (the CPU tests pass a numpy-backed one:
    on the emulated library "device memory" is host memory)."""

    def __init__(self):
        import torch                                     # lazily: this module imports without it
        import weakref
        self.torch = torch
        self.live = weakref.WeakSet()

    def alloc(self, n):
        t = self.torch.empty(max(int(n), 1), dtype=self.torch.uint8, device="cuda")
        self.live.add(t)
        return t.data_ptr(), t

    def to_host(self, ptr, n):
        for t in self.live:
            base = t.data_ptr()
            if base <= ptr and ptr + n <= base + t.numel():
                return t[ptr - base:ptr - base + n].cpu().numpy()
        raise BlpkError("to_host: not inside a buffer this object handed out")

    def to_device(self, arr):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")              # a file image is a read-only array; it is only read
            t = self.torch.from_numpy(arr).to("cuda")
        self.live.add(t)
        return t.data_ptr(), t


def pack_device(lib, src_ptr, nbytes, fh, chunk_size=1 << 20, typesize=8, clevel=5, shuffle=1, cname=b"lz4", checksum=1,
                batch_bytes=1 << 30, mem=None):
    """Compress the `nbytes` bytes at the DEVICE pointer `src_ptr` into the open binary file `fh`: the file `pack` writes for the same
    bytes and settings.  Per `batch_bytes` of source: blosc_gpu_compress_packed (align 1) into one device container,
    blosc_gpu_checksum_packed over its chunks, ONE device-to-host copy of the used bytes, and the chunks and digests written from that
    buffer.  Returns (nchunks, bytes written)."""
    w = _Writer(fh, int(nbytes), chunk_size, typesize, checksum, batch_bytes)
    mem = mem if mem is not None else TorchMem()
    cont = keep = None; room = 0
    for b0, sizes in w.batches():
        m = len(sizes)
        ssz = (C.c_size_t * m)(*sizes)
        bound = lib.blosc_gpu_packed_bound(m, ssz, 1)
        if cont is None or bound > room:
            keep = None                                  # (the first batch is the largest: this runs once)
            cont, keep = mem.alloc(bound); room = bound
        off = (C.c_size_t * (m + 1))(); res = (C.c_int * m)()
        srcs = (C.c_void_p * m)(*[src_ptr + k * chunk_size for k in range(b0, b0 + m)])
        rc = lib.blosc_gpu_compress_packed(clevel, shuffle, typesize, cname, 0, m, srcs, ssz, cont, room, 1, off, res, None)
        if rc != 0 or any(r <= 0 for r in res):
            raise _failed("compression", rc, res)
        dig = (C.c_uint * m)()
        if checksum:
            rc = lib.blosc_gpu_checksum_packed(checksum, m, cont, room, off, (C.c_size_t * m)(*res), dig, None)
            if rc != 0:
                raise BlpkError(f"checksums failed (rc {rc})")
        used = int(off[m])
        body = memoryview(np.ascontiguousarray(mem.to_host(cont, used)))
        digests = memoryview(np.asarray(dig, dtype="<u4").view(np.uint8))
        for k in range(m):
            w.chunk(body[off[k]:off[k] + res[k]], digests[4 * k:4 * k + 4] if checksum else b"")
    return w.close()


def unpack_device(lib, fh, dest_ptr=None, destsize=0, verify=True, mem=None):
    """Read a bloscpack file from the open binary file `fh` into the `destsize` bytes of DEVICE memory at `dest_ptr`; returns the plain
    size (dest_ptr None: the size query, nothing is uploaded or decoded).  The file image is uploaded once; blosc_gpu_checksum_packed
    digests the chunks in it, the digests are compared with the stored ones on the host, and blosc_gpu_decompress_packed decodes the same
    image - a chunk's span to the next one is its bytes plus the digest, which that call takes as padding.  Header, table and chunk
    headers get `unpack`'s checks.  A file without an offset table, or whose table does not rise strictly, is `unpack`'s."""
    raw = fh.read()
    h, offs, sizes, cbytes, dlen = _read_layout(raw)
    nch = len(offs)
    # what this path refuses on top: the image is decoded as ONE packed container, whose table rises and whose chunks do not overlap
    if not h["offsets"]:
        raise BlpkError("no offset table: not a file for unpack_device, use unpack")
    for k in range(1, nch):
        if offs[k] <= offs[k - 1]:
            raise BlpkError(f"chunk {k}: the offset table does not rise: not a file for unpack_device, use unpack")
        if offs[k - 1] + cbytes[k - 1] + dlen > offs[k]:
            raise BlpkError(f"chunk {k - 1}: runs into chunk {k}")
    total = int(sum(sizes))
    if dest_ptr is None:
        return total
    if total > destsize:
        raise BlpkError(f"destination of {destsize} bytes for {total}")
    if nch == 0:
        return 0
    mem = mem if mem is not None else TorchMem()
    image, keep = mem.to_device(np.frombuffer(raw, np.uint8))
    table = (C.c_size_t * (nch + 1))(*offs, offs[-1] + cbytes[-1] + dlen)
    if verify and dlen:
        dig = (C.c_uint * nch)()
        rc = lib.blosc_gpu_checksum_packed(h["checksum"], nch, image, len(raw), table, (C.c_size_t * nch)(*cbytes), dig, None)
        if rc != 0:
            raise BlpkError(f"checksums failed (rc {rc})")
        for k in range(nch):
            if dig[k] != struct.unpack_from("<I", raw, offs[k] + cbytes[k])[0]:
                raise BlpkError(f"chunk {k}: checksum mismatch")
    doff = (C.c_size_t * (nch + 1))(); res = (C.c_int * nch)()
    rc = lib.blosc_gpu_decompress_packed(nch, image, len(raw), table, dest_ptr, destsize, doff, res, None)
    if rc != 0 or any(r != s for r, s in zip(res, sizes)):
        raise _failed("decompression", rc, res)
    del keep
    return total


def pack_file(lib, src_path, dst_path, **kw):
    data = np.fromfile(src_path, np.uint8)
    with open(dst_path, "wb") as fh:
        return pack(lib, data, fh, **kw)


def unpack_file(lib, src_path, dst_path=None, **kw):
    with open(src_path, "rb") as fh:
        out = unpack(lib, fh, **kw)
    if dst_path is not None:
        out.tofile(dst_path)
    return out
