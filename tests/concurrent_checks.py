"""What tests/test_gpu_concurrent_calls.py (device) and tests/test_emu_concurrent_calls.py (wavefront emulator) share: one worker per call
family of the device ABI, a proxy around the ctypes handle that records when every exported call ran, and a runner that releases threads
round by round.

A worker builds its inputs once and holds what it expects before any thread starts; the expectation is that of the family's own checker
(take_checks, put_checks, where_checks, aggregate_checks, params_checks, select_checks, getitem_ranges_checks, checksum_checks, packed_checks):
the oracle's plaintext, numpy, zlib's digests, the chunks of the existing calls - never the call under test.  On top of that a worker
records, per case, what its first call gave - a serial call, made before the threads exist - and every later repetition of that case must
give the same bytes for everything the headers call deterministic: the scheduling of another caller must change nothing.

The runner never touches a process-wide knob (the pass bound, the profile switch, the split mode, the environment) while threads run: a knob
is set before the first barrier and put back after the joins."""
import struct
import threading
import time
from contextlib import contextmanager

import numpy as np

import aggregate_checks as ag
import checksum_checks as cs
import params_checks as pc
import select_checks as sc
import where_checks as wh
from batch_bounds_checks import DETERMINISTIC, mixed_hosts
from getitem_ranges_checks import BLOCKSIZE, SENTINEL, SMALL, check_batch, chunk_ranges, expected, plain, prefix
from helpers import DATASETS, header, orc_compress, orc_decompress, ptr, ref_compress
from packed_checks import FILL, GUARD, check_chunks_decode, host_offsets
from put_checks import check_put
from take_checks import TakeSource, batch_chunks, check_take, index_sets, pack_container, plaintext

JOIN_TIMEOUT = 120.0      # seconds a thread may take over all its rounds before the test gives up on it
NO_CONTEXT = ("blosc_gpu_packed_bound", "blosc_set_", "blosc_amd_", "blosc_cbuffer_")      # exported calls that take no context: not logged


# ---- the recording proxy ----
class _Recorded:
    """one exported function: calls go through, (thread, entry point, t0, t1) goes into the log; argtypes / restype reach the real function"""
    def __init__(self, rec, name, fn):
        self.__dict__.update(_rec=rec, _name=name, _fn=fn)

    def __call__(self, *args):
        who = threading.current_thread().name
        t0 = time.monotonic()
        self._rec.last[who] = (self._name, t0)
        try:
            return self._fn(*args)
        finally:
            self._rec.log.append((who, self._name, t0, time.monotonic()))

    def __getattr__(self, key):
        return getattr(self._fn, key)

    def __setattr__(self, key, value):
        setattr(self._fn, key, value)


class Recorder:
    """stands in for the ctypes handle wherever the package's wrappers and the checkers take `lib=`"""
    def __init__(self, lib):
        self.__dict__.update(_lib=lib, log=[], last={})

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("blosc_") or not callable(fn) or name.startswith(NO_CONTEXT):
            return fn
        self.__dict__[name] = _Recorded(self, name, fn)
        return self.__dict__[name]


def overlapping_pairs(entries):
    """(number of pairs of calls of different threads whose intervals overlap, the entry points of those pairs)"""
    entries = sorted(entries, key=lambda e: e[2])
    pairs, names = 0, set()
    for i, (who, name, t0, t1) in enumerate(entries):
        for other, oname, o0, o1 in entries[i + 1:]:
            if o0 >= t1:
                break
            if other != who:
                pairs += 1
                names.update((name, oname))
    return pairs, names


class Overlap:
    """what really ran side by side in one run_threads: per round the overlapping pairs, over the run the entry points that took part"""
    def __init__(self, log, marks):
        self.rounds = [overlapping_pairs(log[a:b]) for a, b in zip(marks[:-1], marks[1:])]
        self.pairs = sum(p for p, _ in self.rounds)
        self.names = set().union(*[n for _, n in self.rounds]) if self.rounds else set()
        self.calls = marks[-1] - marks[0]

    def rounds_with_overlap(self):
        return sum(1 for p, _ in self.rounds if p)

    def __repr__(self):
        return (f"{self.calls} calls, {self.pairs} overlapping pairs, per round {[p for p, _ in self.rounds]}, "
                f"{len(self.names)} entry points overlapped: {sorted(self.names)}")


# ---- the environment of the workers ----
class Env:
    """pkg (the loader module), lib (a Recorder), mem, oracle, ref, and writer(cname, T, shuffle, turn) -> write(k, data): chunk k by the oracle
    (LZ4, BloscLZ), by the reference where it is built, by the library's stock blosc_compress_ctx on host buffers, in turns"""
    def __init__(self, pkg, lib, mem, oracle, ref):
        self.pkg, self.lib, self.mem, self.oracle, self.ref = pkg, lib, mem, oracle, ref
        pkg.declare(lib._lib)
        # The global split mode has no getter and an earlier test may have left it anywhere (tests/test_gpu_compress.py leaves NEVER, in this
        # library and in the reference alike, and later tests compare the two); the single-parameter calls and every parameter row with
        # splitmode 0 read it, and params_checks.Calls sets the library's default.  So it is set to that default here, before the first serial
        # answer - between a serial answer and its repetitions nothing moves it - and close() puts back what was found
        self.split_mode_found = self.split_mode()
        lib._lib.blosc_set_splitmode(pc.FORWARD_COMPAT_SPLIT)

    def split_mode(self):
        """the global split mode, read off the headers of three small chunks (include/blosc.h, blosc.c:929-959): Zstd is split under ALWAYS
        alone, LZ4 under ALWAYS and FORWARD_COMPAT, BloscLZ under every mode but NEVER"""
        data = plain(4096)
        split = lambda cname: not self.lib_chunk(data, 8, 1, cname)[2] & 0x10
        return 1 if split("zstd") else pc.FORWARD_COMPAT_SPLIT if split("lz4") else 3 if split("blosclz") else pc.NEVER_SPLIT

    def close(self):
        self.lib._lib.blosc_set_splitmode(self.split_mode_found)

    def lib_chunk(self, data, T, shuffle, cname, clevel=5):
        out = np.zeros(data.size + 16, np.uint8)
        r = self.lib._lib.blosc_compress_ctx(clevel, shuffle, T, data.size, ptr(data), ptr(out), out.size, cname.encode(), BLOCKSIZE, 1)
        assert r > 0, (cname, r)
        return out[:r].copy()

    def writer(self, cname, T, shuffle, turn):
        def write(k, data):
            who = (k + turn) % 3
            if who == 0 and cname in ("lz4", "blosclz"): return orc_compress(self.oracle, data, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1]
            if who != 2 and self.ref is not None: return ref_compress(self.ref, data, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1]
            return self.lib_chunk(data, T, shuffle, cname)
        return write


def first_difference(a, b):
    a, b = np.ascontiguousarray(a).view(np.uint8).ravel(), np.ascontiguousarray(b).view(np.uint8).ravel()
    if a.size != b.size:
        return f"{a.size} bytes for {b.size}"
    bad = np.flatnonzero(a != b)
    return f"{bad.size} bytes differ, first at byte {int(bad[0])}: {int(a[bad[0]])} for {int(b[bad[0]])}"


class Worker:
    """A call family.  cases(): every case's name; run(case, stream) -> {output name: array}, checked in full against the expectation on the
    way; turn(r) -> the cases of round r.  first[case] holds the serial answer"""
    entry_points = ()

    def __init__(self):
        self.first = {}

    def turn(self, r):
        return [self.cases()[r % len(self.cases())]]

    def serial(self):
        for case in self.cases():
            self.first[case] = self.run(case, None)
        return self

    def repeat(self, case, stream, who):
        got = self.run(case, stream)
        want = self.first[case]
        assert got.keys() == want.keys(), (who, case, sorted(got), sorted(want))
        for key in want:
            if got[key] is None and want[key] is None:
                continue
            if not np.array_equal(got[key], want[key]):
                raise AssertionError((who, self.entry_of(case), case, key, "differs from the serial call", first_difference(got[key], want[key])))

    def entry_of(self, case):
        """the entry points a case goes through, for the messages"""
        return type(self).__name__, self.entry_points


def swing(r, n):
    """0 .. n - 1 and back: with the entry point alternating by round, every table meets both"""
    return r % n if (r // n) % 2 == 0 else (n - 1 - r) % n


def resized(chunks, nchunks, extra):
    """the chunks of a call cut or extended to nchunks; extra(k) -> one more chunk"""
    if nchunks is None:
        return chunks
    return chunks[:nchunks] + [extra(k) for k in range(len(chunks), nchunks)]


def both_sources(mem, chunks, align=256):
    return {"batch": TakeSource(mem, chunks=chunks), "packed": TakeSource(mem, *(None,) + pack_container(chunks, align))}


# ---- take and put ----
class RowTable:
    """one table of take / put: (codec, typesize, filter), row size, number of chunks (None: batch_chunks' own)"""
    def __init__(self, env, setting, row_bytes, nchunks=None, turn=0, random_rows=3000):
        cname, T, shuffle = setting
        self.setting, self.row_bytes = setting, row_bytes
        scale = 1 if T == 17 else 8      # (the blocks of a split typesize are widened to 64 KiB)
        write = env.writer(cname, T, shuffle, turn)
        self.chunks = resized(batch_chunks(env.oracle, write, row_bytes, scale), nchunks,
                              lambda k: write(k, plain(row_bytes * (1500 // row_bytes + 7 * k), seed=40 + k + turn)))
        assert all(header(c)["nbytes"] % row_bytes == 0 for c in self.chunks)
        self.rows_plain = plaintext(env.oracle, self.chunks)
        sets = index_sets(self.chunks, row_bytes, seed=5 + turn)
        self.index = np.concatenate([sets["edges"], sets["out of bounds"], sets["random"][:random_rows]])
        self.sources = both_sources(env.mem, self.chunks)
        self.params = [env.pkg.cparams(T, 5, shuffle, cname.encode(), BLOCKSIZE) for _ in self.chunks]
        self.name = f"{cname}-T{T}-shuffle{shuffle}-rows-of-{row_bytes}-{len(self.chunks)}-chunks"


class RowWorker(Worker):
    def __init__(self, env, tables, variants=("batch", "packed")):
        super().__init__()
        self.env, self.tables, self.variants = env, tables, variants

    def cases(self):
        return [(t, v) for t in range(len(self.tables)) for v in self.variants]

    def turn(self, r):
        return [(swing(r, len(self.tables)), self.variants[r % len(self.variants)])]

    def entry_of(self, case):
        return type(self).__name__, self.entry_points[("batch", "packed").index(case[1])]


class TakeWorker(RowWorker):
    entry_points = ("blosc_gpu_take_batch", "blosc_gpu_take_packed")

    def run(self, case, stream):
        e, t = self.env, self.tables[case[0]]
        keep = {}
        check_take(e.pkg, e.lib, e.mem, t.sources[case[1]], t.chunks, t.rows_plain, t.row_bytes, t.index, what=(t.name, case[1]), stream=stream, keep=keep)
        return keep


class PutWorker(RowWorker):
    entry_points = ("blosc_gpu_put_batch", "blosc_gpu_put_packed")

    def run(self, case, stream):
        e, t = self.env, self.tables[case[0]]
        keep = {}
        check_put(e.pkg, e.lib, e.mem, e.oracle, t.sources[case[1]], t.chunks, t.row_bytes, t.index, t.params, 1 if case[1] == "batch" else 256,
                  3, True, what=(t.name, case[1]), stream=stream, keep=keep)
        return keep


# the writers of include/blosc_gpu_put.h that give the same bytes for the same input: (codec, typesize, filter) at clevel 5
PUT_SETTINGS = [("lz4", 8, 1), ("blosclz", 17, 2), ("zstd", 4, 1)]
ROW_SIZES = [12, 17, 96, 4080]      # one lane per row, several lanes per row, rows across block boundaries


def row_tables(env, nchunks=None, **kw):
    """the four row sizes, each under a writer of its own (the fourth shares the first's)"""
    return [RowTable(env, PUT_SETTINGS[k % 3], rb, None if nchunks is None else nchunks[k % len(nchunks)], turn=k, **kw) for k, rb in enumerate(ROW_SIZES)]


# ---- where and aggregate ----
FIELD_LAYOUTS = [wh.LAYOUTS[0], wh.LAYOUTS[2]]      # a float32 field in rows of 4 bytes; an int64 field at offset 9 of rows of 17


class FieldTable:
    """one table of where / aggregate: a where_checks layout under a (codec, typesize, filter, scale) setting, cut or extended to nchunks"""
    def __init__(self, env, layout, setting, nchunks=None, turn=0):
        self.layout, self.setting = layout, setting
        row_bytes, offset, kind, nbytes = layout
        self.values = wh.value_set(kind, nbytes)
        wenv = wh.Env(env.pkg, env.lib, env.mem, env.oracle, env.writer)
        chunks, _ = wh.table_call(wenv, setting, layout, wh.drawn(self.values, wh.total_rows(row_bytes, setting[3])), turn)
        write = env.writer(setting[0], setting[1], setting[2], turn)
        more = lambda k: 6000 // row_bytes + 3 + 17 * k      # rows of a chunk behind the layout's own
        extra = lambda k: write(k, wh.make_table(more(k), row_bytes, offset, nbytes, wh.drawn(self.values, more(k), seed=50 + k + turn), seed=60 + k))
        self.chunks = resized(chunks, nchunks, extra)
        self.rows_plain = plaintext(env.oracle, self.chunks)
        self.sources = both_sources(env.mem, self.chunks)
        self.name = f"{setting[0]}-T{setting[1]}-shuffle{setting[2]}-rows-of-{row_bytes}-{wh.kind_name(kind, nbytes)}-{len(self.chunks)}-chunks"


class WhereWorker(RowWorker):
    entry_points = ("blosc_gpu_where_batch", "blosc_gpu_where_packed")

    def __init__(self, env, tables, variants=("batch", "packed"), ops=range(6)):
        super().__init__(env, tables, variants)
        self.ops = ops

    def run(self, case, stream):
        e, t = self.env, self.tables[case[0]]
        row_bytes, offset, kind, nbytes = t.layout
        out = {}
        for op in self.ops:
            keep = {}
            args = (offset, kind, nbytes, op, t.values[(op + 3) % len(t.values)])
            wh.check_where(e.lib, e.mem, t.sources[case[1]], t.chunks, t.rows_plain, row_bytes, args, e.pkg, stream=stream, what=(t.name, case[1]), keep=keep)
            out.update({f"{wh.OPS[op].__name__}.{k}": v for k, v in keep.items()})
        return out


def records(entries):
    """aggregate_checks.entry tuples as the 64 bytes of the header's struct each"""
    return np.frombuffer(b"".join(struct.pack("<5q8s8sQ", *e) for e in entries), np.uint8)


class AggregateWorker(RowWorker):
    """every float sum is compared bit for bit with aggregate_checks.tree_sum, the header's order of additions, inside check_aggregate (its
    `exact` asks for math.fsum's value, which only the tables built for it give)"""
    entry_points = ("blosc_gpu_aggregate_batch", "blosc_gpu_aggregate_packed")

    def __init__(self, env, tables, variants=("batch", "packed")):
        super().__init__(env, tables, variants)
        self.aenv = ag.make_env(env.pkg, env.lib, env.mem, env.oracle, env.writer)

    def run(self, case, stream):
        t = self.tables[case[0]]
        row_bytes, offset, kind, nbytes = t.layout
        pick = (ag.LT, t.values[4]) if kind in (ag.FLOAT, ag.BFLOAT16) else (ag.GE, t.values[2])
        out = {}
        for name, flt in (("unfiltered", None), ("filtered", (offset, kind, nbytes) + pick)):
            total, chunks = ag.check_aggregate(self.aenv, t.sources[case[1]], t.chunks, t.rows_plain, row_bytes, (offset, kind, nbytes), flt, stream=stream,
                                               what=(t.name, case[1]))
            out[name] = records([total] + chunks)
        return out


FIELD_SETTINGS = [("lz4", 8, 1, 8), ("blosclz", 17, 1, 1), ("zstd", 4, 1, 8), ("zlib", 17, 2, 1), ("lz4", 17, 0, 1), ("blosclz", 4, 1, 8)]


def field_tables(env, layouts=FIELD_LAYOUTS, settings=FIELD_SETTINGS, nchunks=None):
    return [FieldTable(env, lay, settings[k % len(settings)], None if nchunks is None else nchunks[k % len(nchunks)], turn=k) for k, lay in enumerate(layouts)]


# ---- packed compress and decompress ----
class PackedWorker(Worker):
    """blosc_gpu_compress_packed and blosc_gpu_decompress_packed over the first chunks of batch_bounds_checks.mixed_hosts(SMALL).  A geometry is
    (number of chunks, typesize, codec, clevel, filter); every container is laid out by the header's rule, read back chunk by chunk by the
    oracle (and the reference where it is built), and decompressed again into the plain bytes"""
    entry_points = ("blosc_gpu_compress_packed", "blosc_gpu_decompress_packed")

    def __init__(self, env, geometries=None, aligns=(1, 256), hosts=None):
        super().__init__()
        self.env, self.aligns = env, aligns
        self.geometries = geometries or [(8, 8, c, l, 1) for c, l in DETERMINISTIC]
        self.hosts = mixed_hosts(SMALL) if hosts is None else hosts
        self.src = [env.mem.put(h) for h in self.hosts]

    def cases(self):
        return [(g, a) for g in range(len(self.geometries)) for a in self.aligns]

    def turn(self, r):
        return [(g, self.aligns[r % len(self.aligns)]) for g in range(len(self.geometries))]

    def run(self, case, stream):
        e = self.env
        n, T, cname, clevel, shuffle = self.geometries[case[0]]
        align = case[1]
        hosts, sizes, ptrs = self.hosts[:n], [h.size for h in self.hosts[:n]], [p for _, p in self.src[:n]]
        what = (self.geometries[case[0]], "align", align)
        pb = e.pkg.PackedBatch(n, lib=e.lib)
        cap = pb.bound(sizes, align)
        buf, base = e.mem.filled(cap + GUARD, FILL)
        assert pb.compress(ptrs, sizes, base, cap, T, clevel, shuffle, cname.encode(), BLOCKSIZE, align, stream=stream) == 0, what
        off, cb = pb.offsets(), pb.results()
        image = e.mem.get(buf)[:cap + GUARD].copy()
        assert all(c > 0 for c in cb) and off == host_offsets(cb, align) and off[-1] <= cap, (what, off, cb)
        assert np.all(image[off[-1]:] == FILL), (what, "bytes behind the container were written")
        chunks = [image[off[i]:off[i] + cb[i]] for i in range(n)]
        for i, c in enumerate(chunks):
            assert header(c)["cbytes"] == cb[i] and header(c)["nbytes"] == sizes[i] and header(c)["typesize"] == T, (what, i, header(c))
            assert np.all(image[off[i] + cb[i]:off[i + 1]] == 0), (what, "padding behind chunk", i)
        check_chunks_decode(chunks, hosts, e.oracle, e.ref)
        total = sum(sizes)
        out, obase = e.mem.filled(total + GUARD, FILL)
        cont, cbase = e.mem.put(image[:off[-1]])
        back = e.pkg.PackedBatch(n, lib=e.lib)
        assert back.decompress(cbase, off[-1], off, obase, total, stream=stream) == 0, what
        plain_bytes = e.mem.get(out)[:total + GUARD].copy()
        assert back.results() == sizes and back.offsets() == host_offsets(sizes, 1), (what, back.results())
        assert np.array_equal(plain_bytes[:total], np.concatenate(hosts)) and np.all(plain_bytes[total:] == FILL), (what, "the plain bytes differ")
        return {"container": image, "offsets": np.array(off, np.int64), "cbytes": np.array(cb, np.int64), "plain": plain_bytes}


# ---- compress with parameters per chunk, trial compression ----
class ParamsSelectWorker(Worker):
    """params_checks.check_every_setting_in_one_batch and select_checks.check_deterministic on mixed_hosts(SMALL).  Their yardstick - the chunks
    of the existing blosc_gpu_compress_batch, one setting a call - is computed here, before the threads: it moves the process-wide split mode"""
    entry_points = ("blosc_gpu_compress_batch_params", "blosc_gpu_compress_packed_params", "blosc_gpu_compress_batch_select", "blosc_gpu_compress_packed_select")

    def __init__(self, env, aligns=(1, 256), nhosts=5):
        super().__init__()
        self.env, self.aligns = env, aligns
        self.calls = sc.Calls(env.pkg, env.lib, env.mem, BLOCKSIZE)
        self.hosts = mixed_hosts(SMALL)[:nhosts]      # two that compress and the three specials
        self.settings = pc.deterministic_settings(2 * BLOCKSIZE)
        self.ref_chunks = pc.reference_chunks(self.calls, self.hosts, self.settings)
        self.candidates = sc.candidates()
        self.yard = sc.yardstick(self.calls, self.hosts, self.candidates)

    def cases(self):
        return ["params", "select"]

    def turn(self, r):
        return self.cases()

    def run(self, case, stream):
        e, keep = self.env, {}
        if case == "params":
            pc.check_every_setting_in_one_batch(self.calls, self.hosts, self.settings, self.ref_chunks, e.oracle, e.ref, self.aligns, stream=stream, keep=keep)
        else:
            sc.check_deterministic(self.calls, self.hosts, self.candidates, self.yard, e.oracle, e.ref, self.aligns, stream=stream, keep=keep)
        return keep


# ---- getitem ranges and checksums ----
FIVE_CODECS = [("lz4", 17, 1), ("blosclz", 4, 2), ("lz4hc", 8, 1), ("zlib", 1, 0), ("zstd", 4, 1)]


class GetitemChecksumWorker(Worker):
    """a seeded sample of getitem_ranges_checks.chunk_ranges over chunks of the five codecs and the three specials, through
    blosc_gpu_getitem_batch (check_batch) and _packed; the digests of checksum_checks.many_runs_case's 300 runs, both kinds, both calls"""
    entry_points = ("blosc_gpu_getitem_batch", "blosc_gpu_getitem_packed", "blosc_gpu_checksum_batch", "blosc_gpu_checksum_packed")

    def __init__(self, env, seed=9, nranges=60):
        super().__init__()
        self.env = env
        small = plain(SMALL)
        self.chunks = []
        for cname, T, shuffle in FIVE_CODECS:
            if env.ref is not None: self.chunks.append(ref_compress(env.ref, small, T, 5, shuffle, cname.encode(), blocksize=BLOCKSIZE)[1])
            elif cname in ("lz4", "blosclz"): self.chunks.append(orc_compress(env.oracle, small, T, 5, shuffle, cname, blocksize=BLOCKSIZE)[1])
            else: self.chunks.append(env.lib_chunk(small, T, shuffle, cname))
        self.chunks += [orc_compress(env.oracle, np.random.default_rng(3).integers(0, 256, 9000, dtype=np.uint8), 4, 5, 1, "lz4")[1],
                        orc_compress(env.oracle, plain(100), 4, 5, 1, "lz4")[1], orc_compress(env.oracle, plain(0), 4, 5, 1, "lz4")[1]]
        every = [(ci, s, k) for ci, c in enumerate(self.chunks) for s, k in chunk_ranges(c)] + [(len(self.chunks), 0, 1)]
        rng = np.random.default_rng(seed)
        self.ranges = [every[int(k)] for k in rng.permutation(len(every))[:nranges]]
        self.want = expected(env.oracle, self.chunks, self.ranges)
        self.flat = np.concatenate([d for r, d in self.want if r > 0])
        image, self.offsets = pack_container(self.chunks, 1)
        self.container, self.size = env.mem.put(image), int(image.size)
        self.buf, self.runs = cs.many_runs_case()
        self.digests = {kind: cs.expected(kind, self.buf, self.runs) for kind in cs.KINDS}
        self.dev = env.mem.put(self.buf)

    def cases(self):
        return ["getitem batch", "getitem packed", "checksum"]

    def turn(self, r):
        return [self.cases()[r % 2], "checksum"]

    def run(self, case, stream):
        e, keep = self.env, {}
        if case == "getitem batch":
            check_batch(e.pkg, e.lib, e.mem, e.oracle, self.chunks, self.ranges, "concurrent", stream=stream, keep=keep)
        elif case == "getitem packed":
            res = [r for r, _ in self.want]
            out, obase = e.mem.filled(self.flat.size + 64, SENTINEL)
            b = e.pkg.ItemRanges(self.ranges, lib=e.lib)
            assert b.packed(self.container[1], self.size, self.offsets, obase, self.flat.size, stream=stream) == 0
            got = e.mem.get(out)[:self.flat.size + 64].copy()
            assert b.results() == res and b.offsets() == prefix(res), [(k, self.ranges[k], g, w) for k, (g, w) in enumerate(zip(b.results(), res)) if g != w][:8]
            assert np.array_equal(got[:self.flat.size], self.flat) and np.all(got[self.flat.size:] == SENTINEL), "the slices differ from the oracle's"
            keep.update(results=np.array(b.results(), np.int64), offsets=np.array(b.offsets(), np.int64), bytes=got)
        else:
            base = self.dev[1]
            for kind in cs.KINDS:
                a = e.pkg.checksums(kind, [base + o for o, _ in self.runs], [n for _, n in self.runs], lib=e.lib, stream=stream)
                b = e.pkg.checksums_packed(kind, base, self.buf.size, [o for o, _ in self.runs] + [self.buf.size], [n for _, n in self.runs], lib=e.lib, stream=stream)
                for form, got in (("batch", a), ("packed", b)):
                    bad = [(i, self.runs[i], hex(got[i]), hex(self.digests[kind][i])) for i in range(len(self.runs)) if got[i] != self.digests[kind][i]]
                    assert not bad, (cs.KIND_IDS[kind - 1], form, len(bad), bad[:5])
                    keep[f"{cs.KIND_IDS[kind - 1]} {form}"] = np.array(got, np.uint32)
        return keep


# ---- the stock _ctx calls on host buffers ----
class CtxWorker(Worker):
    """blosc_compress_ctx, blosc_decompress_ctx and blosc_getitem on host buffers - the calls that run on their context's own stream: a job of
    tests/test_gpu_threads.py's list, its checks"""
    entry_points = ("blosc_compress_ctx", "blosc_decompress_ctx", "blosc_getitem")

    def __init__(self, env, job=("smallints", 1 << 20, 4, 2, b"lz4", 5)):
        super().__init__()
        self.env, self.job = env, job
        self.data = DATASETS[job[0]](job[1])

    def cases(self):
        return ["round trip"]

    def run(self, case, stream):
        L = self.env.lib
        _, n, T, shuffle, cname, clevel = self.job
        data = self.data
        dst = np.full(n + 16 + 64, 0xEE, np.uint8)
        r = L.blosc_compress_ctx(clevel, shuffle, T, n, ptr(data), ptr(dst), n + 16, cname, 0, 1)
        assert 0 < r <= n + 16 and np.all(dst[n + 16:] == 0xEE), r
        chunk = dst[:r].copy()
        r2, out = orc_decompress(self.env.oracle, chunk, n)
        assert r2 == n and np.array_equal(out, data), "the oracle cannot read it"
        back = np.full(n + 64, 0xEE, np.uint8)
        assert L.blosc_decompress_ctx(ptr(chunk), ptr(back), n, 1) == n
        assert np.array_equal(back[:n], data) and np.all(back[n:] == 0xEE)
        nitems = min(1000, n // T)
        start = (n // T - nitems) // 2
        item = np.full(nitems * T + 16, 0xEE, np.uint8)
        assert L.blosc_getitem(ptr(chunk), start, nitems, ptr(item)) == nitems * T
        assert np.array_equal(item[:nitems * T], data[start * T:(start + nitems) * T]) and np.all(item[nitems * T:] == 0xEE)
        return {"chunk": chunk}


# ---- the runner ----
@contextmanager
def no_stream(stream):
    yield


def run_threads(rec, workers, rounds, stream_for=None, on_stream=no_stream, pass_bytes=0, timeout=JOIN_TIMEOUT):
    """One daemon thread per worker of `workers` (every worker's serial answers are there already), `rounds` rounds, each begun together on a
    barrier.  stream_for(thread number) -> (stream object, its handle) or None, made inside the thread; odd rounds run on it, inside
    on_stream(stream object), even rounds on the NULL stream.  pass_bytes: the pass bound for the whole run, set before the threads start and
    put back after the joins.  Every thread's first exception is collected; a thread that is still alive `timeout` seconds after the start
    fails the run with its last logged call.  Returns the Overlap of what ran."""
    n = len(workers)
    marks, errors = [], []
    barrier = threading.Barrier(n, action=lambda: marks.append(len(rec.log)))

    def body(tid):
        who = threading.current_thread().name
        r = -1
        try:
            made = stream_for(tid) if stream_for is not None else None
            for r in range(rounds):
                barrier.wait(timeout)
                side = made is not None and r % 2 == 1
                for case in workers[tid].turn(r):
                    with on_stream(made[0]) if side else no_stream(None):
                        workers[tid].repeat(case, made[1] if side else None, (who, "round", r, "side stream" if side else "NULL stream"))
            if made is not None:
                made[0].synchronize()
        except BaseException as e:      # noqa: BLE001 - reported by the main thread
            errors.append((who, "round", r, repr(e)))
            barrier.abort()

    threads = [threading.Thread(target=body, args=(t,), name=f"t{t}-{type(workers[t]).__name__}", daemon=True) for t in range(n)]
    if pass_bytes:
        rec._lib.blosc_amd_getitem_pass_bytes(pass_bytes)
    try:
        deadline = time.monotonic() + timeout
        for t in threads:
            t.start()
        for t in threads:
            t.join(max(deadline - time.monotonic(), 0.0))
        stuck = [(t.name, rec.last.get(t.name)) for t in threads if t.is_alive()]
    finally:
        if pass_bytes:
            rec._lib.blosc_amd_getitem_pass_bytes(0)
    marks.append(len(rec.log))
    assert not stuck, ("threads still alive after the timeout, with their last logged call", stuck, errors)
    real = [e for e in errors if "BrokenBarrierError" not in e[3]]
    assert not real and not errors, real or errors
    assert len(marks) == rounds + 1, marks
    return Overlap(rec.log, marks)
