"""CPU: the WHOLE library - host engine (tables, queues, staging, return codes) and every kernel - built for the host on top of the
wavefront emulator and its HIP runtime stand-in (tests/tools/blosc_emu_lib.cpp: the same engine.hip / blosc_api.hip / k_*.hip sources,
kernel launches run workgroup by workgroup as groups of fibers).  Test infrastructure, never shipped: the product has no CPU path.
Chunk-level round trips through the stock C ABI for every codec and for every encoder option behind a switch - the options built after
the round's GPU time was spent get their host wiring (kernel selection, scratch allocation) exercised here before their first device
run.  Yardsticks: the oracle and, where oracle/_ref ships, the reference itself."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import DATASETS, golden_npz, header, orc_compress, orc_decompress, ptr, ref_compress, ref_decompress

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SEED = int(os.environ.get("BLOSC_EMU_SEED", "0"))        # soak runs: BLOSC_EMU_FULL=1 BLOSC_EMU_SEED=1, 2, ... draw other streams in the two random-stream tests and another sample of the parameter grid
FULL = os.environ.get("BLOSC_EMU_FULL") == "1"          # the default run is sized for a CPU suite of a few minutes; BLOSC_EMU_FULL=1 takes everything


SOAK = 7919 * int(os.environ.get("BLOSC_EMU_SEED", "0"))      # soak runs (BLOSC_EMU_SEED=1, 2, ...): every random draw of this file moves

@pytest.fixture(scope="module")
def emulib():
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang++")
    csrc = os.path.join(ROOT, "c-blosc_amd", "csrc")
    tools = os.path.join(ROOT, "tests", "tools")
    so = os.path.join(tools, "libblosc_amd_emu.so")
    deps = [os.path.join(tools, "blosc_emu_lib.cpp"), os.path.join(tools, "wave_emu", "wave_emu.h"), os.path.join(tools, "wave_emu", "hip_emu_runtime.h")]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    if os.environ.get("BLOSC_EMU_LIB"):          # a build of one's own, e.g. with -fsanitize=address (HISTORY.md: the sanitizer pass of round 5)
        so = os.environ["BLOSC_EMU_LIB"]
    elif not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([CLANG, "-std=c++17", "-O1", "-shared", "-fPIC", "-w", "-I", os.path.join(tools, "wave_emu"), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), "-x", "c++", deps[0], "-o", so, "-lpthread"])
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkgmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkgmod)
    return pkgmod.declare(C.CDLL(so))


def _compress(L, data, T, clevel, shuffle, cname, blocksize=0):
    data = np.ascontiguousarray(data)
    out = np.full(data.size + 16 + 64, 0xEE, np.uint8)
    r = L.blosc_compress_ctx(clevel, shuffle, T, data.size, ptr(data), ptr(out), data.size + 16, cname, blocksize, 1)
    assert np.all(out[data.size + 16:] == 0xEE)
    return r, out[:max(r, 0)].copy()


def _decompress(L, chunk, n):
    chunk = np.ascontiguousarray(chunk)
    out = np.full(n + 64, 0xEE, np.uint8)
    r = L.blosc_decompress_ctx(ptr(chunk), ptr(out), n, 1)
    assert np.all(out[n:] == 0xEE)
    return r, out[:n]


def _everybody_reads(L, oracle, ref, chunk, data):
    r, out = orc_decompress(oracle, chunk, data.size)
    assert r == data.size and np.array_equal(out, data), "the oracle cannot read it"
    if ref is not None:
        r, out = ref_decompress(ref, chunk, data.size)
        assert r == data.size and np.array_equal(out, data), "stock c-blosc cannot read it"
    r, out = _decompress(L, chunk, data.size)
    assert r == data.size and np.array_equal(out, data), "our own decoder cannot read it"


@pytest.mark.parametrize("cname", [b"lz4", b"blosclz", b"lz4hc", b"zlib", b"zstd"])
def test_round_trips_through_the_c_abi(emulib, oracle, ref, cname):
    for dname, T, shuffle, n in [("bench19", 8, 1, 40000), ("linspace", 8, 1, 20001), ("smallints", 4, 2, 16000), ("randwalk", 8, 1, 10000),
                                 ("zeros", 4, 1, 50000), ("random", 1, 0, 3000), ("bench19", 3, 1, 5000), ("arange", 4, 1, 129)][:8 if FULL else 5]:
        data = DATASETS[dname](n)
        r, chunk = _compress(emulib, data, T, 5, shuffle, cname)
        assert 0 < r <= n + 16 and header(chunk)["cbytes"] == r and header(chunk)["nbytes"] == n
        _everybody_reads(emulib, oracle, ref, chunk, data)
    # chunks written by the reference / the oracle come back bit-exactly, whole and in items
    data = DATASETS["bench19"](30000)
    if ref is not None:
        r, stock = ref_compress(ref, data, 8, 5, 1, cname)
    elif cname in (b"lz4", b"blosclz"):
        r, stock = orc_compress(oracle, data, 8, 5, 1, cname.decode())
    else:
        return
    r2, out = _decompress(emulib, stock, data.size)
    assert r2 == data.size and np.array_equal(out, data)
    item = np.zeros(8 * 100, np.uint8)
    assert emulib.blosc_getitem(ptr(stock), 1000, 100, ptr(item)) == 800 and np.array_equal(item, data[8000:8800])


def test_split_blocks_followed_by_an_unsplit_leftover_block(emulib, oracle, ref):
    """A chunk whose last block is shorter than the block size: the full blocks are split into typesize streams (and unshuffled by the
    decode kernel from one plane per stream), the leftover block is ONE stream holding all planes back to back - both layouts in one
    chunk, through our own writer and the reference's.  (Round 3: a scratch-layout change had the unshuffle of the leftover block
    read its planes one block apart; only the container test on the device noticed.)"""
    for T, forced, bsize, n in ((4, 16384, 65536, 65536 * 2 + 5001), (8, 8192, 65536, 65536 + 12345)):      # (a splittable block is typesize x the forced size, blosc.c:1037-1048)
        data = DATASETS["smallints" if T == 4 else "bench19"](n)
        r, chunk = _compress(emulib, data, T, 5, 1, b"lz4", blocksize=forced)
        assert r > 0 and header(chunk)["blocksize"] == bsize
        _everybody_reads(emulib, oracle, ref, chunk, data)
        ro, stock = orc_compress(oracle, data, T, 5, 1, "lz4", blocksize=forced)
        assert header(stock)["blocksize"] == bsize
        r2, out = _decompress(emulib, stock, n)
        assert r2 == n and np.array_equal(out, data)


@pytest.mark.parametrize("fmt", [1, 0])
def test_random_structured_streams(emulib, oracle, fmt):
    """tests/test_gpu_random_streams.py's generator (sequences drawn from the shapes the ring decoder treats differently: spans, rows, far and near
    sources, short periods) on the emulated library: chunks of split shuffled blocks whose planes are random LZ4 / BloscLZ streams, the oracle's reader
    says what they decode to.  (With the decoder of round 4 this sample has failing chunks: the short-period match behind a span.)"""
    from helpers import wrap_planes_as_chunk
    from test_gpu_random_streams import rand_stream
    rng = np.random.default_rng(1000 + (1 if fmt == 1 else 3) + 7919 * SEED)
    for k in range(160 if FULL else 24):
        T = int(rng.choice([8, 4, 2, 16])); neb = int(rng.choice([128 << 10, 128 << 10, 64 << 10, 40 << 10, 17 << 10]))
        chunk = wrap_planes_as_chunk([rand_stream(rng, neb, fmt) for _ in range(T)], neb, fmt)
        n = T * neb
        want = np.zeros(n, np.uint8)
        assert oracle.orc_decompress(ptr(chunk), ptr(want), n) == n
        r, out = _decompress(emulib, chunk, n)
        assert r == n and np.array_equal(out, want), (fmt, k, T, neb, r, int((out != want).sum()) if r == n else -1)


@pytest.mark.parametrize("fmt", [1, 0])
def test_long_power_of_two_matches_and_the_window_edge(emulib, oracle, fmt):
    """tests/test_gpu_random_streams.py::edge_stream on the emulated library: the row-register form of long power-of-two matches (dec_ring.h: dr_match)
    and the 16-byte guard band at the far edge of the ring it needs."""
    from helpers import wrap_planes_as_chunk
    from test_gpu_random_streams import edge_stream
    rng = np.random.default_rng(4242 + fmt + 7919 * SEED)
    for k in range(120 if FULL else 16):
        T = int(rng.choice([8, 4, 2])); neb = int(rng.choice([128 << 10, 64 << 10, 33 << 10]))
        chunk = wrap_planes_as_chunk([edge_stream(rng, neb, fmt) for _ in range(T)], neb, fmt)
        n = T * neb
        want = np.zeros(n, np.uint8)
        assert oracle.orc_decompress(ptr(chunk), ptr(want), n) == n
        r, out = _decompress(emulib, chunk, n)
        assert r == n and np.array_equal(out, want), (fmt, k, T, neb, r, int((out != want).sum()) if r == n else -1)


def test_short_period_match_right_behind_a_span_on_reference_data(emulib, oracle):
    """Round 5's silent decode error, on the emulator: blocks 7 .. 9 of the reference's chunk of 64 MiB `linspace` float64 labelled typesize 4
    (blosc_getitem decodes only the blocks it needs).  Plane 3 of blocks 8 and 9 is "2 literals, 32 766 bytes at distance 2, 1 literal, 32 767 bytes at
    distance 2, ...": a periodic span that ends exactly on a row boundary, then a short-period match whose first source byte lies below the span's end -
    in global memory only, not in the wave's LDS ring (dec_ring.h: dr_match).  tests/test_gpu_spans.py has the hand-built family."""
    n = 64 << 20
    data = DATASETS["linspace"](n)
    r, chunk = orc_compress(oracle, data, 4, 5, 1, "lz4")
    bs = header(chunk)["blocksize"]
    assert r > 0 and bs == 512 << 10
    ne = bs // 4
    for blk in (7, 8, 9, 31, 32):
        item = np.zeros(bs, np.uint8)
        assert emulib.blosc_getitem(ptr(chunk), blk * ne, ne, ptr(item)) == bs
        assert np.array_equal(item, data[blk * bs:(blk + 1) * bs]), (blk, int((item != data[blk * bs:(blk + 1) * bs]).sum()))


@pytest.mark.parametrize("T", [8, 4, 1])
def test_bitshuffle_inside_the_codec_kernels(emulib, oracle, ref, T):
    """Bit(un)shuffle as work of the encode / decode kernels' own waves (enc_shuffle.h: bitshuffle_block_wave_T, k_decode.hip:
    bitunshuffle_block_wave_T; typesize 8 since round 5 with 16 elements per lane and pass): split blocks whose element count is a multiple of
    the pass (2048 / 1024), of the lane chunk (32 / 16), of 8 only, and not of 8 (the filter then copies the block, shuffle.c:412-414), a
    leftover block, trailing bytes - written here and read by everybody, written by the oracle and read here."""
    for n in [T * (2048 * 2 + 1024 + 48 + 8) + (T - 1), T * 1000 + 3, T * (16384 + 24), 8 * T, 5 * T]:
        for dname in ("smallints", "bench19"):
            data = DATASETS[dname](n)
            for cname in (b"lz4", b"blosclz"):
                for blocksize in (0, 4096):
                    r, chunk = _compress(emulib, data, T, 5, 2, cname, blocksize=blocksize)
                    assert r > 0, (T, n, dname, cname, blocksize)
                    _everybody_reads(emulib, oracle, ref, chunk, data)
                    ro, stock = orc_compress(oracle, data, T, 5, 2, cname.decode(), blocksize=blocksize)
                    assert ro > 0 and header(stock)["blocksize"] == header(chunk)["blocksize"]
                    r2, out = _decompress(emulib, stock, n)
                    assert r2 == n and np.array_equal(out, data), (T, n, dname, cname, blocksize)


@pytest.mark.parametrize("T", [2, 16])
def test_typesize_2_and_16_take_the_fused_paths(emulib, oracle, ref, T):
    """Round 3: the byte (un)shuffle of typesize 2 and 16 runs inside the encode / decode kernels like that of 4 and 8 (enc_shuffle.h:
    shuffle_block_task_x, k_decode.hip: unshuffle_block_wave_T<2> / unshuffle_block_wave_16 with the lane table): split blocks with
    constant, periodic, noisy and incompressible planes + an unsplit leftover block, written here and by the reference."""
    rng = np.random.default_rng(70 + T + SOAK)
    ne = 16384                                                    # bytes per plane of a full block: spans need >= 16 KiB matches
    nfull = 2 if (FULL or T == 2) else 1
    planes = []
    for j in range(T):
        kind = j % 5
        if kind == 0: planes.append(np.zeros(ne * nfull + 777, np.uint8))
        elif kind == 1: planes.append(rng.integers(0, 256, ne * nfull + 777, dtype=np.uint8))
        elif kind == 2: planes.append(np.resize(rng.integers(0, 256, 64, dtype=np.uint8), ne * nfull + 777))
        elif kind == 3: planes.append(rng.integers(0, 3, ne * nfull + 777, dtype=np.uint8))
        else: planes.append(np.resize(rng.integers(0, 256, 4096, dtype=np.uint8), ne * nfull + 777))
    data = np.ascontiguousarray(np.stack(planes, 1)).reshape(-1)
    data = np.concatenate([data, rng.integers(0, 256, T - 1, dtype=np.uint8)])          # bytes that do not form a whole element
    for cname in (b"lz4", b"blosclz"):
        r, chunk = _compress(emulib, data, T, 5, 1, cname, blocksize=ne)               # (a splittable block is typesize x the forced size)
        ro, stock = orc_compress(oracle, data, T, 5, 1, cname.decode(), blocksize=ne)
        bs = header(stock)["blocksize"]
        assert ro > 0 and bs >= ne * T and bs < data.size and not header(stock)["flags"] & 0x10            # (blosc.c:1037-1048 widens small split blocks to 64 KiB); split
        assert r > 0 and header(chunk)["blocksize"] == bs and header(chunk)["typesize"] == T and header(chunk)["flags"] == header(stock)["flags"]
        assert r < data.size * 0.75
        _everybody_reads(emulib, oracle, ref, chunk, data)
        r2, out = _decompress(emulib, stock, data.size)
        assert r2 == data.size and np.array_equal(out, data)
        item = np.zeros(T * 300, np.uint8)
        assert emulib.blosc_getitem(ptr(stock), ne + 100, 300, ptr(item)) == T * 300 and np.array_equal(item, data[T * (ne + 100):T * (ne + 400)])


SWITCHES = [
    (b"zstd", {"BLOSC_AMD_ZSTD_TABLES": "1"}),
    (b"zstd", {"BLOSC_AMD_ZSTD_TABLES": "1", "BLOSC_AMD_ZSTD_HUFFMAN": "1"}),
    (b"zstd", {"BLOSC_AMD_ZSTD_SEARCH": "1"}),
    (b"zstd", {"BLOSC_AMD_ZSTD_SEARCH": "1", "BLOSC_AMD_ZSTD_HUFFMAN": "1"}),
    (b"zlib", {"BLOSC_AMD_ZLIB_SEARCH": "1"}),
    (b"zlib", {"BLOSC_AMD_ZLIB_DYNAMIC": "1"}),
    (b"zlib", {"BLOSC_AMD_ZLIB_DYNAMIC": "1", "BLOSC_AMD_ZLIB_SEARCH": "1"}),
    (b"lz4hc", {"BLOSC_AMD_LZ4HC": "0"}),
]


@pytest.mark.parametrize("cname,env", SWITCHES, ids=["+".join(k[10:].lower() + "=" + v for k, v in e.items()) for _, e in SWITCHES])
def test_encoder_options_behind_switches(emulib, oracle, ref, cname, env):
    """Every switch selects its kernel (and the scratch that kernel needs) in the host engine, chunks stay readable by everybody, and the
    option does what it is for: not larger than the plain path, and smaller where it should be."""
    keys = ("BLOSC_AMD_ZSTD_TABLES", "BLOSC_AMD_ZSTD_HUFFMAN", "BLOSC_AMD_ZSTD_SEARCH", "BLOSC_AMD_ZLIB_SEARCH", "BLOSC_AMD_ZLIB_DYNAMIC", "BLOSC_AMD_LZ4HC")
    old = {k: os.environ.get(k) for k in keys}
    try:
        tot_plain = tot_opt = 0
        for dname, T, n in [("bench19", 8, 98304), ("linspace", 8, 32768), ("smallints", 4, 32768), ("randwalk", 8, 16384), ("zeros", 8, 20000)][:5 if FULL else 3]:
            data = DATASETS[dname](n)
            for k in keys:
                os.environ[k] = "0"                     # the plain writers (several options are the default since round 3)
            if cname == b"lz4hc":
                os.environ["BLOSC_AMD_LZ4HC"] = "1"
            rp, _ = _compress(emulib, data, T, 5, 1, cname)
            os.environ.update(env)
            r, chunk = _compress(emulib, data, T, 5, 1, cname)
            assert r > 0 and rp > 0
            _everybody_reads(emulib, oracle, ref, chunk, data)
            tot_plain += rp; tot_opt += r
        print(f"{cname.decode()} {env}: {tot_plain} -> {tot_opt} bytes")
        if cname == b"lz4hc":
            assert tot_opt >= tot_plain                   # the switch turns the search OFF
        else:
            assert tot_opt < tot_plain
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_reference_written_zstd_chunks_through_the_two_phase_path(emulib, oracle):
    """The committed chunks written by the real reference (tests/golden/ref_zstd_chunks.npz: clevel 1-9, typesize 1-8, every filter) through
    the engine's default Zstd path - k_zstd_entropy (set-up, Huffman streams, 16-bit sequence tables), k_zstd_seq (one lane per frame, the
    three-refill bit reader of round 3), k_zstd_exec with the unshuffle of the decoding wave - intact, and damaged with the oracle's verdict
    and bytes (the oracle is pinned to the reference on damaged frames, tests/test_oracle_zstd.py)."""
    z = golden_npz("ref_zstd_chunks.npz")
    rng = np.random.default_rng(33 + SOAK)
    before = (C.c_ulonglong * 5)(); emulib.emu_zstd_path_counts(before)
    items = []
    for k, m in enumerate(z["meta"]):
        dname, n, T, clevel, shuffle, bs = m.split(",")
        if FULL or k in (0, 5, 10, 20, 3, 13, 21, 15):          # 300 001-byte shuffled typesize-8 chunks (several blocks, a leftover), unfiltered and bit-shuffled ones
            items.append((z[f"c{k}"], dname, int(n)))
    assert len(items) >= 8
    rejected = 0
    for chunk, dname, n in items:
        data = DATASETS[dname](n)
        r, out = _decompress(emulib, chunk, n)
        assert r == n and np.array_equal(out, data), (dname, n)
        for trial in range(12 if FULL else 4):
            c = chunk.copy()
            pos = int(rng.integers(16, c.size))
            if trial % 4 == 3: c[pos] = int(rng.integers(0, 256))
            else: c[pos] ^= 1 << int(rng.integers(0, 8))
            if int(c[12:16].view("<i4")[0]) > c.size:
                continue
            ro, oo = orc_decompress(oracle, c, n)
            rg, og = _decompress(emulib, c, n)
            if ro == n:
                assert rg == n and np.array_equal(og, oo), (dname, n, trial, pos)
            else:
                assert rg < 0, (dname, n, trial, pos, ro, rg)
                rejected += 1
    assert rejected >= 5
    # the paths this test is about really ran: LDS-assembled groups (some with the history kept, some with literals out of the window),
    # frames through k_zstd_seq, blocks unshuffled by the wave that decoded them
    after = (C.c_ulonglong * 5)(); emulib.emu_zstd_path_counts(after)
    ran = [int(a) - int(b) for a, b in zip(after, before)]
    assert ran[0] >= 20 and ran[1] >= 5 and ran[2] >= 5 and ran[3] >= 20 and ran[4] >= 5, ran


def test_reference_written_zlib_chunks_through_the_queued_kernel(emulib, oracle):
    """The committed chunks written by the real reference with zlib (tests/golden/ref_zlib_chunks.npz) through k_zlib_streams as the engine
    launches it since round 3 - per-XCD queues, the block unshuffled by the wave that completes its last stream - intact, and damaged
    with the oracle's verdict and bytes."""
    z = golden_npz("ref_zlib_chunks.npz")
    rng = np.random.default_rng(34 + SOAK)
    items = []
    for k, m in enumerate(z["meta"]):
        dname, n, T, clevel, shuffle, bs = m.split(",")
        if FULL or k in (0, 13, 15):                                  # (inflate on the emulator is slow: ~100 KB/s)
            items.append((z[f"c{k}"], dname, int(n)))
    assert len(items) >= 3
    rejected = 0
    for chunk, dname, n in items:
        data = DATASETS[dname](n)
        r, out = _decompress(emulib, chunk, n)
        assert r == n and np.array_equal(out, data), (dname, n)
        for trial in range(12 if FULL else 3):
            c = chunk.copy()
            pos = int(rng.integers(16, c.size))
            if trial % 4 == 3: c[pos] = int(rng.integers(0, 256))
            else: c[pos] ^= 1 << int(rng.integers(0, 8))
            if int(c[12:16].view("<i4")[0]) > c.size:
                continue
            ro, oo = orc_decompress(oracle, c, n)
            rg, og = _decompress(emulib, c, n)
            if ro == n:
                assert rg == n and np.array_equal(og, oo), (dname, n, trial, pos)
            else:
                assert rg < 0, (dname, n, trial, pos, ro, rg)
                rejected += 1
    assert rejected >= 2


def test_getitem_ranges_and_tight_destinations_sample(emulib, oracle, ref):
    """A seeded sample of blosc_getitem ranges - valid, empty, negative, past the end - on reference-written chunks (return value and bytes of the
    oracle = the reference, blosc.c:1601-1740), and of blosc_compress_ctx into destinations from too small to ample: never more than destsize,
    0 only when it does not fit, whatever is returned decodes with the oracle (blosc.c:1165-1178, :1322-1367; tests/test_maxout.c)."""
    rng = np.random.default_rng(4711 + 7919 * SEED)
    for k in range(60 if FULL else 16):
        cname = ["lz4", "blosclz", "lz4hc", "zlib", "zstd"][k % (5 if ref is not None else 2)]       # (the oracle writes LZ4 and BloscLZ only)
        T = int(rng.choice([1, 2, 3, 4, 8, 16])); shuffle = int(rng.choice([0, 1, 2]))
        n = int(rng.choice([16, 1000, 4096 + 7, 30000, 70001])); n -= n % T if rng.integers(0, 2) else 0
        data = DATASETS[str(rng.choice(["bench19", "smallints", "randwalk", "zeros"]))](n)
        clevel, bs = int(rng.choice([1, 5, 9])), int(rng.choice([0, 0, 1024, 4096]))
        r, chunk = ref_compress(ref, data, T, clevel, shuffle, cname.encode(), blocksize=bs) if ref is not None else orc_compress(oracle, data, T, clevel, shuffle, cname, blocksize=bs)
        assert r > 0
        ni = n // T
        for _ in range(10):
            mode = int(rng.integers(0, 6))
            if mode == 0: s0, cnt = int(rng.integers(0, max(ni, 1))), 0
            elif mode == 1: s0, cnt = -int(rng.integers(1, 5)), int(rng.integers(0, 5))
            elif mode == 2: s0 = int(rng.integers(0, ni + 1)); cnt = ni - s0 + int(rng.integers(1, 4))
            else:
                s0 = int(rng.integers(0, max(ni, 1))); cnt = int(rng.integers(0, ni - s0 + 1))
            want = np.full(max(cnt, 0) * T + 64, 0xEE, np.uint8); got = want.copy()
            r0 = ref.blosc_getitem(ptr(chunk), s0, cnt, ptr(want)) if ref is not None else oracle.orc_getitem(ptr(chunk), s0, cnt, ptr(want))
            r1 = emulib.blosc_getitem(ptr(chunk), s0, cnt, ptr(got))
            assert r0 == r1, (cname, T, n, s0, cnt, r0, r1)
            if r0 > 0: assert np.array_equal(got[:r0], want[:r0])
            assert np.all(got[max(r0, 0):] == 0xEE)
        if cname in ("zlib", "zstd") and n > 40000:
            continue
        for _ in range(4):
            room = int(rng.choice([0, 1, 15, 16, 17, n // 4, n // 2, n, n + 15, n + 16, n + 100]))
            out = np.full(room + 64, 0xEE, np.uint8)
            rc = emulib.blosc_compress_ctx(5, shuffle, T, n, ptr(data), ptr(out), room, cname.encode(), 0, 1)
            assert np.all(out[room:] == 0xEE), "wrote past destsize"
            assert 0 <= rc <= room, (cname, T, n, room, rc)
            if room >= n + 16: assert rc > 0
            if rc > 0:
                back = np.zeros(n, np.uint8)
                rd = ref.blosc_decompress_ctx(ptr(out), ptr(back), n, 1) if ref is not None else oracle.orc_decompress(ptr(out), ptr(back), n)
                assert rd == n and np.array_equal(back, data), (cname, T, n, room, rc, rd)


def test_negative_nbytes_gets_the_references_verdict(emulib, oracle, ref):
    """Bit 31 of the header's nbytes set (damaged input only).  The reference (blosc.c:1485-1511) counts nbytes / blocksize <= 0 blocks, applies its remaining
    header checks with that count, runs no block and returns 0 with nothing written - or -1 / -5 / -9 where one of those checks fails first.  Rounds 1 - 5
    answered -1 throughout (a stated deviation); since round 6 the verdicts are equal, header variant by header variant."""
    data = DATASETS["bench19"](20000)
    for cname in ("lz4", "blosclz"):
        r, chunk = orc_compress(oracle, data, 8, 5, 1, cname)
        base = chunk.copy(); base[7] ^= 0x80
        variants = [("plain", base)]
        t = base.copy(); t[4:8] = np.array([-1], "<i4").view(np.uint8); variants.append(("nbytes -1", t))
        t = base.copy(); t[4:8] = np.array([-(1 << 31)], "<i4").view(np.uint8); variants.append(("nbytes INT_MIN", t))
        t = base.copy(); t[2] |= 0x02; variants.append(("memcpyed flag, sizes disagree", t))
        t = base.copy(); t[2] |= 0x02; t[12:16] = (t[4:8].view("<i4") + 16).view(np.uint8); variants.append(("memcpyed flag, sizes agree", t))
        t = base.copy(); t[2] = (t[2] & 0x1f) | (2 << 5); variants.append(("snappy format id", t))
        t = base.copy(); t[1] = 7; variants.append(("versionlz", t))
        t = base.copy(); t[12:16] = np.array([0], "<i4").view(np.uint8); variants.append(("cbytes 0", t))
        t = base.copy(); t[12:16] = np.array([12], "<i4").view(np.uint8); variants.append(("cbytes 12", t))
        t = base.copy(); t[0] = 3; variants.append(("version", t))
        t = base.copy(); t[2] |= 0x08; variants.append(("reserved flag", t))
        t = base.copy(); t[8:12] = np.array([64], "<i4").view(np.uint8); variants.append(("small blocksize: many negative blocks", t))
        for name, t in variants:
            ro, _ = orc_decompress(oracle, t, data.size)
            if ref is not None:
                dst = np.full(data.size, 0xEE, np.uint8)
                rr = ref.blosc_decompress_ctx(ptr(t), ptr(dst), data.size, 1)
                assert rr == ro and np.all(dst == 0xEE), (cname, name, rr, ro)
            dst = np.full(data.size, 0xEE, np.uint8)
            rg = emulib.blosc_decompress_ctx(ptr(t), ptr(dst), data.size, 1)
            assert rg == ro and np.all(dst == 0xEE), (cname, name, rg, ro)
        assert orc_decompress(oracle, base, data.size)[0] == 0


@pytest.mark.parametrize("cname", ["lz4", "blosclz"])
def test_damaged_chunks_get_the_references_verdict(emulib, oracle, cname):
    """Headers, block offsets, split sizes and stream bytes of reference-written chunks flipped, cut and overwritten: the return code class
    (negative / the size) and, when accepted, the bytes of blosc_decompress in the oracle (= the reference) - through the
    host engine's own validation and the kernels' status words, not only through the stream decoders."""
    rng = np.random.default_rng(17 + 7919 * SEED)
    tried = rejected = 0
    for dname, T, shuffle, n in [("bench19", 8, 1, 20000), ("smallints", 4, 1, 9000), ("randwalk", 8, 0, 5000), ("linspace", 4, 2, 12000)]:
        data = DATASETS[dname](n)
        r, chunk = orc_compress(oracle, data, T, 5, shuffle, cname, blocksize=int(rng.choice([0, 2048, 4096])))
        assert r > 0
        for trial in range(40 if FULL else 20):
            t = chunk.copy()
            mode = trial % 5
            if mode == 0: t[int(rng.integers(0, 16))] ^= 1 << int(rng.integers(0, 8))                      # header
            elif mode == 1: t[int(rng.integers(16, min(t.size, 80)))] ^= 1 << int(rng.integers(0, 8))      # bstarts / first split size
            elif mode == 2: t[int(rng.integers(16, t.size))] = int(rng.integers(0, 256))                  # anywhere
            elif mode == 3: t[int(rng.integers(16, t.size)):] = 0                                           # the tail wiped (the buffer keeps its size: blosc_decompress trusts cbytes)
            else:
                pos = int(rng.integers(16, t.size)); t[pos:pos + 6] = rng.integers(0, 256, min(6, t.size - pos), dtype=np.uint8)
            if int(t[12:16].view("<i4")[0]) > t.size:
                continue                      # cbytes now claims more than the buffer holds: blosc_decompress has no source size, reading it all is the caller's problem
            ro, want = orc_decompress(oracle, t, n)
            r, got = _decompress(emulib, t, n)
            assert (ro < 0) == (r < 0) or (ro == r), f"{dname} {cname} trial {trial} mode {mode}: oracle {ro}, here {r}; header {bytes(chunk[:16]).hex()} -> {bytes(t[:16]).hex()}"
            if ro == n and r == n and mode != 0:
                # accepted by both: same bytes, unless the damage made an LZ4 offset 0 (content unspecified, lz4.c:2356)
                if not np.array_equal(got, want):
                    assert cname == "lz4", (dname, trial, mode)
            tried += 1; rejected += ro < 0
    assert tried > (100 if FULL else 50) and rejected > (20 if FULL else 10)


def test_sampled_parameter_grid(emulib, oracle, ref):
    """A random sample of tests/test_gpu_compress.py's grid (typesize x size x data x shuffle x clevel x codec, leftovers and
    typesizes that are not split included), sized for the emulator: headers as the reference writes them, chunks read by everybody."""
    rng = np.random.default_rng(99 + 7919 * SEED)
    for k in range(70 if FULL else 25):
        cname = [b"lz4hc", b"lz4", b"blosclz", b"zstd", b"zlib"][k % 5]
        T = int(rng.choice([1, 2, 3, 4, 7, 8, 16, 17, 32]))
        n = int(rng.choice([128, 129, 1000, 4096, 32768, 65536 + 17, 100001]))
        dname = str(rng.choice(["bench19", "randwalk", "zeros", "smallints"]))
        shuffle = int(rng.choice([0, 1, 2])); clevel = int(rng.choice([1, 5, 9]))
        if n > 40000 and cname in (b"zstd", b"zlib") and dname == "randwalk":
            n = 32768                                     # (literal-heavy entropy coding is the slowest thing to emulate)
        data = DATASETS[dname](n)
        r, chunk = _compress(emulib, data, T, clevel, shuffle, cname)
        assert 0 < r <= n + 16, (cname, T, n, dname, shuffle, clevel, r)
        if ref is not None:
            rr, stock = ref_compress(ref, data, T, clevel, shuffle, cname)
            a, b = chunk[:12].copy(), stock[:12].copy()
            a[2] &= 0xFD; b[2] &= 0xFD                     # MEMCPYED depends on how well each encoder did
            assert np.array_equal(a, b), (cname, T, n, clevel, header(chunk), header(stock))
        _everybody_reads(emulib, oracle, ref, chunk, data)


FLIPS = [(), ("BLOSC_AMD_SINGLE_QUEUE",), ("BLOSC_AMD_FUSE",), ("BLOSC_AMD_SPANS",), ("BLOSC_AMD_SCHED",), ("BLOSC_AMD_PERIODIC",),
         ("BLOSC_AMD_SINGLE_QUEUE", "BLOSC_AMD_FUSE", "BLOSC_AMD_SPANS", "BLOSC_AMD_SCHED")]


@pytest.mark.parametrize("flip", FLIPS if FULL else [FLIPS[0], FLIPS[1], FLIPS[2], FLIPS[3], FLIPS[-1]], ids=lambda f: "+".join(x.replace("BLOSC_AMD_", "") for x in f) or "defaults")
def test_fallback_switches(emulib, flip):
    """tests/test_gpu_modes.py's switch combinations (one task queue with stand-alone filter kernels, unfused filters, no periodic spans /
    planes, plain block order) on the emulated library, inputs shrunk: the same
    script, a process per combination because the switches are read once."""
    defaults = {"BLOSC_AMD_SINGLE_QUEUE": "0", "BLOSC_AMD_FUSE": "1", "BLOSC_AMD_SPANS": "1", "BLOSC_AMD_SCHED": "1",
                "BLOSC_AMD_PERIODIC": "1"}
    env = dict(os.environ)
    for k, v in defaults.items():
        env[k] = ("1" if v == "0" else "0") if k in flip else v
    env["BLOSC_AMD_LIB"] = os.path.join(ROOT, "tests", "tools", "libblosc_amd_emu.so")
    env["BLOSC_MODE_CHECK_SHRINK"] = "128"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "mode_check.py")], env=env, timeout=900,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "modes ok" in p.stdout, (flip, p.stdout[-2000:], p.stderr[-3000:])


# ---- the reference's OWN test programs (oracle/_ref/ref_suite, built unmodified from the reference's tests where those exist) linked at
#      run time against the emulated library: what tests/test_gpu_ref_suite.py does on the device, here for the programs that are quick
#      enough at emulator speed ----
@pytest.fixture(scope="module")
def ref_programs(emulib, tmp_path_factory):
    bindir = os.path.join(ROOT, "oracle", "_ref", "ref_suite")
    if not os.path.exists(os.path.join(bindir, "test_api")):
        pytest.skip("oracle/_ref/ref_suite is missing (built where the reference's sources exist)")
    libdir = tmp_path_factory.mktemp("libblosc_emu")
    os.symlink(os.path.join(ROOT, "tests", "tools", "libblosc_amd_emu.so"), os.path.join(libdir, "libblosc.so.1"))   # the stock SONAME
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = f"{libdir}:" + env.get("LD_LIBRARY_PATH", "")
    return bindir, env


@pytest.mark.parametrize("prog", ["test_api", "test_maxout", "test_nthreads"])
def test_reference_minunit_programs(ref_programs, prog, tmp_path):
    bindir, env = ref_programs
    p = subprocess.run([os.path.join(bindir, prog)], env=env, cwd=tmp_path, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, errors="replace")
    assert p.returncode == 0 and "ALL TESTS PASSED" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])


def test_reference_bitshuffle_leftovers_and_compat_vectors(ref_programs, tmp_path):
    bindir, env = ref_programs
    # (never the repo root: test_bitshuffle_leftovers.c:24,65 writes two .cdata files into its cwd)
    p = subprocess.run([os.path.join(bindir, "test_bitshuffle_leftovers")], env=env, cwd=tmp_path, timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.count("Successful roundtrip!") == 2, (p.stdout[-1500:], p.stderr[-1500:])
    compat = os.path.join(ROOT, "tests", "golden", "compat")
    names = sorted(f for f in os.listdir(compat) if f.endswith(".cdata"))
    picked = [next(f for f in names if key in f) for key in ("blosclz", "lz4hc", "zlib", "zstd") if any(key in f for f in names)]
    assert len(picked) >= 3
    for f in picked:                                      # compat/filegen.c in decompress mode: 4 MB of arange(10^6, int32) per vector
        p = subprocess.run([os.path.join(bindir, "filegen"), "decompress", os.path.join(compat, f)], env=env, timeout=900,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert p.returncode == 0 and "Decompression successful!" in p.stdout, (f, p.stdout[-500:], p.stderr[-1500:])


def test_tables_kept_on_the_device_serve_only_the_geometry_they_were_made_for(emulib, oracle, ref):
    """Round 6: the block table and the task queues of a call stay on the device, and the next call takes them if ITS block table, fusion flags and
    plane order are the same (engine.hip: EngineState::TableCache) - equal-shaped chunks call after call are the normal case.  Walk one context
    through hits and misses in both directions: the same call twice, other content of the same shape, another typesize, filter, level and size in
    between and back again; every chunk must read everywhere, every decode must return its own plaintext, and equal calls must write equal bytes."""
    n = 3 * 65536 + 123
    a, b = DATASETS["bench19"](n), DATASETS["linspace"](n)
    calls = [(a, 8, 5, 1), (a, 8, 5, 1), (b, 8, 5, 1), (a, 4, 5, 1), (a, 8, 5, 1), (b, 8, 5, 0), (b, 8, 5, 1), (a, 8, 5, 2), (a, 8, 6, 1), (a, 8, 5, 1),
             (a[:n - 8], 8, 5, 1), (a, 8, 5, 1), (b, 8, 5, 1), (b, 8, 1, 1), (b, 8, 5, 1)]
    for cname in (b"lz4", b"blosclz"):
        seen, chunks = {}, []
        for data, T, clevel, shuffle in calls:
            r, chunk = _compress(emulib, data, T, clevel, shuffle, cname)
            assert 0 < r <= data.size + 16, (r, T, clevel, shuffle)
            key = (data.ctypes.data, data.size, T, clevel, shuffle)
            if key in seen:
                assert np.array_equal(seen[key], chunk), ("the same call wrote other bytes", T, clevel, shuffle)
            seen[key] = chunk
            _everybody_reads(emulib, oracle, ref, chunk, data)
            chunks.append((chunk, data))
        # decode in an order of its own: equal geometries with other content back to back, other geometries in between
        for k in (0, 2, 1, 3, 0, 5, 6, 7, 2, 10, 0, 13, 14, 4):
            chunk, data = chunks[k]
            r, out = _decompress(emulib, chunk, data.size)
            assert r == data.size and np.array_equal(out, data), k
        if ref is not None:            # ... and the reference's chunks of the same shapes through the same context
            for data, T, clevel, shuffle in calls[:8]:
                r, chunk = ref_compress(ref, data, T, clevel, shuffle, cname)
                r2, out = _decompress(emulib, chunk[:r], data.size)
                assert r2 == data.size and np.array_equal(out, data), (T, clevel, shuffle)
