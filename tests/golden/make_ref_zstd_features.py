#!/usr/bin/env python3
"""Writes tests/golden/ref_zstd_features.npz: Zstd frames written by the REAL reference's encoder (oracle/_ref/libblosc_ref.so, built by
oracle/Makefile where the reference's sources exist) through its advanced API, chosen so that every optional feature of the frame format
occurs in at least three of them (tests/zstd_feature_checks.py: census, REQUIRED).  ZSTD_compress() at blosc's settings - all the other
fixtures are that - never writes a window descriptor, RLE literals, single-stream Huffman literals, an offset table in repeat mode, ...

Candidates: the inputs of zstd_feature_checks.GENERATORS at a few sizes, levels -5 .. 19, and the switches that change the frame's shape:
targetCBlockSize 1340 (many small blocks: treeless literals, repeat tables), contentSizeFlag 0, seven ZSTD_e_flush pieces through
ZSTD_compressStream2 (no content size, a window descriptor), windowLog 10, literalCompressionMode off, minMatch 3; ZSTD_compressSequences
for a block of more than 0x7F00 sequences.  Every candidate is decoded with the reference's ZSTD_decompress; the selection is greedy, the
smallest frames that fill the census.  Run where oracle/_ref exists:  python tests/golden/make_ref_zstd_features.py"""
import ctypes as C, os, sys
import numpy as np
HERE = os.path.dirname(os.path.abspath(__file__)); ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import ptr, save_golden_npz
from zstd_feature_checks import FIXTURE, MIN_FRAMES, OPTIONAL, REQUIRED, make_input, seq_kernel_frames, walk

R = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libblosc_ref.so"))
sz, vp, i = C.c_size_t, C.c_void_p, C.c_int
class Buf(C.Structure): _fields_ = [("p", vp), ("size", sz), ("pos", sz)]
class Seq(C.Structure): _fields_ = [("offset", C.c_uint), ("litLength", C.c_uint), ("matchLength", C.c_uint), ("rep", C.c_uint)]
R.ZSTD_createCCtx.restype = vp
R.ZSTD_CCtx_reset.argtypes = [vp, i]; R.ZSTD_CCtx_reset.restype = sz
R.ZSTD_CCtx_setParameter.argtypes = [vp, i, i]; R.ZSTD_CCtx_setParameter.restype = sz
R.ZSTD_compress2.argtypes = [vp, vp, sz, vp, sz]; R.ZSTD_compress2.restype = sz
R.ZSTD_compressStream2.argtypes = [vp, C.POINTER(Buf), C.POINTER(Buf), i]; R.ZSTD_compressStream2.restype = sz
R.ZSTD_compressSequences.argtypes = [vp, vp, sz, C.POINTER(Seq), sz, vp, sz]; R.ZSTD_compressSequences.restype = sz
R.ZSTD_decompress.argtypes = [vp, sz, vp, sz]; R.ZSTD_decompress.restype = sz
R.ZSTD_isError.argtypes = [sz]
# zstd.h: ZSTD_cParameter
PARAM = {"level": 100, "wlog": 101, "minmatch": 105, "tcb": 130, "fcs": 200, "lit": 1002, "delim": 1008, "validate": 1009}
CCTX = R.ZSTD_createCCtx()


def ok(r):
    assert not R.ZSTD_isError(r), r
    return r


def compress(data, params):
    """params: 'level=3;tcb=1340;...' (PARAM's names; lit=2 is ZSTD_ps_disable); flush=k: ZSTD_compressStream2 in k ZSTD_e_flush pieces and
    a ZSTD_e_end; stream=1: ZSTD_compressStream2 with one ZSTD_e_end; seqs=1: ZSTD_compressSequences, a match of 3 bytes at distance 3
    behind the first three literals, over and over; seqs=2;ll=k: ZSTD_compressSequences, k literals and one match at distance 1 for the rest"""
    kv = dict(p.split("=") for p in params.split(";"))
    ok(R.ZSTD_CCtx_reset(CCTX, 3))                                       # ZSTD_reset_session_and_parameters
    for k, v in kv.items():
        if k in PARAM: ok(R.ZSTD_CCtx_setParameter(CCTX, PARAM[k], int(v)))
    n = data.size
    out = np.zeros(n + n // 2 + 1024, np.uint8)
    if "seqs" in kv:
        if kv["seqs"] == "1":
            m = (n - 3) // 3
            seqs = (Seq * m)()
            for k in range(m):
                seqs[k].offset, seqs[k].litLength, seqs[k].matchLength = 3, 3 if k == 0 else 0, 3
        else:                                                            # constant input: ll literals, the rest one match at distance 1
            m = 1
            seqs = (Seq * 1)()
            seqs[0].offset, seqs[0].litLength, seqs[0].matchLength = 1, int(kv["ll"]), n - int(kv["ll"])
        r = ok(R.ZSTD_compressSequences(CCTX, ptr(out), out.size, seqs, m, ptr(data), n))
    elif "flush" in kv or "stream" in kv:
        pieces = int(kv.get("flush", 0))
        cuts = [n * (k + 1) // (pieces + 1) for k in range(pieces)] + [n]
        ib, ob = Buf(data.ctypes.data, 0, 0), Buf(out.ctypes.data, out.size, 0)
        for k, cut in enumerate(cuts):
            ib.size = cut
            while True:
                left = ok(R.ZSTD_compressStream2(CCTX, C.byref(ob), C.byref(ib), 2 if k == len(cuts) - 1 else 1))     # ZSTD_e_end / ZSTD_e_flush
                if left == 0 and ib.pos == ib.size: break
        r = ob.pos
    else:
        r = ok(R.ZSTD_compress2(CCTX, ptr(out), out.size, ptr(data), n))
    frame = out[:r].copy()
    back = np.zeros(n, np.uint8)
    assert R.ZSTD_decompress(ptr(back), n, ptr(frame), r) == n and np.array_equal(back, data), "the reference does not read its own frame"
    return frame


def candidates():
    """(recipe, frame, classes, nseq) of everything the selection may take"""
    SWITCHES = ["", "tcb=1340", "stream=1;fcs=0", "flush=7;wlog=10", "flush=7;wlog=10;tcb=1340", "lit=2", "lit=2;tcb=1340;fcs=0;stream=1", "minmatch=3",
                "flush=7;wlog=10;lit=2"]
    todo = []
    for gen, seed in (("bench19", 0), ("linspace", 0), ("smallints", 7), ("randwalk", 42)):
        for n in (1000, 20000, 131072, 300001):
            for level in (-5, 1, 3, 9, 19):
                if n > 131072 and level == 19 and gen != "bench19": continue       # (large frames: one data set is enough)
                todo += [(gen, n, seed, f"level={level}" + (";" + s if s else "")) for s in SWITCHES]
    for gen in ("bits1", "bits2", "const", "text", "tokens"):
        for n in (200, 1000, 20000):
            for seed in (1, 2, 3):
                for level in (-5, 3, 19):
                    todo += [(gen, n, seed, f"level={level}" + (";" + s if s else "")) for s in SWITCHES[:5] + SWITCHES[7:8]]
    todo += [("period3", 131072, s, "level=3;minmatch=3;seqs=1") for s in (1, 2, 3)]           # 43 689 sequences in one block: the 3-byte count
    # RLE literals.  In one block: constant input, the literals spelled out (left alone the encoder writes an RLE block);
    # in a later block: single bytes of one value between matches into the block before
    todo += [("const", n, 170 + n % 7, f"level=3;seqs=2;ll={ll}") for n in (1000, 20000) for ll in (20, 100, 300)]
    todo += [("rlelit", n, s, f"level={lv};flush=1") for n in (1000, 20000) for s in (1, 2) for lv in (3, 19)]
    # both sides of the two-phase path's limit nseq <= out_size / 8, at one size that is a multiple of 8 (tests: the seq_overflow boundary)
    todo += [("sparse", 1024, s, "level=19") for s in range(128)] + [("tokens", 1024, s, "level=19;minmatch=3") for s in range(10, 40)]
    for gen, n, seed, params in todo:
        data = make_input(gen, n, seed)
        frame = compress(data, params)
        w = walk(frame, n)
        yield f"{gen},{n},{seed},{params}", frame, w["classes"], w["nseq"]


def select(cands):
    need = {c: MIN_FRAMES for c in REQUIRED + OPTIONAL}
    have = set(c for _, _, cl, _ in cands for c in cl)
    for c in list(need):
        if c not in have:
            print("NOT REACHED:", c); del need[c]
    picked = []
    def take(k):
        picked.append(k)
        for c in cands[k][2]:
            if need.get(c, 0) > 0: need[c] -= 1
    # the boundary of the two-phase path's sequence limit first: nseq == 128, 127 and the smallest count above, at 1024 bytes
    edge = {}
    for k, (rec, fr, cl, ns) in enumerate(cands):
        if rec.split(",")[1] == "1024" and "two_phase_shape" in cl:
            edge.setdefault(ns[0], k)
    for want in (128, 127, min((v for v in edge if v > 128), default=None)):
        if want in edge: take(edge[want])
        else: print("BOUNDARY NOT REACHED: nseq", want)
    # RLE literals on the general path too (a later block of a frame), and one frame of several full-size blocks
    for want in (lambda rec, cl: rec.startswith("rlelit,") and "lit_rle" in cl, lambda rec, cl: rec.split(",")[1] == "300001" and "multi_block" in cl):
        take(min((k for k in range(len(cands)) if want(cands[k][0], cands[k][2])), key=lambda k: cands[k][1].size))
    while any(v > 0 for v in need.values()):
        def gain(k):
            rec, fr, cl, ns = cands[k]
            g = sum(1 for c in cl if need.get(c, 0) > 0)
            n = int(rec.split(",")[1])
            cost = fr.size + 200 + (4000 if n > 65536 else 0) + (20000 if fr.size > 20000 else 0)     # small frames, and small inputs: the emulator decodes them too
            return g / cost
        k = max((k for k in range(len(cands)) if k not in picked), key=gain)
        assert gain(k) > 0
        take(k)
    # split blocks want, at one size, four or more frames of both shapes (zstd_feature_checks.plane_groups)
    return sorted(picked, key=lambda k: (int(cands[k][0].split(",")[1]), k))


if __name__ == "__main__":
    cands = list(candidates())
    picked = select(cands)
    out, recipes = {}, []
    for j, k in enumerate(picked):
        rec, fr, cl, ns = cands[k]
        out[f"f{j}"] = fr; recipes.append(rec)
    out["recipes"] = np.array(recipes)
    save_golden_npz(FIXTURE, out)
    count = {}
    for k in picked:
        for c in cands[k][2]: count[c] = count.get(c, 0) + 1
    print(len(picked), "frames,", sum(cands[k][1].size for k in picked), "bytes; largest frame", max(cands[k][1].size for k in picked))
    print("two-phase frames with sequences:", sum(seq_kernel_frames(cands[k][2], cands[k][3]) for k in picked))
    for c in sorted(count): print(f"  {c:22s} {count[c]}")
    sizes = {}
    for k in picked: sizes.setdefault(cands[k][0].split(",")[1], []).append(seq_kernel_frames(cands[k][2], cands[k][3]))
    print({n: (len(v), sum(v)) for n, v in sizes.items()})
