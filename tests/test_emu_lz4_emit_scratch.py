"""CPU, wavefront emulator: the parallel LZ4 step (enc_lz4p.h) hands its sequences from the rank lanes to the byte lanes through 64 words of LDS - one
per position of a 64-position step (clevel 9), one per PAIR of positions of a 128-position step (clevel 5).  One LZ4 stream per chunk, sized around the
steps, with inputs that fill the rank lanes, leave them empty, run one match across the steps, start matches on odd positions and end them on the
step's, the stream's and the last start's boundaries (tests/lz4_emit_scratch_cases.py).  Every chunk decodes with the reference (oracle/_ref, where it
is built), the oracle and the library's own decoder, and equals - size and crc32 - what the encoder wrote when the hand-over still had a word per
position (tests/golden/lz4_emit_scratch_parent.json): the parse did not change.  tests/test_gpu_lz4_emit_scratch.py runs the same cases on the device."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from helpers import orc_decompress, ptr, ref_decompress
from lz4_emit_scratch_cases import CLEVELS, KINDS, SIZES, case_key, compress_host, declare, make_case, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.fixture(scope="module")
def emulib():
    if not os.path.exists(CLANG):
        pytest.skip("needs the ROCm clang++")
    csrc = os.path.join(ROOT, "c-blosc_amd", "csrc")
    tools = os.path.join(ROOT, "tests", "tools")
    so = os.path.join(tools, "libblosc_amd_emu.so")
    deps = [os.path.join(tools, "blosc_emu_lib.cpp"), os.path.join(tools, "wave_emu", "wave_emu.h"), os.path.join(tools, "wave_emu", "hip_emu_runtime.h")]
    deps += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith((".hip", ".h"))]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):      # (as tests/test_emu_library.py builds it)
        subprocess.check_call([CLANG, "-std=c++17", "-O1", "-shared", "-fPIC", "-w", "-I", os.path.join(tools, "wave_emu"), "-I", csrc,
                               "-I", os.path.join(ROOT, "include"), "-x", "c++", deps[0], "-o", so, "-lpthread"])
    return declare(C.CDLL(so))


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "lz4_emit_scratch_parent.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clevel", CLEVELS)
def test_chunks_decode_and_equal_the_parents(emulib, oracle, ref, parent, clevel, kind):
    for n in SIZES:
        data = make_case(kind, clevel, n)
        r, chunk = compress_host(emulib, data, clevel)
        assert 0 < r <= n + 16, (n, r)
        if ref is not None:
            rr, out = ref_decompress(ref, chunk, n)
            assert rr == n and np.array_equal(out, data), f"n = {n}: stock c-blosc cannot read it"
        ro, out = orc_decompress(oracle, chunk, n)
        assert ro == n and np.array_equal(out, data), f"n = {n}: the oracle cannot read it"
        back = np.full(n + 64, 0xEE, np.uint8)
        assert emulib.blosc_decompress_ctx(ptr(chunk), ptr(back), n, 1) == n and np.array_equal(back[:n], data) and np.all(back[n:] == 0xEE), f"n = {n}: our own decoder cannot read it"
        assert same_bytes(chunk, parent[case_key(clevel, kind, n)]), f"n = {n}: the compressed bytes differ from the parent commit's"


def test_the_cases_reach_the_encoder(parent):
    """what the fingerprints are worth: the chunks of the structured inputs are real LZ4 streams (smaller than a plain copy) from 255 bytes up"""
    for clevel in CLEVELS:
        for kind in KINDS:
            if kind == "random":
                continue
            for n in (4097, 65549):
                assert parent[case_key(clevel, kind, n)][0] < n, (clevel, kind, n)
