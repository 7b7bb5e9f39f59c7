"""The encoder variants behind blosc_compress_ctx: which switches lead to which mode of k_encode_streams_t (k_encode.hip: the mode table),
shared by tests/test_emu_encoder_variants.py (bytes and launches pinned on the emulated library), tests/test_gpu_encoder_variants.py (one
case per mode on the device) and tests/golden/make_encoder_variants.py (the generator of the pinned answers).

Every variant writes a valid stream, so a round trip cannot tell a launch of the wrong kernel; the chunk's bytes and the profile name the
launch is counted under can."""
import ctypes as C
import hashlib
import os

import numpy as np

from helpers import DATASETS, ptr

# the six switches encoder_variant() reads, on every call (engine.hip)
SWITCHES = ("BLOSC_AMD_LZ4HC", "BLOSC_AMD_ZSTD_TABLES", "BLOSC_AMD_ZSTD_SEARCH", "BLOSC_AMD_ZSTD_HUFFMAN", "BLOSC_AMD_ZLIB_SEARCH", "BLOSC_AMD_ZLIB_DYNAMIC")
# the names a launch of k_encode_streams_t is counted under (blosc_gpu_profile_get)
PROFILE_NAMES = ("k_encode_streams", "k_lz4hc_encode", "k_zstd_encode", "k_zlib_encode")
PROFILE_OF_FAMILY = {"LZ": "k_encode_streams", "HC": "k_lz4hc_encode", "ZSTD": "k_zstd_encode", "ZLIB": "k_zlib_encode"}

# (dataset, bytes, typesize, shuffle)
INPUTS = (("bench19", 40000, 8, 1), ("smallints", 24000, 4, 1))


def _case(cname, clevel, mode, **env):
    return {"cname": cname, "clevel": clevel, "mode": mode, "env": {"BLOSC_AMD_" + k: str(v) for k, v in env.items()}}


# codec, clevel, the mode the switches select, the switches set (every other one is unset: its default)
CASES = (
    _case("lz4", 1, "ENC_LZ"), _case("lz4", 5, "ENC_LZ"), _case("lz4", 9, "ENC_LZ"),
    _case("blosclz", 5, "ENC_LZ"), _case("blosclz", 9, "ENC_LZ"),
    _case("lz4hc", 5, "ENC_HC"), _case("lz4hc", 5, "ENC_LZ", LZ4HC=0),
    _case("zstd", 3, "ENC_ZSTD_T"), _case("zstd", 5, "ENC_ZSTD_T"), _case("zstd", 6, "ENC_ZSTD_HC"), _case("zstd", 7, "ENC_ZSTD_HC"), _case("zstd", 9, "ENC_ZSTD_HC"),
    _case("zstd", 3, "ENC_ZSTD", ZSTD_TABLES=0), _case("zstd", 3, "ENC_ZSTD_TH", ZSTD_HUFFMAN=1),
    _case("zstd", 3, "ENC_ZSTD", ZSTD_TABLES=0, ZSTD_HUFFMAN=1),          # Huffman literals count only with tables or search
    _case("zstd", 3, "ENC_ZSTD_HC", ZSTD_SEARCH=1, ZSTD_TABLES=0),        # search implies tables
    _case("zstd", 7, "ENC_ZSTD_HCH", ZSTD_HUFFMAN=1), _case("zstd", 7, "ENC_ZSTD_T", ZSTD_SEARCH=0),
    _case("zlib", 5, "ENC_ZLIB", ZLIB_SEARCH=0, ZLIB_DYNAMIC=0), _case("zlib", 5, "ENC_ZLIB_HC", ZLIB_SEARCH=1, ZLIB_DYNAMIC=0),
    _case("zlib", 5, "ENC_ZLIB_DYN", ZLIB_SEARCH=0, ZLIB_DYNAMIC=1), _case("zlib", 5, "ENC_ZLIB_DYN_HC", ZLIB_SEARCH=1, ZLIB_DYNAMIC=1),
)
MODES = ("ENC_LZ", "ENC_ZSTD", "ENC_ZLIB", "ENC_HC", "ENC_ZSTD_T", "ENC_ZSTD_HC", "ENC_ZLIB_HC", "ENC_ZSTD_TH", "ENC_ZSTD_HCH", "ENC_ZLIB_DYN", "ENC_ZLIB_DYN_HC")


def case_id(case):
    return f"{case['cname']}-{case['clevel']}" + "".join(f"-{k[10:].lower()}={v}" for k, v in case["env"].items())


def profile_name(mode):
    """the profile name of a mode's launch: the writer family's, the LZ family split by the search"""
    return PROFILE_OF_FAMILY["ZSTD" if "ZSTD" in mode else ("ZLIB" if "ZLIB" in mode else mode[4:])]


def one_case_per_mode():
    """the first case of every mode, in the modes' order"""
    return tuple(next(c for c in CASES if c["mode"] == m) for m in MODES)


def declare(L):
    sz, i, vp = C.c_size_t, C.c_int, C.c_void_p
    L.blosc_compress_ctx.argtypes = [i, i, sz, sz, vp, vp, sz, C.c_char_p, sz, i]
    L.blosc_compress_ctx.restype = i
    L.blosc_gpu_profile.argtypes = [i]; L.blosc_gpu_profile.restype = None
    L.blosc_gpu_profile_reset.argtypes = []; L.blosc_gpu_profile_reset.restype = None
    L.blosc_gpu_profile_get.argtypes = [C.c_char_p, C.POINTER(C.c_double), C.POINTER(i)]; L.blosc_gpu_profile_get.restype = i
    return L


class switches:
    """the six switches as `env` names them and nothing else, for the block; whatever the process had comes back behind it"""
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.pop(k, None) for k in SWITCHES}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def run_case(L, case, data, T, shuffle):
    """(return value, chunk, launches per profile name) of one blosc_compress_ctx call, blocksize 0, under the case's switches"""
    out = np.full(data.size + 16 + 64, 0xEE, np.uint8)
    with switches(case["env"]):
        L.blosc_gpu_profile(1)
        L.blosc_gpu_profile_reset()
        try:
            r = L.blosc_compress_ctx(case["clevel"], shuffle, T, data.size, ptr(data), ptr(out), data.size + 16, case["cname"].encode(), 0, 1)
            launches = {}
            for name in PROFILE_NAMES:
                ms, cnt = C.c_double(0), C.c_int(0)
                L.blosc_gpu_profile_get(name.encode(), C.byref(ms), C.byref(cnt))
                launches[name] = int(cnt.value)
        finally:
            L.blosc_gpu_profile(0)
    assert np.all(out[data.size + 16:] == 0xEE), "wrote past destsize"
    return int(r), out[:max(r, 0)].copy(), launches


def collect(L):
    """what tests/golden/encoder_variants.json records: per case and input the return value, the chunk's sha256 and the launches per name"""
    declare(L)
    inputs = [(np.ascontiguousarray(DATASETS[d](n)), T, shuffle) for d, n, T, shuffle in INPUTS]
    answers = []
    for case in CASES:
        runs = []
        for (dname, n, _, _), (data, T, shuffle) in zip(INPUTS, inputs):
            r, chunk, launches = run_case(L, case, data, T, shuffle)
            runs.append({"input": f"{dname}({n})", "ret": r, "sha256": hashlib.sha256(chunk.tobytes()).hexdigest(), "launches": launches})
        answers.append({"case": case_id(case), "mode": case["mode"], "runs": runs})
    return {"cases": answers}
