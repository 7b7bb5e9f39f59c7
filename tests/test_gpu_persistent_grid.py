"""The persistent kernels (k_encode_streams_t in its modes, k_decode_streams, the Zstd and zlib decoders) are launched with as many
one-wave workgroups per CU as the runtime says stay resident - its occupancy figure, asked once per kernel, which knows the registers the compiler used
and the granules the device hands LDS out in.  A grid above it has workgroups that start when the first ones leave and find the queues empty; a grid
below it - or a kernel whose LDS misses a granule boundary by a little - leaves wave slots empty for the whole launch.
blosc_internal_persistent_grids reports, per kernel, what the engine launches and what the runtime answers."""
import ctypes as C

import numpy as np
import pytest

from helpers import DATASETS, header, ptr

pytestmark = pytest.mark.gpu
KERNELS = 15      # the eleven modes of the encode kernel, k_decode_streams, k_zstd_exec, k_zstd_streams, k_zlib_streams


def _grids(lib):
    lib.blosc_internal_persistent_grids.argtypes = [C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    names, launched, occupancy = (C.c_char_p * 32)(), (C.c_int * 32)(), (C.c_int * 32)()
    n = lib.blosc_internal_persistent_grids(32, names, launched, occupancy)
    assert n == KERNELS, n
    return [(names[i].decode(), launched[i], occupancy[i]) for i in range(n)]


def _launches(pkg):
    return sum(pkg.profile_get(k)[1] for k in ("k_shuffle", "k_bitshuffle", "k_encode_streams", "k_lz4hc_encode", "k_zstd_encode", "k_zlib_encode", "k_chunk_scan",
                                               "k_chunk_compact", "k_decode_plan", "k_decode_streams", "k_zstd_streams", "k_zlib_streams", "k_unshuffle", "k_copy_chunks"))


def test_every_grid_is_the_runtimes_occupancy(lib, pkg):
    lib.blosc_gpu_profile(1)
    lib.blosc_gpu_profile_reset()
    try:
        table = _grids(lib)
        again = _grids(lib)
        assert _launches(pkg) == 0, "the query launched a kernel"
    finally:
        lib.blosc_gpu_profile(0)
    assert table == again
    for name, launched, occupancy in table:
        print(f"{name}: {launched} workgroups per CU launched, occupancy {occupancy}")
    assert len({name for name, _, _ in table}) == KERNELS
    for name, launched, occupancy in table:
        assert 0 < launched <= 32, (name, launched)
        assert launched == occupancy, f"{name}: the engine launches {launched} workgroups per CU, the runtime keeps {occupancy} resident"
    by_name = {name: launched for name, launched, _ in table}
    assert by_name["k_encode_streams_t<ENC_LZ>"] == 24      # 6400 bytes of LDS = 5 granules of 1280, 80 registers: the figure DESIGN.md 3.3 counts on


def test_a_small_compress_takes_every_task_once(lib):
    """8 split blocks of typesize 8: 64 streams and - the byte shuffle runs inside the encode kernel - 8 shuffle tasks; the waves count what they took
    into plane_cost[256], and no workgroup that came too late or too many changes the sum"""
    lib.blosc_internal_last_compress_tasks.argtypes = [C.POINTER(C.c_uint)]
    lib.blosc_internal_last_compress_tasks.restype = None
    probe = DATASETS["bench19"](1 << 18)
    out = np.zeros(probe.size + 16, np.uint8)
    assert lib.blosc_compress_ctx(5, 1, 8, probe.size, ptr(probe), ptr(out), out.size, b"lz4", 4096, 1) > 0
    bs = header(out)["blocksize"]
    data = DATASETS["bench19"](8 * bs)
    out = np.zeros(data.size + 16, np.uint8)
    r = lib.blosc_compress_ctx(5, 1, 8, data.size, ptr(data), ptr(out), out.size, b"lz4", 4096, 1)
    assert r > 0 and header(out)["blocksize"] == bs
    t = (C.c_uint * 3)()
    lib.blosc_internal_last_compress_tasks(t)
    taken, streams, shuffles = t[0], t[1], t[2]
    print(f"tasks taken {taken}, streams {streams}, shuffle tasks {shuffles}")
    assert streams == 64 and shuffles in (0, 8)      # (0: a device without the per-XCD queues shuffles in a kernel of its own)
    assert taken == streams + shuffles
    back = np.zeros(data.size, np.uint8)
    assert lib.blosc_decompress_ctx(ptr(out), ptr(back), data.size, 1) == data.size and np.array_equal(back, data)
