"""CPU: tests/golden/ref_zstd_features.npz - reference-written Zstd frames with every optional feature of the format - through the emulated
library (tests/test_emu_library.py's build: the host engine and every kernel on the wavefront emulator), with the checkers
tests/test_gpu_zstd_features.py runs on the device (tests/zstd_feature_checks.py).  The frames that decode to 64 KiB or less, one frame per
chunk and as planes of split blocks; k_zstd_seq's counter says that the two-phase path took exactly the frames of its shape, every other
frame decoding all the same says that the general path took the rest.  The damaged-header cases of the device test run here first, through
tests/tools/zstd_serial_frame.cpp and through the emulated library."""
import ctypes as C

import numpy as np

from batch_bounds_checks import declare
from getitem_ranges_checks import NumpyMem
from helpers import ptr
from test_emu_library import FULL, SOAK, emulib  # noqa: F401  (the fixture; SOAK moves with BLOSC_EMU_SEED, FULL is BLOSC_EMU_FULL=1)
from test_zstd_serial_cpu import zs  # noqa: F401  (the fixture)
from zstd_feature_checks import (DAMAGE_SEED, EMU_MAX, EmuSide, check_batch, check_getitem, check_planes, check_single, check_verdict, damage_cases, fixture,
                                 wrap_frame)


def _small():
    return [e for e in fixture() if e.n <= EMU_MAX]


def _seq_frames(L):
    c = (C.c_ulonglong * 5)(); L.emu_zstd_path_counts(c)
    return int(c[3])


def test_one_frame_per_chunk_takes_the_path_of_its_shape(emulib, oracle):
    dec = EmuSide(declare(emulib), NumpyMem())
    es = _small()
    assert any(e.seq_kernel for e in es) and any("seq_overflow" in e.classes for e in es) and any("multi_block" in e.classes for e in es)
    before = _seq_frames(emulib)
    check_single(dec, oracle, es)
    assert _seq_frames(emulib) - before == sum(e.seq_kernel for e in es)
    # ... and all of them in ONE launch, in fixture order and in an order of the seed's
    chunks, plains = [wrap_frame(e.frame, e.n) for e in es], [e.plain for e in es]
    for order in (list(range(len(es))), [int(k) for k in np.random.default_rng(5 + SOAK).permutation(len(es))]):
        before = _seq_frames(emulib)
        check_batch(dec, oracle, chunks, plains, order, ("emulated batch", order[:4]))
        assert _seq_frames(emulib) - before == sum(e.seq_kernel for e in es)


def test_planes_of_split_blocks_mix_both_shapes(emulib, oracle):
    dec = EmuSide(declare(emulib), NumpyMem())
    for T in (4, 8):
        before = _seq_frames(emulib)
        groups = check_planes(dec, oracle, _small(), T)
        assert any(0 < sum(e.seq_kernel for e in g) < T for g in groups), "no block with planes of both shapes"
        assert _seq_frames(emulib) - before == sum(e.seq_kernel for g in groups for e in g)


def test_getitem_on_every_frame(emulib):
    check_getitem(EmuSide(declare(emulib), NumpyMem()), _small())


def test_damaged_headers_get_the_oracles_verdict(emulib, zs, oracle):
    """single-bit flips in the first 24 bytes of each block body, one frame per census class, at most 400 cases - the cases
    tests/test_gpu_zstd_features.py sends to the device, here through the serial primitives (all of them) and through the emulated library
    (with BLOSC_EMU_FULL=1 all of them - some six minutes, clean when the cases were drawn; by default those of the frames that decode to
    64 KiB or less)"""
    oracle.orc_zstd_decompress.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    dec = EmuSide(declare(emulib), NumpyMem())
    cases = damage_cases(fixture(), DAMAGE_SEED)
    assert 200 <= len(cases) <= 400
    accepted = emulated = 0
    for e, pos, bit in cases:
        src = np.empty(e.frame.size, np.uint8); src[:] = e.frame; src[pos] ^= 1 << bit
        a = np.zeros(e.n, np.uint8); b = np.zeros(e.n, np.uint8)
        ra = oracle.orc_zstd_decompress(ptr(src), src.size, ptr(a), e.n)
        rb = zs.zs_decompress(ptr(src), src.size, ptr(b), e.n)
        assert (ra == e.n) == (rb == e.n), (e, pos, bit, ra, rb)
        if ra == e.n:
            assert np.array_equal(a, b), (e, pos, bit)
        if FULL or e.n <= EMU_MAX:
            emulated += 1
            accepted += check_verdict(dec.decompress, oracle, (e, pos, bit))
    assert 0 < accepted < emulated and emulated * 2 >= len(cases), (accepted, emulated)
