"""GPU: Zstd decode of tests/golden/ref_zstd_features.npz - frames the reference's own encoder wrote through its advanced API, every optional
feature of the format in at least three of them (tests/test_zstd_features_cpu.py has the census; ZSTD_compress() at blosc's settings, which
wrote every other fixture, leaves most of them out).  Both device paths side by side: k_zstd_entropy / k_zstd_seq / k_zstd_exec for frames
of one compressed block, k_zstd_streams for the rest - several blocks, raw and RLE blocks, treeless literals, repeat tables, more sequences
than the two-phase path's scratch holds.  Yardsticks: the fixture's plain bytes and the oracle's orc_decompress on the same chunk.  The
checkers are tests/zstd_feature_checks.py's; tests/test_emu_zstd_features.py runs them on the emulated library."""
import numpy as np
import pytest

from getitem_ranges_checks import TorchMem
from zstd_feature_checks import (DAMAGE_SEED, DeviceSide, check_batch, check_getitem, check_planes, check_single, check_verdict, damage_cases, fixture, wrap_frame)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(pkg, lib):
    return DeviceSide(pkg, lib, TorchMem())


def test_every_frame_in_a_call_of_its_own(dec, oracle):
    check_single(dec, oracle, fixture())


@pytest.mark.parametrize("shuffled", [False, True], ids=["fixture-order", "shuffled"])
def test_all_frames_in_one_batch(dec, oracle, shuffled):
    """two-phase and general-path frames side by side in one launch; 256 guard bytes around every destination, the buffer compared whole"""
    es = fixture()
    order = [int(k) for k in np.random.default_rng(77).permutation(len(es))] if shuffled else list(range(len(es)))
    check_batch(dec, oracle, [wrap_frame(e.frame, e.n) for e in es], [e.plain for e in es], order, ("batch", "shuffled" if shuffled else "fixture order"))


@pytest.mark.parametrize("T", [4, 8])
def test_split_blocks_whose_planes_are_frames_of_both_shapes(dec, oracle, T):
    groups = check_planes(dec, oracle, fixture(), T)
    assert any(0 < sum(e.seq_kernel for e in g) < T for g in groups)


def test_getitem_on_every_frame(dec):
    check_getitem(dec, fixture())


def test_the_sequence_limit_of_the_two_phase_path(dec, oracle):
    """nseq == out_size / 8 and one fewer stay with k_zstd_seq, one more is handed to k_zstd_streams: the same bytes either way, alone and
    as three planes (and a fourth) of one block"""
    es = sorted((e for e in fixture() if e.n == 1024 and "two_phase_shape" in e.classes), key=lambda e: e.nseq[0])
    assert [e.nseq[0] for e in es][:2] == [127, 128] and es[2].nseq[0] > 128
    check_single(dec, oracle, es)
    check_planes(dec, oracle, es + es[:1], 4)


def test_damaged_headers_get_the_oracles_verdict(dec, oracle):
    """single-bit flips in the literals header, the Huffman description, the sequence count, the modes byte and the table descriptions of one
    frame per census class (at most 400 cases, the ones tests/test_emu_zstd_features.py has taken through the CPU decoders): the oracle's
    verdict, and its bytes where it accepts"""
    cases = damage_cases(fixture(), DAMAGE_SEED)
    accepted = sum(check_verdict(dec.decompress, oracle, c) for c in cases)
    assert 0 < accepted < len(cases)
