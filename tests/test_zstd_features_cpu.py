"""CPU: the census of tests/golden/ref_zstd_features.npz - frames the reference's encoder wrote through its advanced API
(tests/golden/make_ref_zstd_features.py) - read from the frames' headers alone (zstd_feature_checks.walk, RFC 8878 3.1.1): every optional
feature of the format in at least three frames, so that the decoder tests that draw on the fixture (oracle, zstd_serial.h, the emulated
library, the device) visit every branch with valid input."""
import numpy as np

from zstd_feature_checks import MIN_FRAMES, OPTIONAL, REQUIRED, census, fixture, make_input, plane_groups, walk


def test_every_format_feature_in_three_frames():
    entries = fixture()
    count = {}
    for e in entries:
        assert e.n >= 128 and census(e.frame, e.n) == e.classes
        for c in e.classes:
            count[c] = count.get(c, 0) + 1
    print(sorted(count.items()))
    short = {c: count.get(c, 0) for c in REQUIRED if count.get(c, 0) < MIN_FRAMES}
    assert not short, short
    assert all(count.get(c, 0) >= 1 for c in OPTIONAL), count
    # the classes this library's decoder rejects outright stay out of the fixture (tests/golden/README.md)
    assert "dictionary_id" not in count and "checksum" not in count


def test_recipes_name_their_inputs():
    for e in fixture():
        gen, n, seed = e.recipe.split(",")[:3]
        assert np.array_equal(make_input(gen, n, seed), e.plain) and e.n == int(n)


def test_header_walker_on_a_frame_spelled_out_by_hand():
    """a raw block and an RLE block behind a window descriptor, no content size: every field the walker reads, written out byte by byte"""
    f = bytes([0x28, 0xB5, 0x2F, 0xFD, 0x00, 0x58]) + bytes([5 << 3 | 0, 0, 0]) + b"hello" + bytes([200 << 3 & 0xff | 2 | 1, 200 >> 5, 0, 0x41])
    w = walk(np.frombuffer(f, np.uint8), 205)
    assert w["classes"] == {"window_descriptor", "fcs_flag0", "block_raw", "block_rle", "multi_block"} and w["fcs"] is None
    assert [(b["type"], b["body"], b["size"]) for b in w["blocks"]] == [(0, 9, 5), (1, 17, 1)]


def test_the_sequence_limit_has_a_frame_on_either_side_and_one_on_it():
    """one decoded size that is a multiple of 8; nseq == size / 8 (still k_zstd_seq's), one fewer, and more (handed to the general path)"""
    es = [e for e in fixture() if e.n == 1024 and "two_phase_shape" in e.classes]
    nseq = sorted(e.nseq[0] for e in es)
    assert 128 in nseq and 127 in nseq and any(v > 128 for v in nseq), nseq
    for e in es:
        assert ("seq_overflow" in e.classes) == (e.nseq[0] > 128)


def test_split_blocks_can_mix_both_shapes():
    for T in (4, 8):
        groups = plane_groups(fixture(), T)
        assert any(0 < sum(e.seq_kernel for e in g) < T for g in groups), T
