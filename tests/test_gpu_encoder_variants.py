"""Every mode of k_encode_streams_t on the device, through blosc_compress_ctx on host buffers: the switches that select the mode lead to
exactly one launch, counted under the mode's profile name and under none of the other three, and the chunk decodes to the input - through
the oracle and, where oracle/_ref is built, through stock c-blosc.  Inputs and cases are tests/encoder_variant_checks.py's, one case per
mode.  The device's bytes are not compared with the emulator's recorded ones (tests/test_emu_encoder_variants.py): include/blosc_gpu_params.h
promises deterministic bytes on the device for blosclz, lz4 and zstd up to clevel 5 only."""
import numpy as np
import pytest

import encoder_variant_checks as ev
from helpers import DATASETS, header, orc_decompress, ref_decompress

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs():
    return [(np.ascontiguousarray(DATASETS[d](n)), T, shuffle) for d, n, T, shuffle in ev.INPUTS]


def test_one_case_per_mode():
    assert [c["mode"] for c in ev.one_case_per_mode()] == list(ev.MODES)


@pytest.mark.parametrize("case", ev.one_case_per_mode(), ids=lambda c: c["mode"])
def test_the_switches_launch_their_mode(lib, oracle, ref, inputs, case):
    want = {name: int(name == ev.profile_name(case["mode"])) for name in ev.PROFILE_NAMES}
    for data, T, shuffle in inputs:
        r, chunk, launches = ev.run_case(lib, case, data, T, shuffle)
        assert launches == want, (case["mode"], launches)
        assert 0 < r <= data.size + 16 and header(chunk)["cbytes"] == r and header(chunk)["nbytes"] == data.size
        ro, out = orc_decompress(oracle, chunk, data.size)
        assert ro == data.size and np.array_equal(out, data), "the oracle cannot read it"
        if ref is not None:
            rr, out = ref_decompress(ref, chunk, data.size)
            assert rr == data.size and np.array_equal(out, data), "stock c-blosc cannot read it"
