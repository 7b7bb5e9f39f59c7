"""Device twin of tests/test_emu_lz4_emit_scratch.py: the same one-stream chunks (tests/lz4_emit_scratch_cases.py) through the product on the GPU - host
buffers, the stock C ABI.  Every chunk decodes with the reference, the oracle and the library itself, and equals the parent commit's, size and crc32
(tests/golden/lz4_emit_scratch_parent_gpu.json, recorded from the parent commit's product on an MI355X; tests/lz4_emit_scratch_cases.py says why the
emulator's file is another)."""
import json
import os

import numpy as np
import pytest

from helpers import orc_decompress, ptr, ref_decompress
from lz4_emit_scratch_cases import CLEVELS, KINDS, SIZES, case_key, compress_host, make_case, same_bytes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(ROOT, "tests", "golden", "lz4_emit_scratch_parent_gpu.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("clevel", CLEVELS)
def test_chunks_decode_and_equal_the_parents(lib, oracle, ref, parent, clevel, kind):
    for n in SIZES:
        data = make_case(kind, clevel, n)
        r, chunk = compress_host(lib, data, clevel)
        assert 0 < r <= n + 16, (n, r)
        if ref is not None:
            rr, out = ref_decompress(ref, chunk, n)
            assert rr == n and np.array_equal(out, data), f"n = {n}: stock c-blosc cannot read it"
        ro, out = orc_decompress(oracle, chunk, n)
        assert ro == n and np.array_equal(out, data), f"n = {n}: the oracle cannot read it"
        back = np.full(n + 64, 0xEE, np.uint8)
        assert lib.blosc_decompress_ctx(ptr(chunk), ptr(back), n, 1) == n and np.array_equal(back[:n], data) and np.all(back[n:] == 0xEE), f"n = {n}: our own decoder cannot read it"
        assert same_bytes(chunk, parent[case_key(clevel, kind, n)]), f"n = {n}: the compressed bytes differ from the parent commit's"
