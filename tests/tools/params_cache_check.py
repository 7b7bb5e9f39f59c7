"""Child process of tests/test_emu_params.py::test_table_cache_and_feedback: the library named by BLOSC_AMD_LIB (the emulator build, where
"device" memory is the host's) compresses a homogeneous batch twice, a heterogeneous one twice, and the homogeneous one twice again.  With
BLOSC_AMD_DEBUG_COST set the engine says on stderr whether each call found its tables on the device; this script checks the bytes and
prints 'cache ok'."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import DATASETS  # noqa: E402

spec = importlib.util.spec_from_file_location("c_blosc_amd", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
pkg = importlib.util.module_from_spec(spec); spec.loader.exec_module(pkg)
L = pkg.load()

hosts = [DATASETS[nm](n) for nm, n in (("bench19", 40000), ("randwalk", 8 * 3001), ("zeros", 8000), ("linspace", 16392))]
sizes = [h.size for h in hosts]


def call(rows):
    dst = [np.full(n + 16, 0xEE, np.uint8) for n in sizes]
    b = pkg.DeviceBatch([h.ctypes.data for h in hosts], sizes, [d.ctypes.data for d in dst], [d.size for d in dst])
    assert b.compress_params(rows) == 0 and all(c > 0 for c in b.results()), b.results()
    return [d[:c].copy() for d, c in zip(dst, b.results())]


same = [pkg.cparams(8, 5, 1, b"lz4", 8192)] * 4
mixed = [pkg.cparams(8, 5, 1, b"lz4", 8192), pkg.cparams(8, 3, 1, b"zstd", 8192), pkg.cparams(4, 5, 2, b"blosclz", 8192), pkg.cparams(8, 5, 1, b"lz4hc", 8192)]
first = call(same)
assert all(np.array_equal(a, b) for a, b in zip(first, call(same)))
m1 = call(mixed)
m2 = call(mixed)
assert all(np.array_equal(a, b) for a, b in zip(m1[:3], m2[:3]))
assert np.array_equal(m1[0], first[0]), "the lz4 chunk of the mixed call differs from the homogeneous call's"
assert all(np.array_equal(a, b) for a, b in zip(first, call(same))), "the homogeneous batch changed after a heterogeneous call"
assert all(np.array_equal(a, b) for a, b in zip(first, call(same)))
print("cache ok")
