"""include/blosc_gpu_checksum.h on the device: zlib's adler32 / crc32 of many runs in one call.  The yardstick is Python's zlib for both
digests; the cases are tests/checksum_checks.py's (the emulator's grid with the product's tile of 256 KiB), plus what only a device
holds: runs of 64 MiB, and runs on both sides of the 4 GiB offset of one buffer."""
import numpy as np
import pytest

from checksum_checks import KIND_IDS, KINDS, LONG_COUNTS, ZLIB, alignment_case, check_runs, grid_case, lay_out, long_search_case, many_runs_case
from helpers import DATASETS

pytestmark = pytest.mark.gpu
TILE = 256 << 10


def to_dev(buf):
    import torch
    t = torch.from_numpy(buf).to("cuda:0")
    assert t.data_ptr() % 16 == 0
    return t


@pytest.fixture(scope="module")
def grid():
    buf, runs = grid_case(TILE)
    return buf, runs, to_dev(buf)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_lengths_and_contents(pkg, lib, grid, kind):
    buf, runs, dev = grid
    check_runs(pkg, lib, kind, dev.data_ptr(), buf, runs, "grid")


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_alignment_and_many_runs(pkg, lib, kind):
    for what, (buf, runs) in (("alignment", alignment_case()), ("300 runs", many_runs_case()), ("20000 runs", many_runs_case(15, 20000, 40))):
        dev = to_dev(buf)
        check_runs(pkg, lib, kind, dev.data_ptr(), buf, runs, what)


@pytest.mark.parametrize("nruns", LONG_COUNTS)
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_more_runs_than_two_rounds_of_the_search(pkg, lib, kind, nruns):
    """4096 runs are found in two rounds of the 64-way search of a tile's run, 4097 and 5000 take a third; stretches of 70 and 4100 empty runs"""
    buf, runs = long_search_case(nruns)
    assert len(runs) == nruns
    dev = to_dev(buf)
    check_runs(pkg, lib, kind, dev.data_ptr(), buf, runs, f"{nruns} runs")


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(16)
    n = (64 << 20) + 5
    buf, runs = lay_out([rng.integers(0, 256, n, dtype=np.uint8), np.full(n, 0xFF, np.uint8)], shifts=[7, 0])
    return buf, runs, to_dev(buf)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_runs_of_64_mib(pkg, lib, big, kind):
    buf, runs, dev = big
    check_runs(pkg, lib, kind, dev.data_ptr(), buf, runs, "64 MiB + 5")


def test_runs_on_both_sides_of_4_gib(pkg, lib):
    import torch
    size = (4 << 30) + (1 << 20)
    dev = torch.empty(size, dtype=torch.uint8, device="cuda:0")       # never filled apart from the runs
    rng = np.random.default_rng(17)
    offs = [12345, (4 << 30) - 70001, (4 << 30) + 3, size - 50000]
    hosts = [rng.integers(0, 256, n, dtype=np.uint8) for n in (30000, 70000, 65521, 50000)]
    assert offs[1] + hosts[1].size < 4 << 30
    for o, h in zip(offs, hosts):
        dev[o:o + h.size] = torch.from_numpy(h).to("cuda:0")
    for kind in KINDS:
        got = pkg.checksums_packed(kind, dev.data_ptr(), size, offs + [size], [h.size for h in hosts], lib=lib)
        assert got == [ZLIB[kind](h.tobytes()) for h in hosts], KIND_IDS[kind - 1]


def test_container_of_compress_packed(pkg, lib):
    import torch
    n = 1 << 20
    hosts = [DATASETS["bench19" if k % 3 else "random"](n) for k in range(16)]
    src = [torch.from_numpy(h).to("cuda:0") for h in hosts]
    b = pkg.PackedBatch(16)
    room = b.bound([n] * 16, 1)
    cont = torch.empty(room, dtype=torch.uint8, device="cuda:0")
    assert b.compress([t.data_ptr() for t in src], [n] * 16, cont.data_ptr(), room, 8, 5, 1, b"lz4", 0, 1) == 0
    off, cb = b.offsets(), b.results()
    assert all(c > 0 for c in cb)
    host = cont.cpu().numpy()
    for kind in KINDS:
        got = pkg.checksums_packed(kind, cont.data_ptr(), room, off, cb, lib=lib)
        assert got == [ZLIB[kind](host[off[i]:off[i] + cb[i]].tobytes()) for i in range(16)], KIND_IDS[kind - 1]
        assert pkg.checksums_packed(kind, cont.data_ptr(), room, off, None, lib=lib) == got      # align 1: the spans are the chunks
