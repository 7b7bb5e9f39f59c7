"""CPU: tests/test_gpu_batch_bounds.py's cases 1 and 2 on the emulated library - the same device sources (host engine, k_chunk_scan,
k_chunk_compact, the filters and the decode kernels) run by the wavefront emulator, "device" memory being the host's.  The checkers are
tests/batch_bounds_checks.py's; the chunks are of the 40 KiB class only and the settings a handful: one per filter path (the wave's LDS tile
for typesize 17, fused bitshuffle, fused byte shuffle, the stand-alone unshuffle kernel behind the Zstd decoder, none), the three deterministic
writers and one of the others."""
import pytest

from batch_bounds_checks import (check_capacity, check_odd_compress, check_odd_decompress, check_policy, declare, mixed_hosts, stock_chunks)
from getitem_ranges_checks import SMALL, NumpyMem
from test_emu_library import emulib  # noqa: F401  (the fixture)

# (compressor, clevel, typesize, doshuffle), deterministic writer
CAPACITY = [(("lz4", 5, 17, 1), True), (("blosclz", 5, 4, 2), True)]
RESIDUES = [(("lz4", 5, 17, 1), True), (("blosclz", 5, 4, 2), True), (("lz4", 5, 8, 1), True), (("zstd", 5, 3, 1), True), (("lz4hc", 7, 1, 0), False)]
ids = lambda settings: ["-".join(str(x) for x in s) for s, _ in settings]


@pytest.fixture(scope="module")
def elib(emulib):
    return declare(emulib)


@pytest.mark.parametrize("setting,deterministic", CAPACITY, ids=ids(CAPACITY))
def test_compress_capacity(elib, oracle, ref, setting, deterministic):
    """(the deterministic settings also confirm on the CPU that the chunks of the capacity cases are regular ones, not MEMCPYED)"""
    check_capacity(elib, NumpyMem(), oracle, ref, setting, SMALL, deterministic, rotations=(0,))


@pytest.mark.parametrize("cname,T,shuffle", [("lz4", 17, 1), ("blosclz", 4, 2), ("zstd", 1, 0), ("zlib", 8, 1)])
def test_policy_outcomes_are_the_references(elib, oracle, ref, cname, T, shuffle):
    if ref is None and cname not in ("lz4", "blosclz"):
        cname = "lz4"                   # (the oracle writes LZ4 and BloscLZ only)
    check_policy(elib, NumpyMem(), oracle, ref, cname, T, shuffle)


@pytest.mark.parametrize("setting,deterministic", RESIDUES, ids=ids(RESIDUES))
def test_every_address_residue(elib, oracle, ref, setting, deterministic):
    mem = NumpyMem()
    hosts, own = check_odd_compress(elib, mem, oracle, ref, setting, SMALL, deterministic, light=True)
    stock = stock_chunks(oracle, ref, mixed_hosts(SMALL, 0, light=True), setting)
    check_odd_decompress(elib, mem, hosts, (stock if stock is not None else own[:8]) + own[8:], setting)
