"""CPU: trial compression (include/blosc_gpu_select.h) on the emulated library - one chunk-table entry per candidate through the host
engine's grouping, k_candidate_select on the wavefront emulator, and layout, headers and compaction over the entries that are left.
The checks are tests/select_checks.py's, shared with tests/test_gpu_select.py; sizes: test_emu_packed.py's, blocksize 8192."""
import importlib.util
import os

import pytest

import select_checks as sc
from getitem_ranges_checks import NumpyMem
from helpers import DATASETS
from test_emu_library import emulib  # noqa: F401  (the fixture)
from test_emu_packed import BLOCKSIZE, EMU_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def calls(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_compress_packed_select"), "the library has no compress calls with candidates per chunk"
    return sc.Calls(pkgmod, emulib, NumpyMem(), BLOCKSIZE)


@pytest.fixture(scope="module")
def hosts():
    return sc.select_hosts(EMU_SIZES)


@pytest.fixture(scope="module")
def settings():
    return sc.candidates()


@pytest.fixture(scope="module")
def yard(calls, hosts, settings):
    return sc.yardstick(calls, hosts, settings)


def test_what_the_inputs_are_chosen_for(calls, hosts, settings, yard):
    sc.check_inputs_of_the_first_check(hosts, settings, yard)


def test_deterministic_candidates(calls, hosts, settings, yard, oracle, ref):
    sc.check_deterministic(calls, hosts, settings, yard, oracle, ref)


def test_one_candidate_per_chunk(calls, hosts, settings):
    sc.check_one_candidate_per_chunk(calls, hosts, settings[:5])


def test_ragged_tables(calls, hosts, settings):
    sc.check_ragged(calls, DATASETS["bench19"](4000), hosts[7], sc.seventy(), settings[1:3])


def test_three_hundred_chunks(calls):
    sc.check_many_chunks(calls, sc.many_hosts(300, 4096), sc.THREE, 16)


def test_errors_stay_where_they_belong(calls, hosts, settings):
    sc.check_errors(calls, [hosts[7], hosts[5], hosts[8]], settings[1:3])


# (the capacity checks call many times: without the two large chunks, which hold four fifths of the bytes)
def test_capacity_batch(calls, hosts, settings, yard):
    sc.check_capacity_batch(calls, hosts[2:], settings, [r[2:] for r in yard])


@pytest.mark.parametrize("align", [1, 16])
def test_capacity_packed(calls, hosts, settings, yard, align):
    sc.check_capacity_packed(calls, hosts[2:], settings, [r[2:] for r in yard], align)


def test_nondeterministic_candidates(calls, hosts, oracle, ref):
    sc.check_nondeterministic(calls, [hosts[0], hosts[5], hosts[7], hosts[8], hosts[4]], sc.NONDETERMINISTIC, oracle, ref)
