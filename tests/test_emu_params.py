"""CPU: the compress calls with parameters per chunk (include/blosc_gpu_params.h) on the emulated library - the host engine's grouping of
a batch by encoder variant, one launch per group with queues, tickets and scratch of its own, and everything around the launches once
for the batch.  The checks are tests/params_checks.py's, shared with tests/test_gpu_params.py; sizes: test_emu_packed.py's."""
import importlib.util
import os
import subprocess
import sys

import pytest

import params_checks as pc
from getitem_ranges_checks import NumpyMem
from packed_checks import SETTINGS, SETTING_IDS, mixed_batch
from test_emu_library import emulib  # noqa: F401  (the fixture)
from test_emu_packed import BLOCKSIZE, EMU_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORCED = 2 * BLOCKSIZE      # the one setting with a blocksize of its own


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def calls(emulib, pkgmod):
    assert hasattr(emulib, "blosc_gpu_compress_batch_params"), "the library has no compress calls with parameters per chunk"
    return pc.Calls(pkgmod, emulib, NumpyMem(), BLOCKSIZE)


@pytest.fixture(scope="module")
def hosts():
    return mixed_batch(EMU_SIZES)


@pytest.fixture(scope="module")
def settings():
    return pc.deterministic_settings(FORCED)


@pytest.fixture(scope="module")
def ref_chunks(calls, hosts, settings):
    return pc.reference_chunks(calls, hosts, settings)


@pytest.mark.parametrize("cname,shuffle,T", SETTINGS, ids=SETTING_IDS)
def test_one_setting_equals_the_old_call(calls, hosts, cname, shuffle, T):
    pc.check_one_setting(calls, hosts, pc.Setting(cname, shuffle, T, 5))


def test_shapes_of_the_batch(hosts, settings, ref_chunks):
    """what the sizes are chosen for: full blocks and a leftover block, a split block and an unsplit one, MEMCPYED by the host and by the scan"""
    lz4 = ref_chunks[0]
    flags = [int(c[2]) for c in lz4]
    assert flags[4] & 2 and flags[6] & 2 and not flags[2] & 2, flags
    bs = int(lz4[1][8:12].view("<i4")[0])
    assert bs < hosts[1].size and hosts[1].size % bs
    assert not lz4[0][2] & 0x10 and ref_chunks[7][0][2] & 0x10 and ref_chunks[2][0][2] & 0x10      # split; never split; zstd is not split
    assert int(ref_chunks[8][1][8:12].view("<i4")[0]) == FORCED and int(ref_chunks[2][1][8:12].view("<i4")[0]) == BLOCKSIZE      # a blocksize of its own


def test_every_deterministic_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref):
    pc.check_every_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref)


def test_all_encoder_variants_in_one_call(calls, hosts, settings, ref_chunks, oracle, ref):
    pc.check_all_variants(calls, hosts, settings, ref_chunks, pc.OTHER_SETTINGS, oracle, ref)


def test_errors_stay_with_their_chunk(calls, hosts, settings):
    pc.check_errors_stay_with_their_chunk(calls, hosts, settings)


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(calls, hosts, settings, ref_chunks, align):
    pc.check_capacity(calls, hosts, settings, ref_chunks, align)


def test_destsize_and_addresses(calls, hosts, settings, ref_chunks):
    pc.check_destsize_and_addresses(calls, hosts, settings, ref_chunks)


def test_table_cache_and_feedback(emulib):
    """A child process with the table cache's messages switched on (the switch is read once per process): a homogeneous batch twice - the
    second call finds its tables on the device -, a heterogeneous call, then the homogeneous batch again with the bytes of before."""
    env = dict(os.environ, BLOSC_AMD_DEBUG_COST="1", BLOSC_AMD_LIB=emulib._name)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "params_cache_check.py")], env=env, timeout=600,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and "cache ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
    said = [("still on the device" in ln) for ln in p.stderr.splitlines() if ln.startswith("[blosc_amd] compress: block table and queues")]
    # homogeneous: built, hit | heterogeneous: built, and hit when it is repeated | homogeneous again: built (one set of tables is kept), hit
    assert said == [False, True, False, True, False, True], p.stderr[-3000:]
