"""The compress calls with parameters per chunk on the device (include/blosc_gpu_params.h): one call, one synchronisation, one launch per
encoder variant the batch holds.  The checks are tests/params_checks.py's, shared with tests/test_emu_params.py; sizes:
packed_checks.MIXED_SIZES with the automatic blocksize."""
import pytest

import params_checks as pc
from getitem_ranges_checks import TorchMem
from packed_checks import SETTINGS, SETTING_IDS, mixed_batch

pytestmark = pytest.mark.gpu
FORCED = 40000      # the one setting with a blocksize of its own: many blocks and a leftover in every chunk above it


@pytest.fixture(scope="module")
def calls(pkg, lib):
    assert hasattr(lib, "blosc_gpu_compress_batch_params"), "the library has no compress calls with parameters per chunk"
    return pc.Calls(pkg, lib, TorchMem(), 0)


@pytest.fixture(scope="module")
def hosts():
    return mixed_batch()


@pytest.fixture(scope="module")
def settings():
    return pc.deterministic_settings(FORCED)


@pytest.fixture(scope="module")
def ref_chunks(calls, hosts, settings):
    return pc.reference_chunks(calls, hosts, settings)


@pytest.mark.parametrize("cname,shuffle,T", SETTINGS, ids=SETTING_IDS)
def test_one_setting_equals_the_old_call(calls, hosts, cname, shuffle, T):
    pc.check_one_setting(calls, hosts, pc.Setting(cname, shuffle, T, 5))


def test_every_deterministic_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref):
    pc.check_every_setting_in_one_batch(calls, hosts, settings, ref_chunks, oracle, ref)


def test_all_encoder_variants_in_one_call(calls, pkg, lib, hosts, settings, ref_chunks, oracle, ref):
    pc.check_all_variants(calls, hosts, settings, ref_chunks, pc.OTHER_SETTINGS, oracle, ref)
    # one launch per variant and call: the twelve settings are five variants under four kernel names (the two Zstd variants share theirs)
    every = settings + pc.OTHER_SETTINGS
    order = pc.interleave(hosts, every)
    batch, rows = [hosts[d] for d, _ in order], [calls.row(every[s]) for _, s in order]
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        res, _, _ = calls.new_batch(batch, rows)
        counts = {name: pkg.profile_get(name)[1] for name in pc.VARIANT_LAUNCHES}
        scans = pkg.profile_get("k_chunk_scan")[1]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_gpu_profile_reset()
    assert all(r > 0 for r in res)
    assert counts == pc.VARIANT_LAUNCHES and scans == 1, (counts, scans)


def test_errors_stay_with_their_chunk(calls, hosts, settings):
    pc.check_errors_stay_with_their_chunk(calls, hosts, settings)


@pytest.mark.parametrize("align", [1, 16])
def test_capacity(calls, hosts, settings, ref_chunks, align):
    pc.check_capacity(calls, hosts, settings, ref_chunks, align)


def test_destsize_and_addresses(calls, hosts, settings, ref_chunks):
    pc.check_destsize_and_addresses(calls, hosts, settings, ref_chunks)
