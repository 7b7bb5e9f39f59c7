"""Trial compression on the device (include/blosc_gpu_select.h): every candidate of every chunk encoded by one launch per encoder
variant, one k_candidate_select, and only the winners written - one call, one synchronisation.  The checks are tests/select_checks.py's,
shared with tests/test_emu_select.py; sizes: packed_checks.MIXED_SIZES with the automatic blocksize."""
import importlib.util
import os

import numpy as np
import pytest

import select_checks as sc
from getitem_ranges_checks import TorchMem
from helpers import DATASETS, header
from packed_checks import MIXED_SIZES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def calls(pkg, lib):
    assert hasattr(lib, "blosc_gpu_compress_packed_select"), "the library has no compress calls with candidates per chunk"
    return sc.Calls(pkg, lib, TorchMem(), 0)


@pytest.fixture(scope="module")
def hosts():
    return sc.select_hosts(MIXED_SIZES)


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


def test_capacity_batch(calls, hosts, settings, yard):
    sc.check_capacity_batch(calls, hosts, settings, yard)


@pytest.mark.parametrize("align", [1, 16])
def test_capacity_packed(calls, hosts, settings, yard, align):
    sc.check_capacity_packed(calls, hosts, settings, yard, align)


def test_nondeterministic_candidates(calls, hosts, oracle, ref):
    sc.check_nondeterministic(calls, hosts, sc.NONDETERMINISTIC, oracle, ref)


def test_launch_counts(calls, pkg, lib, hosts):
    """candidates of two encoder variants: one scan, one selection, one launch per variant, one compaction - for the whole call"""
    two = [sc.Setting(b"lz4", 1, 8, 5), sc.Setting(b"zstd", 1, 8, 3), sc.Setting(b"lz4", 2, 8, 5)]
    first, rows = sc.tables([[calls.row(s) for s in two]] * len(hosts))
    names = ["k_chunk_scan", "k_candidate_select", "k_encode_streams", "k_zstd_encode", "k_chunk_compact", "k_lz4hc_encode", "k_zlib_encode"]
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        res, choice, _, _, _ = calls.select_batch(hosts, first, rows)
        counts = [pkg.profile_get(name)[1] for name in names]
        lib.blosc_gpu_profile_reset()
        need = sum((h.size + 16 + 15) // 16 * 16 for h in hosts)
        _, cb, choice_p, _, _ = calls.select_packed(hosts, first, rows, 16, need)
        counts_p = [pkg.profile_get(name)[1] for name in names]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_gpu_profile_reset()
    assert all(r > 0 for r in res) and cb == res and choice_p == choice and len(set(choice)) > 1
    assert counts == [1, 1, 1, 1, 1, 0, 0] and counts_p == counts, (counts, counts_p)


def test_pack_tensors_with_candidates(pkg, lib):
    """c-blosc_amd/tensors.py: the returned choices are the settings in the headers that were written, and the tensors come back"""
    import torch
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_select", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    tm = importlib.util.module_from_spec(spec); spec.loader.exec_module(tm)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(5)
    walk = torch.cumsum(torch.randn(1 << 18, device=dev, generator=g) * 1e-3, 0)
    tensors = [walk.reshape(512, 512), (walk[:333 * 77].reshape(333, 77) * 100).to(torch.bfloat16),
               torch.randint(0, 4, (129, 257), dtype=torch.int8, device=dev, generator=g),
               torch.randint(0, 1 << 10, (40001,), dtype=torch.int32, device=dev, generator=g),
               torch.from_numpy(sc.text_like(70001)).to(dev), torch.arange(3001, dtype=torch.int64, device=dev) * 7,
               torch.empty((0, 5), dtype=torch.int8, device=dev)]
    cands = [dict(shuffle=0), dict(shuffle=1), dict(shuffle=2), dict(shuffle=1, cname=b"zstd", clevel=3)]
    own = [dict(shuffle=1), dict(shuffle=0)]      # listed for tensor 4 itself: tried as it stands, though its elements are single bytes
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        cont, off, meta, choices = tm.pack_tensors(lib, tensors, cname=b"lz4", clevel=5, align=64, candidates=cands, overrides={4: dict(candidates=own)})
        scans, selects = pkg.profile_get("k_chunk_scan")[1], pkg.profile_get("k_candidate_select")[1]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_gpu_profile_reset()
    assert scans == 1 and selects == 1, "more than one compress call"
    image = cont.cpu().numpy()
    fmt = {b"lz4": 1, b"zstd": 4}
    assert len(choices) == len(tensors) and len({(c["shuffle"], c["cname"]) for c in choices}) >= 3, choices
    for k, (t, c) in enumerate(zip(tensors, choices)):
        h = header(image[off[k]:off[k] + 16])
        assert h["typesize"] == t.element_size() and h["nbytes"] == t.numel() * t.element_size(), (k, h)
        assert h["flags"] >> 5 == fmt[c["cname"]] and (h["flags"] & 1, h["flags"] & 4) == (int(c["shuffle"] == 1), 4 * int(c["shuffle"] == 2)), (k, h, c)
        assert c["clevel"] == (3 if c["cname"] == b"zstd" else 5)
    # single bytes: byte shuffle is not tried next to no filter (it ties and comes later), unless the tensor lists it itself
    assert all(not (c["shuffle"] == 1 and c["cname"] == b"lz4") for c in (choices[2], choices[6])) and choices[4] == dict(cname=b"lz4", clevel=5, shuffle=1)
    assert header(image[off[4]:])["flags"] & 1
    back = tm.unpack_tensors(lib, cont, off, meta)
    for k, (t, u) in enumerate(zip(tensors, back)):
        assert u.dtype == t.dtype and u.shape == t.shape, k
        assert np.array_equal(u.contiguous().view(torch.uint8).cpu().numpy() if u.numel() else np.empty(0, np.uint8),
                              t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.empty(0, np.uint8)), k
