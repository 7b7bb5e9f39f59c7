"""GPU: c-blosc_amd/tensors.py - a dict of tensors of mixed dtypes packed into one container by ONE call with a typesize per chunk
(include/blosc_gpu_params.h) and unpacked bit for bit through blosc_gpu_decompress_packed."""
import importlib.util
import os

import numpy as np
import pytest

from helpers import header

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tensors_mod(pkg):
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def state_dict():
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(11)
    walk = torch.cumsum(torch.randn(1 << 20, device=dev, generator=g) * 1e-3, 0)                 # 4 MiB of float32 that compresses
    return {
        "embed.weight": walk.reshape(1024, 1024),
        "ln.bias": torch.linspace(-1, 1, 1023, device=dev),                                      # float32, odd length
        "proj.weight": (walk[:333 * 77].reshape(333, 77) * 100).to(torch.bfloat16),
        "proj.bias": torch.zeros(77, dtype=torch.bfloat16, device=dev),
        "quant.weight": torch.randint(-8, 8, (129, 257), dtype=torch.int8, device=dev, generator=g),
        "quant.empty": torch.empty((0, 5), dtype=torch.int8, device=dev),
        "steps": torch.arange(3001, dtype=torch.int64, device=dev) * 7,
        "index": torch.randint(0, 50, (13, 3, 5), dtype=torch.int64, device=dev, generator=g).transpose(0, 2),      # not contiguous
    }


def test_pack_and_unpack_a_mixed_state_dict(tensors_mod, pkg, lib, oracle):
    import torch
    sd = state_dict()
    names, tensors = list(sd), list(sd.values())
    assert {t.dtype for t in tensors} == {torch.float32, torch.bfloat16, torch.int8, torch.int64} and len(tensors) == 8
    lib.blosc_gpu_profile(1)
    try:
        lib.blosc_gpu_profile_reset()
        cont, off, meta = tensors_mod.pack_tensors(lib, tensors, cname=b"lz4", clevel=5, shuffle=1, align=64,
                                                   overrides={0: dict(cname=b"zstd", clevel=3), 4: dict(shuffle=2)})
        scans = pkg.profile_get("k_chunk_scan")[1]
    finally:
        lib.blosc_gpu_profile(0)
        lib.blosc_gpu_profile_reset()
    assert scans == 1, "more than one compress call"
    assert len(off) == 9 and off[0] == 0 and all(o % 64 == 0 for o in off) and cont.numel() == off[-1] and cont.dtype == torch.uint8
    assert meta == [(t.dtype, tuple(t.shape)) for t in tensors]
    image = cont.cpu().numpy()
    for k, t in enumerate(tensors):
        h = header(image[off[k]:off[k] + 16])
        assert h["typesize"] == t.element_size() and h["nbytes"] == t.numel() * t.element_size(), (names[k], h)
        assert off[k] + h["cbytes"] <= off[k + 1]
    assert header(image[off[0]:])["flags"] >> 5 == 4 and header(image[off[1]:])["flags"] >> 5 == 1      # zstd for tensor 0, lz4 for the rest
    assert header(image[off[4]:])["flags"] & 4 and header(image[off[2]:])["flags"] & 1                   # bitshuffle for tensor 4, shuffle elsewhere
    sizes = [t.numel() * t.element_size() for t in tensors]
    assert off[-1] <= pkg.PackedBatch(len(sizes)).bound(sizes, 64)
    back = tensors_mod.unpack_tensors(lib, cont, off, meta)
    for name, t, u in zip(names, tensors, back):
        assert u.dtype == t.dtype and u.shape == t.shape and u.device == t.device, name
        assert np.array_equal(u.contiguous().view(torch.uint8).cpu().numpy() if u.numel() else np.empty(0, np.uint8),
                              t.contiguous().view(torch.uint8).cpu().numpy() if t.numel() else np.empty(0, np.uint8)), name


def test_empty_list_and_errors(tensors_mod, lib):
    import torch
    cont, off, meta = tensors_mod.pack_tensors(lib, [])
    assert cont.numel() == 0 and off == [0] and meta == [] and tensors_mod.unpack_tensors(lib, cont, off, meta) == []
    t = torch.ones(1000, device="cuda:0")
    with pytest.raises(RuntimeError):
        tensors_mod.pack_tensors(lib, [t, t], overrides={1: dict(clevel=12)})
    with pytest.raises(ValueError):
        tensors_mod.pack_tensors(lib, [t], align=48)
    cont, off, meta = tensors_mod.pack_tensors(lib, [t])
    with pytest.raises(RuntimeError):
        tensors_mod.unpack_tensors(lib, cont, off, [(torch.float32, (999,))])
