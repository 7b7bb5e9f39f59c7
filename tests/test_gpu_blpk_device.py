"""GPU: whole files from and to DEVICE memory (c-blosc_amd/blpk.py: pack_device / unpack_device) - the data sets and settings of
tests/test_gpu_blpk.py, crosswise with pack / unpack; every chunk inside is an ordinary c-blosc chunk, read here by the oracle and the
reference."""
import importlib.util
import io
import os
import struct

import numpy as np
import pytest

from helpers import DATASETS, orc_decompress, ref_decompress

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("bench19", (5 << 20) + 12345, 1 << 20, 8, 1), ("randwalk", 3 << 20, 1 << 19, 8, 2), ("zeros", 100, 1 << 20, 1, 0),
         ("smallints", (1 << 22) + 4, 700001, 4, 1))


@pytest.fixture(scope="module")
def blpk():
    spec = importlib.util.spec_from_file_location("blpk", os.path.join(ROOT, "c-blosc_amd", "blpk.py"))
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    return m


def read_device(blpk, lib, blob, n):
    import torch
    assert blpk.unpack_device(lib, io.BytesIO(blob)) == n
    out = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    assert blpk.unpack_device(lib, io.BytesIO(blob), out.data_ptr(), n) == n
    back = out.cpu().numpy()
    assert np.all(back[n:] == 0xEE)
    return back[:n]


@pytest.mark.parametrize("cname", [b"lz4", b"blosclz", b"zstd", b"zlib"])
def test_file_roundtrip_and_chunks_are_stock(blpk, lib, oracle, ref, cname):
    import torch
    for dname, n, cs, T, checksum in CASES:
        data = DATASETS[dname](n)
        dev = torch.from_numpy(data).to("cuda:0")
        kw = dict(chunk_size=cs, typesize=T, clevel=5, shuffle=1, cname=cname, checksum=checksum, batch_bytes=2 << 20)
        by_device, by_pack = io.BytesIO(), io.BytesIO()
        nchunks, nbytes = blpk.pack_device(lib, dev.data_ptr(), n, by_device, **kw)
        assert nchunks == (n + cs - 1) // cs and len(by_device.getvalue()) == nbytes
        blpk.pack(lib, data, by_pack, **kw)
        if cname in (b"lz4", b"blosclz"):                # the settings whose bytes the packed call pins to the batch call's
            assert by_device.getvalue() == by_pack.getvalue(), (dname, cname)
        assert np.array_equal(read_device(blpk, lib, by_device.getvalue(), n), data), (dname, cname)
        assert np.array_equal(read_device(blpk, lib, by_pack.getvalue(), n), data), (dname, cname, "pack -> unpack_device")
        assert np.array_equal(blpk.unpack(lib, io.BytesIO(by_device.getvalue()), batch_bytes=2 << 20), data), (dname, cname, "pack_device -> unpack")
        blob = by_device.getvalue()
        offs = np.frombuffer(blob, "<i8", nchunks, 32)
        for k in range(nchunks):
            o = int(offs[k]); nb, _, cb = struct.unpack("<iii", blob[o + 4:o + 16])
            chunk = np.frombuffer(blob, np.uint8, cb, o).copy()
            want = data[k * cs:min(n, (k + 1) * cs)]
            r, out = orc_decompress(oracle, chunk, nb)
            assert r == want.size and np.array_equal(out, want), (dname, cname, k)
            if ref is not None:
                r2, out2 = ref_decompress(ref, chunk, nb)
                assert r2 == want.size and np.array_equal(out2, want)


@pytest.mark.parametrize("checksum", [1, 2])
def test_corrupt_file_is_refused(blpk, lib, checksum):
    import torch
    data = DATASETS["bench19"](3 << 20)
    dev = torch.from_numpy(data).to("cuda:0")
    buf = io.BytesIO()
    blpk.pack_device(lib, dev.data_ptr(), data.size, buf, chunk_size=1 << 20, typesize=8, cname=b"lz4", checksum=checksum)
    blob = bytearray(buf.getvalue())
    blob[-100] ^= 0x40                                   # inside the last chunk: its digest no longer fits
    out = torch.zeros(data.size, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(blpk.BlpkError, match="chunk 2: checksum"):
        blpk.unpack_device(lib, io.BytesIO(bytes(blob)), out.data_ptr(), data.size)
    with pytest.raises(blpk.BlpkError):
        blpk.unpack(lib, io.BytesIO(bytes(blob)))
