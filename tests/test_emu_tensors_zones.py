"""CPU: tensors.zone_map / Zones.refresh / aggregate_rows_fields and the `zones=` keyword of the two clause functions (c-blosc_amd/tensors.py)
on the emulated library, whose "device memory" is the host's: the table of tests/zones_checks.py read as int32 [rows, 4].  put_rows wants
device tensors (tests/test_gpu_tensors_zones.py); here the chunk is written again by the oracle and refreshed."""
import importlib.util
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import orc_compress
from take_checks import BLOCKSIZE, chunk_rows, pack_container
from test_emu_library import emulib  # noqa: F401  (the fixture)
import zones_checks as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class HostMem:
    def alloc(self, n):
        t = torch.empty(max(int(n), 1), dtype=torch.uint8)
        return t.data_ptr(), t


@pytest.fixture(scope="module")
def tensors():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_zones_emu", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod, "zone_map"), "tensors.py has no zone calls"
    return mod


def packed(chunks):
    container, offsets = pack_container(chunks)
    return torch.from_numpy(container.copy()), offsets


def test_zone_map_where_and_refresh(emulib, tensors, oracle):
    rows = [300, 0, 1025, 64]
    first = [int(x) for x in np.concatenate([[0], np.cumsum(rows)])]
    pats = (Z.stamp(np.arange(sum(rows))) % 2 ** 32).astype(np.uint32)
    table = np.zeros((sum(rows), 4), "<i4")
    table[:, 0] = pats.view("<i4")
    table[:, 1] = np.arange(sum(rows)) % 7 - 3
    table[:, 3] = (np.arange(sum(rows)) * 37) % 11
    chunk_of = lambda a: orc_compress(oracle, np.ascontiguousarray(a).view(np.uint8).ravel(), 4, 5, 1, "lz4", blocksize=BLOCKSIZE)[1]
    chunks = [chunk_of(table[first[k]:first[k + 1]]) for k in range(len(rows))]
    assert chunk_rows(chunks, 16) == rows
    cont, off = packed(chunks)
    meta = [(torch.int32, (n, 4)) for n in rows]
    mem = HostMem()
    # several columns in one call
    got = tensors.aggregate_rows_fields(emulib, cont, off, meta, columns=[0, 3, 0], where=("ge", 0, 1))
    for column, one in zip([0, 3, 0], got):
        assert one == tensors.aggregate_rows(emulib, cont, off, meta, column=column, where=("ge", 0, 1)), column
    mask = table[:, 1] >= 0
    assert got[1].count == int(mask.sum()) and got[1].sum == int(table[mask, 3].sum()) and got[0].min == int(table[mask, 0].min())
    # the map, and the two clause functions with it
    zones = tensors.zone_map(emulib, cont, off, meta, [0, 3])
    assert zones.entries.shape == (4, 2) and [int(r) for r in zones.entries["rows"][:, 0]] == rows
    assert [int(x) for x in zones.entries["min_row"][:, 0]] == [0, -1, 300, 1325]
    assert int(zones.entries["min"][2, 0].view("<i4")[0]) == Z.stamp(300)
    clauses = [(">=", Z.stamp(310), 0), ("<", Z.stamp(330), 0), ("!=", 4, 3)]
    want = np.flatnonzero((table[:, 0] >= Z.stamp(310)) & (table[:, 0] < Z.stamp(330)) & (table[:, 3] != 4))
    index, total = tensors.where_rows_clauses(emulib, cont, off, meta, clauses, mem=mem, zones=zones)
    plain, _ = tensors.where_rows_clauses(emulib, cont, off, meta, clauses, mem=mem)
    assert total == want.size > 0 and np.array_equal(index.numpy(), want) and np.array_equal(plain.numpy(), want)
    assert (tensors.aggregate_rows_clauses(emulib, cont, off, meta, column=3, clauses=clauses, zones=zones)
            == tensors.aggregate_rows_clauses(emulib, cont, off, meta, column=3, clauses=clauses))
    # chunk 3 is written again with a value of chunk 2's range: the stale map misses the row, the refreshed one finds it
    changed = table.copy()
    changed[first[3] + 5, 0] = Z.stamp(320)
    chunks2 = list(chunks)
    chunks2[3] = chunk_of(changed[first[3]:first[4]])
    cont2, off2 = packed(chunks2)
    want = np.flatnonzero((changed[:, 0] >= Z.stamp(310)) & (changed[:, 0] < Z.stamp(330)) & (changed[:, 3] != 4))
    assert want[-1] == first[3] + 5
    stale, _ = tensors.where_rows_clauses(emulib, cont2, off2, meta, clauses, mem=mem, zones=zones)
    assert np.array_equal(stale.numpy(), want[:-1]), "a stale map is the caller's: chunk 3 was skipped"
    zones.refresh(emulib, cont2, off2, meta, [3])
    assert zones.entries.tobytes() == tensors.zone_map(emulib, cont2, off2, meta, [0, 3]).entries.tobytes()
    again, _ = tensors.where_rows_clauses(emulib, cont2, off2, meta, clauses, mem=mem, zones=zones)
    assert np.array_equal(again.numpy(), want)
    with pytest.raises(ValueError):
        zones.refresh(emulib, cont2, off2, meta, [4])
    with pytest.raises(ValueError):
        tensors.zone_map(emulib, cont, off, meta, list(range(4)) * 5)
