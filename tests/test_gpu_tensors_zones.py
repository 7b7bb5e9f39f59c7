"""tensors.zone_map / Zones / aggregate_rows_fields and the `zones=` keyword on the device (c-blosc_amd/tensors.py; include/blosc_gpu_zones.h):
a pack_rows table whose column 0 ascends.  With a map the answers are those without one; the map's entries are torch's minimum and maximum
of every chunk; after put_rows moved a value out of a chunk's old range the stale map misses the row and the refreshed one finds it."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, PER_CHUNK = 5000, 1100


@pytest.fixture(scope="module")
def tensors():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_zones", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod, "zone_map"), "tensors.py has no zone calls"
    return mod


def make_table(dtype):
    import torch
    dev = torch.device("cuda:0")
    dt = getattr(torch, dtype)
    g = torch.Generator(device=dev); g.manual_seed(29)
    table = torch.randint(-6, 7, (ROWS, 4), device=dev, generator=g).to(dt)
    table[:, 0] = (torch.arange(ROWS, device=dev) // 2 - 1000).to(dt)      # ascending, every value twice
    if dt.is_floating_point:
        table[:, 2] = table[:, 2] * 0.375 + torch.rand((ROWS,), device=dev, generator=g).to(dt) * 1e-3
        table[::37, 2] = float("nan")
    return table


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_zones_on_a_packed_table(lib, tensors, dtype):
    import torch
    table = make_table(dtype)
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=PER_CHUNK, cname=b"lz4", shuffle=1)
    nchunks = len(meta)
    # ---- several columns in one call: what aggregate_rows answers for each ----
    for where in (None, ("ge", 1, 3), [("ge", 1, 3), [("lt", -900, 0), ("gt", 0, 1)]]):
        got = tensors.aggregate_rows_fields(lib, cont, off, meta, columns=[2, 0, 2, 3], where=where)
        clauses = [where] if isinstance(where, tuple) else where
        for column, one in zip([2, 0, 2, 3], got):
            assert one == tensors.aggregate_rows_clauses(lib, cont, off, meta, column=column, clauses=clauses), (dtype, where, column)
        if where is None or isinstance(where, tuple):
            assert got[1] == tensors.aggregate_rows(lib, cont, off, meta, column=0, where=where)
    with pytest.raises(ValueError):
        tensors.aggregate_rows_fields(lib, cont, off, meta, columns=[])
    with pytest.raises(ValueError):
        tensors.aggregate_rows_fields(lib, cont, off, meta, columns=[0] * 17)
    with pytest.raises(ValueError):
        tensors.aggregate_rows_fields(lib, cont, off, meta, columns=[4])
    # ---- the map: torch's extremes of every chunk ----
    zones = tensors.zone_map(lib, cont, off, meta, [0, 2])
    assert zones.entries.shape == (nchunks, 2) and zones.columns == [0, 2]
    for k in range(nchunks):
        part = table[k * PER_CHUNK:(k + 1) * PER_CHUNK]
        for f, column in enumerate((0, 2)):
            col = part[:, column]
            live = col[~torch.isnan(col)] if col.dtype.is_floating_point else col
            e = zones.entries[k, f]
            raw = lambda x: bytes(torch.tensor([x], dtype=table.dtype).view(torch.uint8).tolist())
            assert int(e["rows"]) == int(e["count"]) == part.shape[0] and int(e["nans"]) == part.shape[0] - live.numel()
            assert bytes(e["min"])[:len(raw(0))] == raw(live.min().item()) and bytes(e["max"])[:len(raw(0))] == raw(live.max().item())
            assert int(e["min_row"]) == k * PER_CHUNK + int(torch.nonzero(col == live.min())[0])
    # ---- with the map: the same answers; a range of column 0 lives in one chunk ----
    c = [table[:, k] for k in range(4)]
    queries = {"a range in chunk 2": ([(">=", 200, 0), ("<", 260, 0)], (c[0] >= 200) & (c[0] < 260)),
               "a range and a key": ([(">=", -450, 0), ("<=", -440, 0), [("==", 1, 1), ("==", 3, 1)]], (c[0] >= -450) & (c[0] <= -440) & ((c[1] == 1) | (c[1] == 3))),
               "nothing": ([(">", 5000, 0)], c[0] > 5000),
               "everything but the NaNs" if table.dtype.is_floating_point else "every row": ([[("<", 0, 2), (">=", 0, 2)]], (c[2] < 0) | (c[2] >= 0))}
    for name, (clauses, mask) in queries.items():
        want = torch.nonzero(mask).flatten()
        index, total = tensors.where_rows_clauses(lib, cont, off, meta, clauses, zones=zones)
        plain_index, plain_total = tensors.where_rows_clauses(lib, cont, off, meta, clauses)
        assert total == plain_total == want.numel() and torch.equal(index, want) and torch.equal(plain_index, want), (dtype, name)
        for column in (2, 1):
            assert (tensors.aggregate_rows_clauses(lib, cont, off, meta, column=column, clauses=clauses, zones=zones)
                    == tensors.aggregate_rows_clauses(lib, cont, off, meta, column=column, clauses=clauses)), (dtype, name, column)
    # the range was served from one chunk's decode
    pkg = tensors._sibling("", "__init__.py")
    zoned = pkg.RowWhereZoned(4 * table.element_size(), lib=lib)
    terms, *_ = tensors._clause_terms(pkg, meta, "the test", queries["a range in chunk 2"][0])
    assert zoned.packed(cont.data_ptr(), int(cont.numel()), list(off), terms, zones.fields, zones.table(pkg), None, 0) == 0
    assert zoned.pruned() == [1, 1, 0, 1, 1] and zoned.total() == int(queries["a range in chunk 2"][1].sum())
    with pytest.raises(ValueError):
        tensors.where_rows_clauses(lib, cont, off, meta[:-1], [("==", 1, 0)], zones=zones)
    # ---- put_rows moves a value out of chunk 0's old range: the stale map misses it, the refreshed one finds it ----
    row = 17
    new = table[row:row + 1].clone()
    new[0, 0] = 225      # a value of chunk 2's range, now in chunk 0
    index = torch.tensor([row], dtype=torch.int64, device=table.device)
    cont2, off2, rewritten = tensors.put_rows(lib, cont, off, meta, index, new, return_rewritten=True)
    assert rewritten == [0]
    assert len(tensors.put_rows(lib, cont, off, meta, index, new)) == 2      # as before without the keyword
    changed = table.clone(); changed[row] = new[0]
    clauses = [(">=", 220, 0), ("<", 230, 0)]
    want = torch.nonzero((changed[:, 0] >= 220) & (changed[:, 0] < 230)).flatten()
    assert want[0] == row and want.numel() > 1
    unzoned, _ = tensors.where_rows_clauses(lib, cont2, off2, meta, clauses)
    assert torch.equal(unzoned, want)
    stale, _ = tensors.where_rows_clauses(lib, cont2, off2, meta, clauses, zones=zones)
    assert torch.equal(stale, want[1:]), "a stale map is the caller's: chunk 0 was skipped"
    before = zones.entries.copy()
    assert zones.refresh(lib, cont2, off2, meta, rewritten) is zones
    assert (zones.entries[1:] == before[1:]).all() and int(zones.entries[0, 0]["max_row"]) == row
    fresh = tensors.zone_map(lib, cont2, off2, meta, [0, 2])
    assert zones.entries.tobytes() == fresh.entries.tobytes(), "refresh of the rewritten chunks gives the map of the new container"
    again, total = tensors.where_rows_clauses(lib, cont2, off2, meta, clauses, zones=zones)
    assert torch.equal(again, want) and total == want.numel()
    assert (tensors.aggregate_rows_clauses(lib, cont2, off2, meta, column=0, clauses=clauses, zones=zones)
            == tensors.aggregate_rows_clauses(lib, cont2, off2, meta, column=0, clauses=clauses))
    # refresh of a chunk in the middle keeps the table's row numbers
    assert zones.refresh(lib, cont2, off2, meta, [3, 1]).entries.tobytes() == fresh.entries.tobytes()
