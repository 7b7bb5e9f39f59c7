"""tensors.where_rows_clauses / aggregate_rows_clauses on the device (c-blosc_amd/tensors.py; include/blosc_gpu_clauses.h): a pack_rows
table of float32 and of int16 with 4 columns.  The index table is torch.nonzero of the same boolean expression; count, min, max and argmin
are torch's on the masked column; the floating-point sum is held bit for bit, per chunk, against aggregate_checks.tree_sum over the rows
torch lets through, the integer sum exactly.  The index table is then fed to take_rows."""
import importlib.util
import os

import numpy as np
import pytest

from aggregate_checks import tree_sum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, PER_CHUNK = 5000, 1100


@pytest.fixture(scope="module")
def tensors():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_tensors_clauses", os.path.join(ROOT, "c-blosc_amd", "tensors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert hasattr(mod, "where_rows_clauses"), "tensors.py has no clause calls"
    return mod


def make_table(dtype):
    import torch
    dev = torch.device("cuda:0")
    dt = getattr(torch, dtype)
    g = torch.Generator(device=dev); g.manual_seed(23)
    table = torch.randint(-6, 7, (ROWS, 4), device=dev, generator=g).to(dt)
    if dt.is_floating_point:
        table = table * 0.375 + torch.rand((ROWS, 4), device=dev, generator=g).to(dt) * 1e-3      # sums that round
        table[:, 1] = torch.randint(0, 5, (ROWS,), device=dev, generator=g).to(dt)               # a key column
        table[::37, 0] = float("nan"); table[5::41, 2] = float("inf"); table[3::43, 2] = -0.0
    return table


# name -> (clauses, the same expression on the torch table)
def queries(t, floating):
    c = [t[:, k] for k in range(4)]
    q = {
        "a range": ([(">=", -1, 0), ("<", 2, 0)], (c[0] >= -1) & (c[0] < 2)),
        "two columns": ([("ge", 0, 0), ("eq", 3, 1)], (c[0] >= 0) & (c[1] == 3)),
        "a key set": ([[("==", 1, 1), ("==", 3, 1), ("==", 4, 1)]], (c[1] == 1) | (c[1] == 3) | (c[1] == 4)),
        "a range and a key set": ([(">", -2, 2), ("<=", 1, 2), [("==", 0, 1), ("==", 2, 1)], ("!=", 0, 3)],
                                  (c[2] > -2) & (c[2] <= 1) & ((c[1] == 0) | (c[1] == 2)) & (c[3] != 0)),
    }
    if floating:
        q["no NaN"] = ([[("<", 0.1, 0), (">=", 0.1, 0)]], (c[0] < 0.1) | (c[0] >= 0.1))
    return q


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_clauses_on_a_packed_table(lib, tensors, dtype):
    import torch
    table = make_table(dtype)
    dt = table.dtype
    cont, off, meta = tensors.pack_rows(lib, table, rows_per_chunk=PER_CHUNK, cname=b"lz4", shuffle=1)
    for name, (clauses, mask) in queries(table, dt.is_floating_point).items():
        want = torch.nonzero(mask).flatten()
        assert 0 < want.numel() < ROWS, name
        index, total = tensors.where_rows_clauses(lib, cont, off, meta, clauses)
        assert index.dtype == torch.int64 and index.is_cuda and total == want.numel() and torch.equal(index, want), (dtype, name)
        rows = tensors.take_rows(lib, cont, off, meta, index)
        assert torch.equal(rows.contiguous().view(torch.uint8), table[want].contiguous().view(torch.uint8)), (dtype, name)      # (bytes: NaN rows are among them)
        half, total = tensors.where_rows_clauses(lib, cont, off, meta, clauses, max_matches=want.numel() // 2)
        assert total == want.numel() and torch.equal(half, want[:want.numel() // 2])
        for column in (2, 0):
            got = tensors.aggregate_rows_clauses(lib, cont, off, meta, column=column, clauses=clauses)
            col = table[:, column]
            nan = torch.isnan(col) if dt.is_floating_point else torch.zeros_like(mask)
            live = mask & ~nan
            assert (got.count, got.nans) == (int(mask.sum()), int((mask & nan).sum())), (dtype, name, column)
            vals = col[live]
            assert vals.numel() > 0
            assert got.min == vals.min().item() and got.max == vals.max().item(), (dtype, name, column)
            at = torch.nonzero(live).flatten()
            assert got.argmin == int(at[torch.nonzero(vals == vals.min())[0]]), (dtype, name, column)      # the lowest row that holds it
            assert got.argmax == int(at[torch.nonzero(vals == vals.max())[0]]), (dtype, name, column)
            if dt.is_floating_point:
                x = torch.where(live, col, torch.zeros_like(col)).to(torch.float64).cpu().numpy()
                with np.errstate(invalid="ignore"):
                    sums = [tree_sum(x[a:a + PER_CHUNK]) for a in range(0, ROWS, PER_CHUNK)]
                for k, (chunk, model) in enumerate(zip(got.chunks, sums)):
                    assert chunk.sum == model or (np.isnan(model) and np.isnan(chunk.sum)), (dtype, name, column, "chunk", k, chunk.sum, model)
                total_sum = 0.0
                for s in sums:      # the header's left fold of the chunks
                    total_sum += s
                assert got.sum == total_sum or (np.isnan(total_sum) and np.isnan(got.sum)), (dtype, name, column)
            else:
                assert got.sum == int(vals.to(torch.int64).sum()), (dtype, name, column)
    # no clauses: every row, as aggregate_rows answers
    assert tensors.aggregate_rows_clauses(lib, cont, off, meta, column=1) == tensors.aggregate_rows(lib, cont, off, meta, column=1)
    assert (tensors.aggregate_rows_clauses(lib, cont, off, meta, column=1, clauses=[("ge", 1, 3)])
            == tensors.aggregate_rows(lib, cont, off, meta, column=1, where=("ge", 1, 3)))
    with pytest.raises(ValueError):
        tensors.where_rows_clauses(lib, cont, off, meta, [("eq", 1, 4)])
    if not dt.is_floating_point:
        with pytest.raises(ValueError, match="1.5"):
            tensors.where_rows_clauses(lib, cont, off, meta, [("eq", 1, 0), ("lt", 1.5, 1)])
