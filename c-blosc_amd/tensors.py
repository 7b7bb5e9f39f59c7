"""tensors.py — a list of device tensors of mixed dtypes in ONE packed container, written by ONE call (include/blosc_gpu_params.h; with
candidate settings to choose from: include/blosc_gpu_select.h).

A state dict, a table's columns, a cache line of activations: float32, bfloat16, int8 and int64 side by side.  Every tensor becomes one
c-blosc chunk whose typesize is the tensor's element size, with the codec, filter and clevel of the call or of its own; the chunks lie
back to back in one device buffer with an offset table (include/blosc_gpu_packed.h), in the caller's order.  `unpack_tensors` is the
reverse through blosc_gpu_decompress_packed, which reads chunks of any format, typesize and filter in one call anyway.
`pack_rows` / `take_rows` keep ONE tensor as a table of rows in such a container - cut along dim 0 into chunks of whole rows - and read rows
back by a device index tensor: index_select on the compressed table, one blosc_gpu_take_packed (include/blosc_gpu_take.h).
`put_rows` writes rows by a device index tensor - index_copy_ on the compressed table - into a new container, one blosc_gpu_put_packed
(include/blosc_gpu_put.h): only the chunks a row lands in are decoded and compressed again.
`where_rows` makes the index tensor both read - the rows whose column satisfies a comparison with a scalar, torch.nonzero on the compressed
table - by blosc_gpu_where_packed (include/blosc_gpu_where.h), holding one pass of plaintext at a time.
`aggregate_rows` reduces a column over such rows - count, sum, min, max and the rows of the extremes, per chunk and for the table - by
blosc_gpu_aggregate_packed (include/blosc_gpu_aggregate.h), without an index table.
`where_rows_clauses` / `aggregate_rows_clauses` are the two for SEVERAL comparisons - an AND of OR clauses over any columns: a range, two
columns, a small key set - in one call and one decode (include/blosc_gpu_clauses.h).
`aggregate_rows_fields` reduces several columns in one decode, `zone_map` keeps the per-chunk minimum and maximum of up to 16 columns as a
`Zones`, and the two clause functions take it as `zones=` and do not decode the chunks it excludes (include/blosc_gpu_zones.h).

Like blpk.py's device functions this module only drives the library: `lib` is the ctypes handle (load() of the package), memory comes
from a `mem` with blpk.TorchMem's alloc().  There is no CPU implementation: without the library and a GPU the calls fail.
"""
import collections
import ctypes as C
import importlib.util
import os
import sys

MAX_CHUNK = 2 ** 31 - 1 - 16      # BLOSC_MAX_BUFFERSIZE: one tensor is one chunk


def _sibling(name, file):
    """the package's loader / blpk.py, whether this file was imported as part of the package or loaded by its path"""
    if __package__:
        return importlib.import_module("." + name if name else __package__, __package__) if name else sys.modules[__package__]
    key = "_c_blosc_amd_" + (name or "pkg")
    if key not in sys.modules:
        spec = importlib.util.spec_from_file_location(key, os.path.join(os.path.dirname(os.path.abspath(__file__)), file))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[key] = mod
        spec.loader.exec_module(mod)
    return sys.modules[key]


def _distinct(settings, element_size):
    """`settings` without those that cannot give another size for a tensor of this element size than one in front of them: a byte
    shuffle of single bytes is no filter (it writes another flag byte, never a smaller chunk)"""
    seen, out = set(), []
    for kw in settings:
        key = tuple(sorted(dict(kw, shuffle=0 if (element_size == 1 and kw.get("shuffle") == 1) else kw.get("shuffle")).items()))
        if key not in seen:
            seen.add(key)
            out.append(kw)
    return out


def pack_tensors(lib, tensors, cname=b"lz4", clevel=5, shuffle=1, align=256, overrides=None, mem=None, stream=None, candidates=None):
    """Compress the device tensors `tensors` into one container with one call of blosc_gpu_compress_packed_params.
    Tensor i is chunk i: typesize = its element_size(); codec, clevel and filter are the call's unless overrides[i] (overrides: a dict
    index -> dict with any of cname / clevel / shuffle / blocksize / splitmode) says otherwise.
    Returns (container, offsets, meta): a uint8 device tensor of offsets[-1] bytes, the offset table [n + 1] (multiples of `align`), and
    [(dtype, shape)] for unpack_tensors.
    candidates: a list of such dicts, each tried on top of every tensor's setting by one call of blosc_gpu_compress_packed_select - the
    smallest chunk is the one written, the first of the list on a tie.  Candidates that cannot differ for a tensor are tried once
    (_distinct); overrides[i] may carry a list "candidates" of its own, which is tried as it stands.  Then the result is
    (container, offsets, meta, choices), choices[i] the setting tensor i was written with (a dict of cname / clevel / shuffle / ...)."""
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_packed(lib)
    pkg.declare_params(lib)
    n = len(tensors)
    if n == 0:
        return mem.alloc(0)[1][:0], [0], []
    flat = [t.contiguous() for t in tensors]      # (kept alive until the call has returned)
    sizes = [t.numel() * t.element_size() for t in flat]
    if max(sizes) > MAX_CHUNK:
        raise ValueError("a tensor above 2 GiB - 17 bytes does not fit one chunk: split it")
    tried = []      # per tensor: the settings to try
    for k, t in enumerate(flat):
        kw = dict(cname=cname, clevel=clevel, shuffle=shuffle)
        own = dict((overrides or {}).get(k, {}))
        listed = own.pop("candidates", None)
        kw.update(own)
        if listed is not None: tried.append([dict(kw, **c) for c in listed])
        elif candidates is not None: tried.append(_distinct([dict(kw, **c) for c in candidates], t.element_size()))
        else: tried.append([kw])
    select = candidates is not None or any("candidates" in o for o in (overrides or {}).values())
    rows = [pkg.cparams(t.element_size(), **kw) for t, kws in zip(flat, tried) for kw in kws]
    b = pkg.PackedBatch(n, lib=lib)
    cap = b.bound(sizes, align)
    if cap == 0 and any(sizes):
        raise ValueError("align must be a power of two up to 4096")
    dest, keep = mem.alloc(cap)
    ptrs = [t.data_ptr() if s else 0 for t, s in zip(flat, sizes)]
    if select:
        pkg.declare_select(lib)
        first = [0]
        for kws in tried: first.append(first[-1] + len(kws))
        if b.compress_select(ptrs, sizes, first, rows, dest, cap, align, stream) != 0:
            raise RuntimeError("blosc_gpu_compress_packed_select failed")
    elif b.compress_params(ptrs, sizes, rows, dest, cap, align, stream) != 0:
        raise RuntimeError("blosc_gpu_compress_packed_params failed")
    bad = [(k, r) for k, r in enumerate(b.results()) if r <= 0]
    if bad:
        raise RuntimeError(f"tensors that did not compress (index, code): {bad}")
    off = b.offsets()
    meta = [(t.dtype, tuple(t.shape)) for t in tensors]
    if select:
        return keep[:off[-1]], off, meta, [kws[c] for kws, c in zip(tried, b.choices())]
    return keep[:off[-1]], off, meta


def unpack_tensors(lib, container, offsets, meta, mem=None, stream=None):
    """The tensors of a container of pack_tensors, bit for bit, through one blosc_gpu_decompress_packed."""
    import torch
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_packed(lib)
    n = len(meta)
    if n == 0:
        return []
    want = [int(torch.empty(0, dtype=dt).element_size()) * int(torch.Size(shape).numel()) for dt, shape in meta]
    total = sum(want)
    dest, keep = mem.alloc(total)
    b = pkg.PackedBatch(n, lib=lib)
    if b.decompress(container.data_ptr(), int(container.numel()), list(offsets), dest, total, stream) != 0:
        raise RuntimeError("blosc_gpu_decompress_packed failed")
    if b.results() != want:
        raise RuntimeError(f"the container does not hold these tensors: decoded sizes {b.results()}, expected {want}")
    at = b.offsets()
    # a slice of the byte buffer begins wherever the tensors in front of it end: each tensor gets storage of its own, aligned for its dtype
    return [keep[at[k]:at[k + 1]].clone().view(dt).reshape(shape) for k, (dt, shape) in enumerate(meta)]


def pack_rows(lib, tensor, rows_per_chunk=None, **settings):
    """A device tensor as a table of rows along dim 0, cut into chunks of whole rows and packed by pack_tensors(lib, slices, **settings):
    (container, offsets, meta), meta[i] the dtype and shape of slice i.  rows_per_chunk: default the largest count that keeps a chunk
    under MAX_CHUNK - so a table above 2 GiB, which is no tensor for pack_tensors, has a home.  take_rows reads rows back by index,
    unpack_tensors the slices."""
    if tensor.dim() < 1:
        raise ValueError("a table has a dim 0 to cut along")
    t = tensor.contiguous()
    row_bytes = t.element_size() * int(t[0].numel()) if t.shape[0] else 0
    if t.shape[0] and (row_bytes < 1 or row_bytes > MAX_CHUNK):
        raise ValueError(f"rows of {row_bytes} bytes do not fit a chunk")
    if rows_per_chunk is None:
        rows_per_chunk = max(MAX_CHUNK // max(row_bytes, 1), 1)
    if rows_per_chunk < 1:
        raise ValueError("rows_per_chunk must be positive")
    slices = [t[a:a + rows_per_chunk] for a in range(0, t.shape[0], rows_per_chunk)] or [t]
    return pack_tensors(lib, slices, **settings)


def take_rows(lib, container, offsets, meta, index, mem=None, stream=None):
    """tensor.index_select(0, index) for the table pack_rows packed, by ONE blosc_gpu_take_packed: `index` is an int64 tensor on the device,
    the result has the shape [len(index), *row shape] and the table's dtype.  Raises if any row failed (an index outside the table, a
    block that does not decode), naming how many."""
    import torch
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_take(lib)
    dtype, row_shape = meta[0][0], tuple(meta[0][1][1:])
    if any(dt != dtype or tuple(shape[1:]) != row_shape for dt, shape in meta):
        raise ValueError("the container's chunks are not slices of one table")
    row_bytes = int(torch.empty(0, dtype=dtype).element_size()) * int(torch.Size(row_shape).numel())
    if not 1 <= row_bytes <= 65536:
        raise ValueError(f"rows of {row_bytes} bytes: blosc_gpu_take_packed takes 1 ... 65536")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda:
        raise ValueError("index: a one-dimensional int64 tensor on the device")
    idx = index.contiguous()
    n = int(idx.numel())
    dest, keep = mem.alloc(n * row_bytes)
    take = pkg.RowTake(row_bytes, lib=lib)
    if take.packed(container.data_ptr(), int(container.numel()), list(offsets), idx.data_ptr(), n, dest, None, stream) != 0:
        raise RuntimeError(f"blosc_gpu_take_packed failed; rows per chunk (negative: the chunk's code): {take.chunk_rows()}")
    if take.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {take.chunk_rows()}")
    if take.failed():
        raise RuntimeError(f"{take.failed()} of {n} rows failed (an index outside 0 ... {sum(take.chunk_rows()) - 1}, or a block that does not decode)")
    return keep[:n * row_bytes].view(dtype).reshape((n,) + row_shape)


_WHERE_OPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5, "==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}


def _table_fields(pkg, meta, call, *columns):
    """What where_rows and aggregate_rows read from `meta`: (the table's dtype, its field kind, its element size, the bytes of a row);
    ValueError for chunks that are not slices of one table, a dtype without a field kind, rows `call` does not take, a column outside the row"""
    import torch
    dtype, row_shape = meta[0][0], tuple(meta[0][1][1:])
    if any(dt != dtype or tuple(shape[1:]) != row_shape for dt, shape in meta):
        raise ValueError("the container's chunks are not slices of one table")
    kinds = {torch.uint8: pkg.FIELD_UINT, torch.bool: pkg.FIELD_UINT, torch.int8: pkg.FIELD_INT, torch.int16: pkg.FIELD_INT, torch.int32: pkg.FIELD_INT,
             torch.int64: pkg.FIELD_INT, torch.float16: pkg.FIELD_FLOAT, torch.float32: pkg.FIELD_FLOAT, torch.float64: pkg.FIELD_FLOAT,
             torch.bfloat16: pkg.FIELD_BFLOAT16}
    if dtype not in kinds:
        raise ValueError(f"no predicate for a table of {dtype}")
    element = int(torch.empty(0, dtype=dtype).element_size())
    per_row = int(torch.Size(row_shape).numel())
    row_bytes = element * per_row
    if not 1 <= row_bytes <= 65536:
        raise ValueError(f"rows of {row_bytes} bytes: {call} takes 1 ... 65536")
    for column in columns:
        if not 0 <= column < per_row:
            raise ValueError(f"column {column} of rows of {per_row} elements")
    return dtype, kinds[dtype], element, row_bytes


def _where_predicate(pkg, dtype, kind, element, op, value, column):
    """column `op` value as a Predicate; ValueError for an op nobody knows, and for a value that an integer (or bool) dtype does not hold"""
    import torch
    name = getattr(op, "__name__", op)
    if name not in _WHERE_OPS:
        raise ValueError(f"op {op!r}: one of {sorted(_WHERE_OPS)}")
    if not dtype.is_floating_point:
        # an integer column is compared with the value itself: 1.5, a NaN or 300 on uint8 is no constant of the dtype, and rounding or
        # wrapping it would answer another question than torch's op(column, value)
        low, high = (0, 1) if dtype == torch.bool else (torch.iinfo(dtype).min, torch.iinfo(dtype).max)
        try:
            whole = int(value)
        except (TypeError, ValueError, OverflowError):      # a NaN, an infinity, no number at all
            whole = None
        if whole is None or whole != value or not low <= whole <= high:
            raise ValueError(f"the value {value!r} is none that {dtype} holds: a table of integers is compared with an integer of {low} ... {high}")
        value = whole
    # the constant in the table's own representation: torch rounds a floating-point one as it would round the scalar of the comparison
    raw = bytes(torch.tensor([value], dtype=dtype).view(torch.uint8).tolist())
    return pkg.predicate(kind, element, _WHERE_OPS[name], raw, offset=column * element)


def where_rows(lib, container, offsets, meta, op, value, column=0, max_matches=None, mem=None, stream=None):
    """torch.nonzero(op(table.reshape(nrows, -1)[:, column], value)).flatten() for the table pack_rows packed, without its plaintext:
    blosc_gpu_where_packed (include/blosc_gpu_where.h) decodes pass by pass and keeps the row numbers alone.  op: "eq" / "ne" / "lt" / "le" /
    "gt" / "ge" (or "==", "!=", ...; the functions of `operator` and the torch comparisons are taken by their name), value: a scalar of the
    table's dtype, column: the flat element number inside a row.  The predicate's type is the table's dtype: torch.uint8 and bool are
    unsigned bytes, int8 ... int64, float16 / float32 / float64, bfloat16; any other raises ValueError.
    The value of a floating-point table is rounded to the dtype, as torch rounds the scalar of its own comparison (0.1 on float16 is the
    float16 next to 0.1, 1e6 on float16 is inf).  The value of an integer or bool table must be one the dtype holds - an int, a bool or an
    integral float such as 2.0 inside its range: 1.5, a NaN, an infinity, 300 on uint8 or 2**63 on int64 raise ValueError and are never
    rounded or wrapped into another constant.
    Returns (index, total): an int64 device tensor - what take_rows and put_rows read - and the number of matches.  With max_matches the
    table has min(total, max_matches) entries, the first ones, and one call is made.  With max_matches=None TWO calls are made: one with
    capacity 0 that counts, one that fills a table of exactly `total` (none if nothing matches).
    Raises, like take_rows, if the container does not hold this table or if any row was unread (a chunk that does not decode)."""
    import torch
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_where(lib)
    dtype, kind, element, row_bytes = _table_fields(pkg, meta, "blosc_gpu_where_packed", column)
    pred = _where_predicate(pkg, dtype, kind, element, op, value, column)
    where = pkg.RowWhere(row_bytes, lib=lib)

    def call(ptr, capacity):
        if where.packed(container.data_ptr(), int(container.numel()), list(offsets), pred, ptr, capacity, stream) != 0:
            raise RuntimeError(f"blosc_gpu_where_packed failed; rows per chunk (negative: the chunk's code): {where.chunk_rows()}")
        if where.chunk_rows() != [int(shape[0]) for _, shape in meta]:
            raise RuntimeError(f"the container does not hold this table: rows per chunk {where.chunk_rows()}")
        if where.unread():
            raise RuntimeError(f"{where.unread()} of {sum(where.chunk_rows())} rows were not read (chunks that do not decode: {where.chunk_matches()})")
        return where.total()

    if max_matches is not None and max_matches < 0:
        raise ValueError("max_matches must not be negative")
    total = call(None, 0) if max_matches is None else None      # the counting call
    capacity = total if max_matches is None else int(max_matches)
    dest, keep = mem.alloc(capacity * 8)
    if capacity:
        total = call(dest, capacity)
    elif total is None:
        total = call(None, 0)
    return keep[:min(total, capacity) * 8].view(torch.int64), total


class Aggregated(collections.namedtuple("Aggregated", "count nans sum min max argmin argmax chunks")):
    """What aggregate_rows answers: the rows counted, the NaNs among them (left out of the rest), the sum (an int, modulo 2^64 as the dtype's
    signedness reads it; a float for the floating-point dtypes), min and max as scalars of the table's dtype with the lowest row that holds
    each (None: no value), and `chunks`: the same per chunk (their own `chunks` is None)"""
    __slots__ = ()


def aggregate_rows(lib, container, offsets, meta, column=0, where=None, mem=None, stream=None):
    """count / sum / min / max / argmin / argmax of table.reshape(nrows, -1)[:, column] for the table pack_rows packed, without its plaintext and
    without an index table: ONE blosc_gpu_aggregate_packed (include/blosc_gpu_aggregate.h), which decodes pass by pass and keeps 64 bytes per
    chunk.  where=(op, value, column): only the rows whose `column` (any column of the row) satisfies the comparison, with where_rows' op names
    and value - rounded to a floating-point dtype as torch rounds it, ValueError if an integer or bool dtype does not hold it (1.5, a NaN,
    300 on uint8); None: every row.  The field's type is the table's dtype, as in where_rows.  NaNs are counted in `nans` and left out of sum, min
    and max; the floating-point sum is added in float64, in an order the chunk's row count fixes (the header has the rules).
    Returns an Aggregated; its `chunks` are the per-chunk results - their min and max are a zone map of the container.
    Raises, like where_rows, if the container does not hold this table or if any row was unread (a chunk that does not decode)."""
    import torch
    pkg = _sibling("", "__init__.py")
    pkg.declare_aggregate(lib)
    columns = (column,) if where is None else (column, where[2] if len(where) > 2 else 0)
    dtype, kind, element, row_bytes = _table_fields(pkg, meta, "blosc_gpu_aggregate_packed", *columns)
    pred = None if where is None else _where_predicate(pkg, dtype, kind, element, where[0], where[1], columns[1])
    agg = pkg.RowAggregate(row_bytes, lib=lib)
    if agg.packed(container.data_ptr(), int(container.numel()), list(offsets), pkg.field(kind, element, offset=column * element), pred, stream) != 0:
        raise RuntimeError(f"blosc_gpu_aggregate_packed failed; rows per chunk (negative: the chunk's code): {agg.chunk_rows()}")
    if agg.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {agg.chunk_rows()}")
    if agg.unread():
        raise RuntimeError(f"{agg.unread()} of {sum(agg.chunk_rows())} rows were not read (chunks that do not decode: {agg.chunk_status()})")

    def scalar(raw):
        return torch.tensor(list(raw[:element]), dtype=torch.uint8).view(dtype)[0].item()

    def result(a, chunks):
        total = a.sum.f if dtype.is_floating_point else (a.sum.i if kind == pkg.FIELD_INT else a.sum.u)
        return Aggregated(int(a.count), int(a.nans), total, scalar(a.min) if a.min_row >= 0 else None, scalar(a.max) if a.max_row >= 0 else None,
                          int(a.min_row) if a.min_row >= 0 else None, int(a.max_row) if a.max_row >= 0 else None, chunks)

    return result(agg.total(), [result(c, None) for c in agg.chunks()])


def _clause_terms(pkg, meta, call, clauses, *columns):
    """`clauses` as the list of Term a call of include/blosc_gpu_clauses.h takes, and what _table_fields reads from `meta` (`columns`: more
    columns to check).  clauses: a list that is ANDed; each entry is (op, value, column) or a list of such triples that is ORed - entry k is
    clause k.  op and value are where_rows': the value goes through _where_predicate unchanged.  ValueError for an entry that is neither, an
    empty OR list, more than 16 clauses and more than 16 terms"""
    groups = []
    for entry in clauses or []:
        group = [entry] if isinstance(entry, tuple) else list(entry) if isinstance(entry, list) else None
        if group is None or any(not isinstance(t, tuple) or len(t) != 3 for t in group):
            raise ValueError(f"clause {entry!r}: (op, value, column) or a list of such triples")
        if not group:
            raise ValueError("an OR list without a comparison matches no row: leave the clause out or give it one")
        groups.append(group)
    if len(groups) > pkg.MAX_TERMS or sum(map(len, groups)) > pkg.MAX_TERMS:
        raise ValueError(f"{len(groups)} clauses of {sum(map(len, groups))} terms: a call takes {pkg.MAX_TERMS} of each")
    dtype, kind, element, row_bytes = _table_fields(pkg, meta, call, *columns, *[t[2] for g in groups for t in g])
    terms = [pkg.term(_where_predicate(pkg, dtype, kind, element, op, value, column), k) for k, g in enumerate(groups) for op, value, column in g]
    return terms, dtype, kind, element, row_bytes


def where_rows_clauses(lib, container, offsets, meta, clauses, max_matches=None, mem=None, stream=None, zones=None):
    """where_rows for several comparisons at once: torch.nonzero of an AND of OR clauses over the columns of the table pack_rows packed, by
    blosc_gpu_where_clauses_packed (include/blosc_gpu_clauses.h) - one decode, whatever the number of comparisons.  clauses: a list that is
    ANDed; each entry is (op, value, column) or a list of such triples that is ORed:
        [(">=", t0, 0), ("<", t1, 0)]                        t0 <= column 0 < t1
        [(">=", t0, 0), [("==", 3, 1), ("==", 5, 1)]]        column 0 >= t0 and column 1 in {3, 5}
    op, value and column are where_rows', with the same rounding to a floating-point dtype and the same ValueError for a value an integer
    dtype does not hold; at most 16 comparisons in at most 16 clauses, at least one.  max_matches, the two calls without it, the result
    (index, total) and the errors raised are where_rows'.
    zones: a Zones of this container (zone_map) - the chunks whose entries show that no row can pass are not decoded
    (blosc_gpu_where_zoned_packed, include/blosc_gpu_zones.h); the answer is the same as long as the map describes the container.  A map that
    was not refreshed after put_rows makes the call miss rows: that is the caller's to prevent (Zones.refresh).  None: no map."""
    import torch
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_clauses(lib)
    terms, dtype, kind, element, row_bytes = _clause_terms(pkg, meta, "blosc_gpu_where_clauses_packed", clauses)
    if not terms:
        raise ValueError("where_rows_clauses takes at least one comparison")
    if zones is not None:
        zones.check(meta)
        pkg.declare_zones(lib)
    where = pkg.RowWhereClauses(row_bytes, lib=lib) if zones is None else pkg.RowWhereZoned(row_bytes, lib=lib)

    def call(ptr, capacity):
        if zones is None:
            rc = where.packed(container.data_ptr(), int(container.numel()), list(offsets), terms, ptr, capacity, stream)
        else:
            rc = where.packed(container.data_ptr(), int(container.numel()), list(offsets), terms, zones.fields, zones.table(pkg), ptr, capacity, stream)
        if rc != 0:
            raise RuntimeError(f"blosc_gpu_where_clauses_packed failed; rows per chunk (negative: the chunk's code): {where.chunk_rows()}")
        if where.chunk_rows() != [int(shape[0]) for _, shape in meta]:
            raise RuntimeError(f"the container does not hold this table: rows per chunk {where.chunk_rows()}")
        if where.unread():
            raise RuntimeError(f"{where.unread()} of {sum(where.chunk_rows())} rows were not read (chunks that do not decode: {where.chunk_matches()})")
        return where.total()

    if max_matches is not None and max_matches < 0:
        raise ValueError("max_matches must not be negative")
    total = call(None, 0) if max_matches is None else None      # the counting call
    capacity = total if max_matches is None else int(max_matches)
    dest, keep = mem.alloc(capacity * 8)
    if capacity:
        total = call(dest, capacity)
    elif total is None:
        total = call(None, 0)
    return keep[:min(total, capacity) * 8].view(torch.int64), total


def aggregate_rows_clauses(lib, container, offsets, meta, column=0, clauses=None, mem=None, stream=None, zones=None):
    """aggregate_rows over the rows that an AND of OR clauses lets through (clauses: where_rows_clauses'; None or empty: every row), by ONE
    blosc_gpu_aggregate_clauses_packed (include/blosc_gpu_clauses.h).  Returns an Aggregated, as aggregate_rows does, and raises as it does.
    zones: where_rows_clauses' - the chunks the map excludes are not decoded (blosc_gpu_aggregate_zoned_packed) and count no row."""
    import torch
    pkg = _sibling("", "__init__.py")
    pkg.declare_clauses(lib)
    terms, dtype, kind, element, row_bytes = _clause_terms(pkg, meta, "blosc_gpu_aggregate_clauses_packed", clauses, column)
    if zones is None:
        agg = pkg.RowAggregateClauses(row_bytes, lib=lib)
        rc = agg.packed(container.data_ptr(), int(container.numel()), list(offsets), pkg.field(kind, element, offset=column * element), terms, stream)
    else:
        zones.check(meta)
        pkg.declare_zones(lib)
        agg = pkg.RowAggregateZoned(row_bytes, lib=lib)
        rc = agg.packed(container.data_ptr(), int(container.numel()), list(offsets), pkg.field(kind, element, offset=column * element), terms, zones.fields,
                        zones.table(pkg), stream)
    if rc != 0:
        raise RuntimeError(f"blosc_gpu_aggregate_clauses_packed failed; rows per chunk (negative: the chunk's code): {agg.chunk_rows()}")
    if agg.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {agg.chunk_rows()}")
    if agg.unread():
        raise RuntimeError(f"{agg.unread()} of {sum(agg.chunk_rows())} rows were not read (chunks that do not decode: {agg.chunk_status()})")

    def scalar(raw):
        return torch.tensor(list(raw[:element]), dtype=torch.uint8).view(dtype)[0].item()

    def result(a, chunks):
        total = a.sum.f if dtype.is_floating_point else (a.sum.i if kind == pkg.FIELD_INT else a.sum.u)
        return Aggregated(int(a.count), int(a.nans), total, scalar(a.min) if a.min_row >= 0 else None, scalar(a.max) if a.max_row >= 0 else None,
                          int(a.min_row) if a.min_row >= 0 else None, int(a.max_row) if a.max_row >= 0 else None, chunks)

    return result(agg.total(), [result(c, None) for c in agg.chunks()])


def _aggregated(pkg, dtype, kind, element, a, chunks):
    """one blosc_gpu_aggregate of a column of this dtype as an Aggregated"""
    import torch
    def scalar(raw):
        return torch.tensor(list(raw[:element]), dtype=torch.uint8).view(dtype)[0].item()
    total = a.sum.f if dtype.is_floating_point else (a.sum.i if kind == pkg.FIELD_INT else a.sum.u)
    return Aggregated(int(a.count), int(a.nans), total, scalar(a.min) if a.min_row >= 0 else None, scalar(a.max) if a.max_row >= 0 else None,
                      int(a.min_row) if a.min_row >= 0 else None, int(a.max_row) if a.max_row >= 0 else None, chunks)


def _fields_call(pkg, lib, meta, columns, clauses, run):
    """blosc_gpu_aggregate_fields_* for `columns`: run(agg, fields, terms) makes the call on a RowAggregateFields and returns its answer.
    Returns (agg, fields, dtype, kind, element), the outputs checked as aggregate_rows checks them"""
    pkg.declare_zones(lib)
    columns = [int(c) for c in columns]
    if not 1 <= len(columns) <= pkg.MAX_ZONE_FIELDS:
        raise ValueError(f"{len(columns)} columns: a call takes 1 ... {pkg.MAX_ZONE_FIELDS}")
    terms, dtype, kind, element, row_bytes = _clause_terms(pkg, meta, "blosc_gpu_aggregate_fields_packed", clauses, *columns)
    fields = [pkg.field(kind, element, offset=c * element) for c in columns]
    agg = pkg.RowAggregateFields(row_bytes, lib=lib)
    if run(agg, fields, terms) != 0:
        raise RuntimeError(f"blosc_gpu_aggregate_fields failed; rows per chunk (negative: the chunk's code): {agg.chunk_rows()}")
    return agg, fields, dtype, kind, element


def aggregate_rows_fields(lib, container, offsets, meta, columns, where=None, mem=None, stream=None):
    """aggregate_rows for SEVERAL columns in one decode: ONE blosc_gpu_aggregate_fields_packed (include/blosc_gpu_zones.h) for up to 16
    columns, which may repeat.  where: None (every row), one (op, value, column), or a clause list as where_rows_clauses takes it.
    Returns a list with one Aggregated per column - each what aggregate_rows_clauses answers for that column alone, bit for bit - and raises
    as aggregate_rows does."""
    pkg = _sibling("", "__init__.py")
    clauses = [where] if isinstance(where, tuple) else where
    agg, fields, dtype, kind, element = _fields_call(pkg, lib, meta, columns, clauses, lambda a, f, t: a.packed(
        container.data_ptr(), int(container.numel()), list(offsets), f, t, stream))
    if agg.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {agg.chunk_rows()}")
    if agg.unread():
        raise RuntimeError(f"{agg.unread()} of {sum(agg.chunk_rows())} rows were not read (chunks that do not decode: {agg.chunk_status()})")
    per_chunk = agg.chunks()
    return [_aggregated(pkg, dtype, kind, element, total, [_aggregated(pkg, dtype, kind, element, c[f], None) for c in per_chunk])
            for f, total in enumerate(agg.totals())]


def _zone_dtype():
    import numpy as np
    return np.dtype([("rows", "<u8"), ("count", "<u8"), ("nans", "<u8"), ("min_row", "<i8"), ("max_row", "<i8"), ("min", "u1", 8), ("max", "u1", 8),
                     ("sum", "<u8")])      # blosc_gpu_aggregate, 64 bytes


class Zones:
    """A zone map of a table pack_rows packed: `columns`, their `fields` (the package's Field) and `entries`, a numpy array [chunks, columns]
    of blosc_gpu_aggregate records (rows, count, nans, min_row, max_row, min, max, sum; min and max as the column's 8 bytes, zero-extended) -
    what blosc_gpu_aggregate_fields_packed answers for every row of every chunk.  where_rows_clauses and aggregate_rows_clauses take it as
    `zones=` and skip the chunks it excludes.  The map describes the container it was computed from: after put_rows, refresh() the chunks
    that call rewrote (put_rows(..., return_rewritten=True)), or the zoned calls miss rows."""

    def __init__(self, columns, fields, entries):
        self.columns, self.fields, self.entries = list(columns), list(fields), entries

    def check(self, meta):
        if self.entries.shape != (len(meta), len(self.columns)):
            raise ValueError(f"a zone map of {self.entries.shape[0]} chunks for a container of {len(meta)}")

    def table(self, pkg):
        """the entries as the ctypes array the zoned calls take"""
        n = int(self.entries.size)
        return (pkg.Aggregate * max(n, 1)).from_buffer_copy(self.entries.tobytes() if n else bytes(64))

    def refresh(self, lib, container, offsets, meta, chunks):
        """Recompute the entries of the chunks numbered in `chunks` from `container` - the one put_rows returned - by ONE
        blosc_gpu_aggregate_fields_batch over those chunks' addresses: the others are neither decoded nor touched.  Returns self."""
        import numpy as np
        pkg = _sibling("", "__init__.py")
        self.check(meta)
        chunks = sorted({int(k) for k in chunks})
        if any(not 0 <= k < len(meta) for k in chunks):
            raise ValueError(f"chunks {chunks} of a container of {len(meta)}")
        if not chunks:
            return self
        base = container.data_ptr()
        agg, _, _, _, _ = _fields_call(pkg, lib, [meta[k] for k in chunks], self.columns, None,
                                       lambda a, f, t: a.batch([base + int(offsets[k]) for k in chunks], f, t))
        if agg.chunk_rows() != [int(meta[k][1][0]) for k in chunks] or agg.unread():
            raise RuntimeError(f"the container does not hold these chunks: rows {agg.chunk_rows()}, unread {agg.unread()}")
        fresh = np.frombuffer(bytes(agg.entries()), _zone_dtype())[:len(chunks) * len(self.columns)].reshape(len(chunks), len(self.columns)).copy()
        first = np.concatenate([[0], np.cumsum([int(shape[0]) for _, shape in meta])])
        at = 0      # the call numbered its rows from the first of ITS chunks: back to the table's numbers
        for i, k in enumerate(chunks):
            for name in ("min_row", "max_row"):
                fresh[name][i] = np.where(fresh[name][i] >= 0, fresh[name][i] - at + int(first[k]), -1)
            at += int(meta[k][1][0])
            self.entries[k] = fresh[i]
        return self


def zone_map(lib, container, offsets, meta, columns, mem=None, stream=None):
    """The zone map of `columns` (up to 16) of the table pack_rows packed: per chunk and column the minimum, the maximum, the NaNs and the
    rest of a blosc_gpu_aggregate over every row, by ONE blosc_gpu_aggregate_fields_packed (include/blosc_gpu_zones.h) - one decode of the
    container, whatever the number of columns.  Returns a Zones; raises as aggregate_rows does."""
    import numpy as np
    pkg = _sibling("", "__init__.py")
    agg, fields, _, _, _ = _fields_call(pkg, lib, meta, columns, None, lambda a, f, t: a.packed(
        container.data_ptr(), int(container.numel()), list(offsets), f, t, stream))
    if agg.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {agg.chunk_rows()}")
    if agg.unread():
        raise RuntimeError(f"{agg.unread()} of {sum(agg.chunk_rows())} rows were not read (chunks that do not decode: {agg.chunk_status()})")
    n = len(meta) * len(fields)
    entries = np.frombuffer(bytes(agg.entries()), _zone_dtype())[:n].reshape(len(meta), len(fields)).copy()
    return Zones(columns, fields, entries)


def put_rows(lib, container, offsets, meta, index, rows, mem=None, stream=None, align=256, return_rewritten=False, **settings):
    """table.index_copy_(0, index, rows) for the table pack_rows packed, by ONE blosc_gpu_put_packed (include/blosc_gpu_put.h): `index` is an
    int64 tensor on the device, `rows` a device tensor of the shape [len(index), *row shape] and the table's dtype; of an index that occurs
    several times the last occurrence wins.  Returns (new_container, new_offsets) - the container given is not written and `meta` stays what
    it is.  Only the chunks some row lands in are decoded and compressed again, with the typesize of the table's dtype and `settings`
    (cname / clevel / shuffle / blocksize / splitmode, pack_tensors' defaults); the others are copied.  Raises if any row failed (an index
    outside the table, a chunk that does not decode), naming how many.
    return_rewritten=True: returns (new_container, new_offsets, rewritten) - the numbers of the chunks that were decoded and compressed again,
    which are the chunks whose entries of a zone map no longer hold (Zones.refresh)."""
    import torch
    pkg = _sibling("", "__init__.py")
    mem = mem if mem is not None else _sibling("blpk", "blpk.py").TorchMem()
    pkg.declare_put(lib)
    pkg.declare_packed(lib)
    dtype, row_shape = meta[0][0], tuple(meta[0][1][1:])
    if any(dt != dtype or tuple(shape[1:]) != row_shape for dt, shape in meta):
        raise ValueError("the container's chunks are not slices of one table")
    element = int(torch.empty(0, dtype=dtype).element_size())
    row_bytes = element * int(torch.Size(row_shape).numel())
    if not 1 <= row_bytes <= 65536:
        raise ValueError(f"rows of {row_bytes} bytes: blosc_gpu_put_packed takes 1 ... 65536")
    if index.dtype != torch.int64 or index.dim() != 1 or not index.is_cuda:
        raise ValueError("index: a one-dimensional int64 tensor on the device")
    n = int(index.numel())
    if rows.dtype != dtype or tuple(rows.shape) != (n,) + row_shape or not rows.is_cuda:
        raise ValueError(f"rows: a device tensor of dtype {dtype} and shape {(n,) + row_shape}")
    idx, new = index.contiguous(), rows.contiguous()
    kw = dict(cname=b"lz4", clevel=5, shuffle=1)
    kw.update(settings)
    params = [pkg.cparams(element, **kw) for _ in meta]
    sizes = [element * int(torch.Size(shape).numel()) for _, shape in meta]
    cap = pkg.PackedBatch(len(meta), lib=lib).bound(sizes, align)
    if cap == 0 and any(sizes):
        raise ValueError("align must be a power of two up to 4096")
    dest, keep = mem.alloc(cap)
    put = pkg.RowPut(row_bytes, lib=lib)
    if put.packed(container.data_ptr(), int(container.numel()), list(offsets), idx.data_ptr() if n else None, n, new.data_ptr() if n else None, params,
                  dest, cap, align, None, stream) != 0:
        raise RuntimeError(f"blosc_gpu_put_packed failed; rows per chunk (negative: the chunk's code): {put.chunk_rows()}")
    if put.chunk_rows() != [int(shape[0]) for _, shape in meta]:
        raise RuntimeError(f"the container does not hold this table: rows per chunk {put.chunk_rows()}")
    if put.failed():
        raise RuntimeError(f"{put.failed()} of {n} rows failed (an index outside 0 ... {sum(put.chunk_rows()) - 1}, or a chunk that does not decode)")
    off = put.offsets()
    if return_rewritten:
        return keep[:off[-1]], off, [k for k, r in enumerate(put.rewritten()) if r == 1]
    return keep[:off[-1]], off
