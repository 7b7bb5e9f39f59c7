"""CPU: the constant that tensors.where_rows and tensors.aggregate_rows hand to the library (c-blosc_amd/tensors.py: _where_predicate), without
a library call.  The Predicate it returns is evaluated here as the kernels read it - its `value` bytes as a pattern of its kind, compared by
where_checks.comparable / OPS - on a small torch column that holds the constant's neighbours, and the answer is torch's own op(column, value)
on the CPU: what the docstrings of the two calls promise.  A floating-point dtype takes any number, rounded as torch rounds the scalar; an
integer or bool dtype takes the values it holds and raises ValueError, naming value and dtype, for every other."""
import importlib.util
import math
import operator
import os
import re

import numpy as np
import pytest

from test_gpu_where import DTYPES
import where_checks as W

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["eq", "ne", "lt", "le", "gt", "ge"]      # W.OPS' order
FLOAT_DTYPES = [d for d in DTYPES if getattr(torch, d).is_floating_point]
INT_DTYPES = [d for d in DTYPES if d not in FLOAT_DTYPES]


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pkgmod():
    return load("c_blosc_amd_for_predicate_cpu", "__init__.py")


@pytest.fixture(scope="module")
def tensors():
    return load("c_blosc_amd_tensors_predicate_cpu", "tensors.py")


def fields(tensors, pkgmod, dt):
    """(kind, element size) of a table of this dtype, as where_rows reads them from `meta`"""
    _, kind, element, _ = tensors._table_fields(pkgmod, [(dt, (4, 3))], "the test", 1)
    return kind, element


def column_of_patterns(patterns, dt, element):
    """the torch column whose elements have these unsigned patterns"""
    signed = np.ascontiguousarray(patterns, dtype=f"<u{element}").view(f"<i{element}")
    return torch.from_numpy(signed.copy()).view(dt)


def library_answer(pred, patterns, kind, element):
    """what the kernels answer for rows whose field has these patterns: numpy's comparison of the patterns with the predicate's value bytes"""
    constant = int.from_bytes(bytes(pred.value)[:element], "little")
    assert bytes(pred.value)[element:] == bytes(8 - element) and (pred.kind, pred.bytes) == (kind, element)
    with np.errstate(invalid="ignore"):
        return np.asarray(W.OPS[pred.op](W.comparable(patterns, kind, element), W.comparable([constant], kind, element)[0]))


def check_against_torch(tensors, pkgmod, dt, patterns, value):
    """all six ops, by name and as the function of `operator`: the predicate's answer on the column is torch's op(column, value)"""
    kind, element = fields(tensors, pkgmod, dt)
    col = column_of_patterns(patterns, dt, element)
    for at, name in enumerate(NAMES):
        fn = getattr(operator, name)
        pred = tensors._where_predicate(pkgmod, dt, kind, element, name if at % 2 else fn, value, column=1)
        assert (pred.op, pred.offset) == (at, element)
        got, want = library_answer(pred, patterns, kind, element), fn(col, value).numpy()
        assert np.array_equal(got, want), (dt, name, value, [hex(int(p)) for p in np.asarray(patterns)[got != want]])


FLOAT_VALUES = [0.1, -0.1, 1e6, 65520.0, 1e39, math.inf, -math.inf, math.nan, 1, 2 ** 24 + 1]


@pytest.mark.parametrize("value", FLOAT_VALUES, ids=[repr(v) for v in FLOAT_VALUES])
@pytest.mark.parametrize("dtype", FLOAT_DTYPES)
def test_a_floating_point_constant_is_rounded_as_torch_rounds_it(tensors, pkgmod, dtype, value):
    """0.1 is no value of any of them, 1e6 and 65520 become inf on float16, 1e39 on float32 and bfloat16, 2^24 + 1 is no float32: the column
    holds the rounded constant, the patterns next to it on both sides and their negatives, both zeros, both infinities, a NaN and +-1"""
    dt = getattr(torch, dtype)
    kind, element = fields(tensors, pkgmod, dt)
    bits = 8 * element
    sign, top = 1 << (bits - 1), (1 << bits) - 1
    p = int.from_bytes(bytes(torch.tensor([value], dtype=dt).view(torch.uint8).tolist()), "little")
    one = int.from_bytes(bytes(torch.tensor([1.0], dtype=dt).view(torch.uint8).tolist()), "little")
    inf = int.from_bytes(bytes(torch.tensor([math.inf], dtype=dt).view(torch.uint8).tolist()), "little")
    near = [q & top for q in (p - 2, p - 1, p, p + 1, p + 2)]
    patterns = near + [q ^ sign for q in near] + [0, sign, inf, inf | sign, inf - 1, (inf - 1) | sign, inf + 1, one, one | sign, 1, sign | 1]
    check_against_torch(tensors, pkgmod, dt, np.array(patterns, dtype=np.uint64), value)


def int_range(dt):
    return (0, 1) if dt == torch.bool else (torch.iinfo(dt).min, torch.iinfo(dt).max)


def int_patterns(dt, element, around):
    """the dtype's extremes, 0 and 1, and `around` with its two neighbours where the dtype holds them"""
    low, high = int_range(dt)
    values = {low, high, 0, 1} | {v for v in (around - 1, around, around + 1) if low <= v <= high}
    return np.array([v % (1 << (8 * element)) for v in sorted(values)], dtype=np.uint64)


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_an_integer_dtype_takes_the_values_it_holds(tensors, pkgmod, dtype):
    """its extremes, 0 and 1 as int, as integral float and as bool: torch's comparison on a column of the value's neighbours"""
    dt = getattr(torch, dtype)
    kind, element = fields(tensors, pkgmod, dt)
    low, high = int_range(dt)
    values = [low, high, 0, 1, 1.0, 0.0, True, False] + ([] if dt == torch.bool else [2.0, high - 1, low + 1, np.int64(1)])
    if element <= 2:      # (torch compares an integer column with a float scalar in float32: beyond 2^24 its own answer is no longer the integers')
        values += [float(low), float(high)]
    for value in values:
        check_against_torch(tensors, pkgmod, dt, int_patterns(dt, element, int(value)), value)


def rejected(dt):
    low, high = int_range(dt)
    values = [1.5, -0.5, math.nan, math.inf, -math.inf, high + 1, low - 1, high + 0.5, "1"]
    values += {torch.uint8: [300, -1], torch.bool: [2, -1, 0.5], torch.int32: [2 ** 31, 2.0 ** 31], torch.int64: [2 ** 63, -2 ** 63 - 1, 2.0 ** 63]}.get(dt, [])
    return values


@pytest.mark.parametrize("dtype", INT_DTYPES)
def test_an_integer_dtype_refuses_every_other_value(tensors, pkgmod, dtype):
    """a non-integral float, a NaN, an infinity, an integer outside the range: ValueError that names the value and the dtype - never an error
    out of torch, never the predicate of another constant"""
    dt = getattr(torch, dtype)
    kind, element = fields(tensors, pkgmod, dt)
    for value in rejected(dt):
        for op in ("lt", operator.eq):
            with pytest.raises(ValueError, match=re.escape(repr(value))) as caught:
                tensors._where_predicate(pkgmod, dt, kind, element, op, value, column=0)
            assert str(dt) in str(caught.value), (dtype, value, str(caught.value))


def test_an_op_nobody_knows_is_refused_first(tensors, pkgmod):
    with pytest.raises(ValueError, match="like"):
        tensors._where_predicate(pkgmod, torch.int32, W.INT, 4, "like", 1.5, column=0)
