"""CPU: the clause-list builder of tensors.where_rows_clauses / aggregate_rows_clauses (c-blosc_amd/tensors.py: _clause_terms), without a
library call: the shapes it takes, the raw terms it makes of them - every value through _where_predicate, entry k of the list as clause k -
and the ValueError for what it does not take."""
import importlib.util
import os

import pytest

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(name, file):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "c-blosc_amd", file))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pkgmod():
    return load("c_blosc_amd_for_clauses_cpu", "__init__.py")


@pytest.fixture(scope="module")
def tensors():
    mod = load("c_blosc_amd_tensors_clauses_cpu", "tensors.py")
    assert hasattr(mod, "where_rows_clauses") and hasattr(mod, "aggregate_rows_clauses"), "tensors.py has no clause calls"
    return mod


def raw(terms):
    """(offset, bytes, kind, op, the value's bytes, clause) of every term"""
    return [(t.test.offset, t.test.bytes, t.test.kind, t.test.op, bytes(t.test.value)[:t.test.bytes], t.clause) for t in terms]


def test_the_shapes_it_takes(tensors, pkgmod):
    meta = [(torch.float32, (10, 4)), (torch.float32, (7, 4))]
    terms, dtype, kind, element, row_bytes = tensors._clause_terms(pkgmod, meta, "the test", [(">=", 0.5, 0), ("lt", 2.0, 0)])
    assert (dtype, kind, element, row_bytes) == (torch.float32, pkgmod.FIELD_FLOAT, 4, 16)
    assert raw(terms) == [(0, 4, 2, 5, b"\x00\x00\x00\x3f", 0), (0, 4, 2, 2, b"\x00\x00\x00\x40", 1)]
    assert all(t.pad_ == 0 for t in terms)
    # an OR list is one clause; a triple next to it the next one; entry k is clause k
    terms, *_ = tensors._clause_terms(pkgmod, meta, "the test", [[("==", 1.0, 3), ("==", 2.0, 3), ("!=", -0.0, 1)], (">", 0.1, 2)])
    assert [(t[0], t[3], t[5]) for t in raw(terms)] == [(12, 0, 0), (12, 0, 0), (4, 1, 0), (8, 4, 1)]
    assert raw(terms)[3][4] == bytes(torch.tensor([0.1], dtype=torch.float32).view(torch.uint8).tolist())      # rounded to the dtype, as where_rows does
    # the same predicate as where_rows' own builder gives
    one = tensors._where_predicate(pkgmod, torch.float32, pkgmod.FIELD_FLOAT, 4, ">", 0.1, 2)
    assert bytes(terms[3].test) == bytes(one)
    # an OR list of one is the triple; no clauses at all: no terms (aggregate: every row)
    a, *_ = tensors._clause_terms(pkgmod, meta, "the test", [[("le", 3, 1)]])
    b, *_ = tensors._clause_terms(pkgmod, meta, "the test", [("le", 3, 1)])
    assert raw(a) == raw(b) and len(a) == 1
    for nothing in (None, []):
        assert tensors._clause_terms(pkgmod, meta, "the test", nothing)[0] == []
    # 16 terms in one clause, 16 clauses of one term
    many, *_ = tensors._clause_terms(pkgmod, meta, "the test", [[("==", float(k), k % 4) for k in range(16)]])
    assert len(many) == 16 and {t.clause for t in many} == {0}
    many, *_ = tensors._clause_terms(pkgmod, meta, "the test", [("!=", float(k), k % 4) for k in range(16)])
    assert [t.clause for t in many] == list(range(16))
    # an int16 table: integers as they are, negative ones in two's complement
    terms, dtype, kind, element, row_bytes = tensors._clause_terms(pkgmod, [(torch.int16, (5, 4))], "the test", [("ge", -2, 3), [("eq", 300, 0), ("eq", 2.0, 1)]])
    assert (kind, element, row_bytes) == (pkgmod.FIELD_INT, 2, 8)
    assert raw(terms) == [(6, 2, 1, 5, b"\xfe\xff", 0), (0, 2, 1, 0, b"\x2c\x01", 1), (2, 2, 1, 0, b"\x02\x00", 1)]


def test_what_it_refuses(tensors, pkgmod):
    meta = [(torch.int16, (10, 4))]
    build = lambda clauses, *columns: tensors._clause_terms(pkgmod, meta, "the test", clauses, *columns)
    with pytest.raises(ValueError, match="17"):
        build([[("eq", k, 0) for k in range(17)]])
    with pytest.raises(ValueError, match="17"):
        build([("ne", k, 0) for k in range(17)])
    with pytest.raises(ValueError, match="17"):
        build([[("eq", k, 0) for k in range(9)], [("eq", k, 1) for k in range(8)]])
    with pytest.raises(ValueError, match="OR list"):
        build([("eq", 1, 0), []])
    for value in (1.5, float("nan"), 40000, -32769):      # none that int16 holds: _where_predicate's error, value and dtype named
        with pytest.raises(ValueError, match="int16"):
            build([("eq", 1, 0), [("lt", value, 1)]])
    with pytest.raises(ValueError, match="op"):
        build([("almost", 1, 0)])
    with pytest.raises(ValueError, match="column"):
        build([("eq", 1, 4)])
    with pytest.raises(ValueError, match="column"):
        build([("eq", 1, 0)], 4)      # the aggregated column
    for entry in ("eq", ("eq", 1), [("eq", 1, 0, 0)], [["eq", 1, 0]]):
        with pytest.raises(ValueError, match="triples"):
            build([entry])
    with pytest.raises(ValueError, match="at least one"):
        tensors.where_rows_clauses(None, None, [0], meta, [])
