"""CPU: where_terms_test (c-blosc_amd/csrc/row_prims.h) alone on the wavefront emulator - the per-row evaluation of a term list that
k_where_mark_terms and k_aggregate_tiles_terms share, the SAME source the GPU runs - over truth tables, in the manner of
tests/test_wave_emu_row_prims.py.  The list is given in the kernels' own form (dev_types.h: WhereTerms), which this file builds by itself:
the distinct fields, the terms sorted by field, a bit per clause.  The host's way to that form is tests/test_emu_clauses.py's business."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

from helpers import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
MAX_TERMS, MAX_FIELDS = 16, 17


class Pred(C.Structure):      # dev_types.h: WherePred
    _fields_ = [("offset", C.c_uint32), ("bytes", C.c_uint32), ("kind", C.c_int32), ("op", C.c_int32), ("key", C.c_int64), ("inf", C.c_uint64),
                ("nan", C.c_int32), ("pad_", C.c_int32)]


class Terms(C.Structure):     # dev_types.h: WhereTerms
    _fields_ = [("nterms", C.c_uint32), ("nfields", C.c_uint32), ("clauses", C.c_uint32), ("pad_", C.c_uint32), ("offset", C.c_uint32 * MAX_FIELDS),
                ("bytes", C.c_uint32 * MAX_FIELDS), ("first", C.c_uint32 * (MAX_FIELDS + 1)), ("bit", C.c_uint32 * MAX_TERMS), ("test", Pred * MAX_TERMS)]


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(CLANG):
        pytest.skip("the emulator needs the ROCm clang++ (ext_vector_type / address_space in host code)")
    csrc, tools = os.path.join(ROOT, "c-blosc_amd", "csrc"), os.path.join(ROOT, "tests", "tools")
    src, so = os.path.join(tools, "clauses_wave_cpu.cpp"), os.path.join(tools, "libclauses_wave_cpu.so")
    assert os.path.exists(src), "no entry point for where_terms_test"
    deps = [src, os.path.join(tools, "wave_emu", "wave_emu.h")] + [os.path.join(csrc, f) for f in ("row_prims.h", "dev_types.h", "mem_prims.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call([CLANG, "-std=c++17", "-O1", "-shared", "-fPIC", "-w", "-I", os.path.join(tools, "wave_emu"), "-I", csrc, "-x", "c++", src, "-o", so])
    E = C.CDLL(so)
    E.emu_terms_test.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    E.emu_terms_test.restype = None
    assert E.emu_terms_sizeof() == C.sizeof(Terms), "this file's WhereTerms is not dev_types.h's"
    return E


def build(fields, terms):
    """fields: [(offset, bytes)]; terms: [(field, op, constant, clause)], every one an unsigned comparison.  The kernels' form of it"""
    q = Terms()
    q.nfields = len(fields)
    for f, (offset, nbytes) in enumerate(fields):
        q.offset[f], q.bytes[f] = offset, nbytes
    for f in range(len(fields)):
        q.first[f] = q.nterms
        for field, op, constant, clause in terms:
            if field == f:
                key = (constant ^ (1 << 63)) - (1 << 64 if not constant >> 63 else 0)      # where_key of UINT: bit 63 flipped, read as signed
                q.test[q.nterms] = Pred(fields[f][0], fields[f][1], 0, op, key, 0, 0, 0)
                q.bit[q.nterms] = 1 << clause
                q.clauses |= 1 << clause
                q.nterms += 1
    for f in range(len(fields), MAX_FIELDS + 1):
        q.first[f] = q.nterms
    assert q.nterms == len(terms)
    return q


def run(emu, q, rows):
    """(pass per row, field 0 per row) for a [nrows, row_bytes] uint8 table, which ends at the end of its buffer"""
    rows = np.ascontiguousarray(rows, np.uint8)
    got, v0 = np.full(rows.shape[0] + 8, 0xEE, np.uint8), np.zeros(rows.shape[0], np.uint64)
    emu.emu_terms_test(C.addressof(q), ptr(rows), rows.shape[1], rows.shape[0], ptr(got), ptr(v0))
    assert np.all(got[rows.shape[0]:] == 0xEE)
    return got[:rows.shape[0]].astype(bool), v0


def expected(truth, clauses):
    """truth [nrows, nterms]: a row passes when every clause that occurs has a true term"""
    want = np.ones(truth.shape[0], bool)
    for c in set(clauses):
        want &= truth[:, [k for k, x in enumerate(clauses) if x == c]].any(axis=1)
    return want


PARTITIONS3 = [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 1, 2]]      # the five partitions of three terms into clauses


@pytest.mark.parametrize("clauses", PARTITIONS3, ids=lambda p: "".join(map(str, p)))
@pytest.mark.parametrize("numbers", [(0, 1, 2), (15, 7, 0)], ids=["clauses 0 1 2", "clauses 15 7 0"])
def test_every_subset_of_three_terms(emu, clauses, numbers):
    """term k is true where byte k of the row is 1: the eight rows are the eight subsets; rows of 3 bytes, then 64 + 5 rows so that a second
    wave step with idle lanes runs"""
    truth = np.array(list(itertools.product([0, 1], repeat=3)), np.uint8)
    truth = np.concatenate([truth] * 8 + [truth[:5]])
    named = [numbers[c] for c in clauses]
    q = build([(0, 1), (1, 1), (2, 1)], [(k, 0, 1, named[k]) for k in range(3)])
    got, v0 = run(emu, q, truth)
    assert np.array_equal(got, expected(truth.astype(bool), named)), (clauses, numbers)
    assert np.array_equal(v0, truth[:, 0].astype(np.uint64))


EXTREMES = {"16 clauses": list(range(16)), "one clause": [4] * 16, "15 + 1": [11] * 9 + [3] + [11] * 6}


@pytest.mark.parametrize("name", list(EXTREMES))
def test_sixteen_terms(emu, name):
    """16 terms on 16 one-byte fields: no term true, all true, every single one true, every single one false, and 2000 random subsets"""
    clauses = EXTREMES[name]
    rng = np.random.default_rng(16)
    eye = np.eye(16, dtype=np.uint8)
    truth = np.concatenate([np.zeros((1, 16), np.uint8), np.ones((1, 16), np.uint8), eye, 1 - eye, (rng.random((2000, 16)) < 0.8).astype(np.uint8),
                            (rng.random((2000, 16)) < 0.1).astype(np.uint8)])
    q = build([(k, 1) for k in range(16)], [(k, 0, 1, clauses[k]) for k in range(16)])
    got, _ = run(emu, q, truth)
    want = expected(truth.astype(bool), clauses)
    assert np.array_equal(got, want), name
    assert want.any() and not want.all() and want[1] and not want[0]


def test_several_terms_on_one_field_and_a_field_without_terms(emu):
    """the aggregate's form: field 0 (8 bytes at an odd offset) has no term and is loaded all the same; field 1 (2 bytes) carries a range
    with a hole in three clauses and field 2 (4 bytes) two terms of one clause; a list without terms lets every row through"""
    rng = np.random.default_rng(3)
    nrows = 300
    rows = rng.integers(0, 256, (nrows, 17), dtype=np.uint8)
    a = rng.integers(0, 12, nrows).astype("<u2")
    b = rng.integers(0, 5, nrows).astype("<u4") * np.uint32(0x01000001)
    rows[:, 9:11] = a.view(np.uint8).reshape(nrows, 2)
    rows[:, 11:15] = b.view(np.uint8).reshape(nrows, 4)
    fields = [(1, 8), (9, 2), (11, 4)]
    q = build(fields, [(1, 5, 3, 0), (1, 2, 9, 1), (1, 1, 6, 2), (2, 0, 0x02000002, 1), (2, 4, 0x03000003, 2)])      # GE 3, LT 9 | b == 2.., NE 6 | b > 3..
    got, v0 = run(emu, q, rows)
    want = (a >= 3) & ((a < 9) | (b == 0x02000002)) & ((a != 6) | (b > 0x03000003))
    assert np.array_equal(got, want) and want.any() and not want.all()
    assert np.array_equal(v0, np.ascontiguousarray(rows[:, 1:9]).view("<u8").ravel())
    got, v0 = run(emu, build(fields[:1], []), rows)
    assert got.all() and np.array_equal(v0, np.ascontiguousarray(rows[:, 1:9]).view("<u8").ravel())
