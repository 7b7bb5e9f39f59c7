"""CPU: include/blosc_gpu_clauses.h against the Python loader and the built library - the declared names, the exported symbols, the header as
C, sizeof(blosc_gpu_term), and the whole-call answers that need no device: every refusal the header lists leaves every host output at its
sentinel; the calls without chunks answer 0 with a total of nothing."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_clauses_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    assert hasattr(pkgmod, "CLAUSES_SYMBOLS"), "the loader has no clause calls"
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_where_clauses_packed"), "the library has no clause calls"
    return pkgmod.declare_clauses(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_clauses.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.CLAUSES_SYMBOLS) and len(set(declared)) == len(declared) == 4, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS + pkgmod.TAKE_SYMBOLS + pkgmod.PUT_SYMBOLS + pkgmod.WHERE_SYMBOLS + pkgmod.AGGREGATE_SYMBOLS)
    assert not set(pkgmod.CLAUSES_SYMBOLS) & set(others)
    for s in pkgmod.CLAUSES_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    outs = "size_t*, int*, int*, size_t*, void*"
    aggs = "const blosc_gpu_field*, const blosc_gpu_term*, int, blosc_gpu_aggregate*, blosc_gpu_aggregate*, int*, int*, size_t*, void*"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_clauses.h"\n'
                   f'int (*wb)(int, const void* const*, size_t, const blosc_gpu_term*, int, int64_t*, size_t, {outs}) = blosc_gpu_where_clauses_batch;\n'
                   f'int (*wp)(int, const void*, size_t, const size_t*, size_t, const blosc_gpu_term*, int, int64_t*, size_t, {outs}) = blosc_gpu_where_clauses_packed;\n'
                   f'int (*ab)(int, const void* const*, size_t, {aggs}) = blosc_gpu_aggregate_clauses_batch;\n'
                   f'int (*ap)(int, const void*, size_t, const size_t*, size_t, {aggs}) = blosc_gpu_aggregate_clauses_packed;\n'
                   'blosc_gpu_term range[2] = {{{0, 4, BLOSC_GPU_FIELD_FLOAT, BLOSC_GPU_WHERE_GE, {0, 0, 192, 63}}, 0, 0},\n'
                   '                           {{0, 4, BLOSC_GPU_FIELD_FLOAT, BLOSC_GPU_WHERE_LT, {0, 0, 0, 64}}, 1, 0}};\n'
                   'int sizes[sizeof(blosc_gpu_term) == 32 && BLOSC_GPU_MAX_TERMS == 16 ? 1 : -1];\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


def test_the_term_builder(pkgmod):
    assert C.sizeof(pkgmod.Term) == 32 and pkgmod.MAX_TERMS == 16
    t = pkgmod.term(pkgmod.predicate(pkgmod.FIELD_INT, 2, pkgmod.WHERE_LT, -2, offset=3), 15)
    assert (t.test.offset, t.test.bytes, t.test.kind, t.test.op, bytes(t.test.value[:2]), t.clause, t.pad_) == (3, 2, 1, 2, b"\xfe\xff", 15, 0)
    assert bytes(t)[24:] == bytes([15, 0, 0, 0, 0, 0, 0, 0])
    for clause in (-1, 16):
        with pytest.raises(ValueError):
            pkgmod.term(pkgmod.predicate(pkgmod.FIELD_UINT, 1, 0, 0), clause)
    table, n = pkgmod.terms_table([t, t])
    assert n == 2 and C.sizeof(table) == 64 and pkgmod.terms_table([]) == (None, 0) and pkgmod.terms_table(None) == (None, 0)


SENT = 0xA5


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    falls, beyond = (sz * 3)(0, 40, 32), (sz * 3)(0, 32, 65)
    rows, matches, status, total, unread = (i * 2)(-7, -7), (i * 2)(-8, -8), (i * 2)(-9, -9), sz(77), sz(78)
    agg_total, agg_chunks = pkgmod.Aggregate(), (pkgmod.Aggregate * 2)()
    idx, cont = vp(4096), vp(12288)      # addresses nobody reads: every call below is answered from its arguments
    wouts = (C.byref(total), matches, rows, C.byref(unread), None)
    aouts = (C.byref(agg_total), agg_chunks, status, rows, C.byref(unread), None)
    wb, wp, ab, ap = (getattr(L, s) for s in pkgmod.CLAUSES_SYMBOLS)
    fld = pkgmod.field(pkgmod.FIELD_UINT, 4, offset=0)

    def fresh():
        C.memset(C.byref(agg_total), SENT, 64)
        C.memset(agg_chunks, SENT, 128)
        total.value, unread.value = 77, 78

    def untouched():
        return ((list(rows), list(matches), list(status), total.value, unread.value) == ([-7, -7], [-8, -8], [-9, -9], 77, 78)
                and bytes(agg_total) == bytes([SENT]) * 64 and bytes(agg_chunks) == bytes([SENT]) * 128)

    def listed(*terms):
        return (pkgmod.Term * len(terms))(*terms), len(terms)

    def refused(terms, nterms, rb=8, n=2, s=src, c=cont, o=off, table=idx, cap=4, size=64, f=fld, where=True, aggregate=True):
        fp = C.byref(f) if f is not None else None
        if where:
            assert wb(n, s, rb, terms, nterms, table, cap, *wouts) < 0
            assert wp(n, c, size, o, rb, terms, nterms, table, cap, *wouts) < 0
        if aggregate:
            assert ab(n, s, rb, fp, terms, nterms, *aouts) < 0
            assert ap(n, c, size, o, rb, fp, terms, nterms, *aouts) < 0
        assert untouched()

    fresh()
    P = pkgmod.Predicate
    good = pkgmod.term(pkgmod.predicate(pkgmod.FIELD_UINT, 4, pkgmod.WHERE_EQ, 1, offset=4), 0)
    other = pkgmod.term(pkgmod.predicate(pkgmod.FIELD_INT, 2, pkgmod.WHERE_LT, -1, offset=1), 3)
    one, _ = listed(good)
    # where: terms NULL, nterms outside 1 ... 16;  aggregate: nterms outside 0 ... 16, NULL with terms, terms without a count
    refused(None, 1)
    refused(None, 0, aggregate=False)
    refused(one, 0)
    refused(one, -1)
    seventeen, _ = listed(*[good] * 17)
    refused(seventeen, 17)
    # a clause above 15, a pad_ that is not 0 - in the first and in the last term of a list
    for bad in (pkgmod.Term(good.test, 16, 0), pkgmod.Term(good.test, 2 ** 32 - 1, 0), pkgmod.Term(good.test, 0, 1)):
        refused(*listed(bad))
        refused(*listed(good, other, bad))
    # a term that blosc_gpu_where_* would refuse: op, the kind / bytes pair, a field that ends behind the row
    for op in (-1, 6):
        refused(*listed(good, pkgmod.Term(P(0, 4, pkgmod.FIELD_UINT, op), 1, 0)))
    for kind, nbytes in ((pkgmod.FIELD_UINT, 0), (pkgmod.FIELD_UINT, 3), (pkgmod.FIELD_INT, 16), (pkgmod.FIELD_FLOAT, 1), (pkgmod.FIELD_FLOAT, 3),
                         (pkgmod.FIELD_BFLOAT16, 4), (pkgmod.FIELD_BFLOAT16, 1), (-1, 4), (4, 4)):
        refused(*listed(pkgmod.Term(P(0, nbytes, kind, pkgmod.WHERE_EQ), 0, 0), good))
    refused(*listed(good, pkgmod.Term(P(5, 4, pkgmod.FIELD_UINT, pkgmod.WHERE_EQ), 0, 0)))
    refused(*listed(pkgmod.Term(P(2 ** 32 - 2, 4, pkgmod.FIELD_UINT, pkgmod.WHERE_EQ), 0, 0)))
    # the whole-call checks of the existing calls: the row size (also without chunks), a negative count, NULL tables
    small = listed(pkgmod.term(pkgmod.predicate(pkgmod.FIELD_UINT, 1, 0, 0), 0))
    for rb in (0, 65537):
        refused(*small, rb=rb, f=pkgmod.field(pkgmod.FIELD_UINT, 1))
        refused(*small, rb=rb, n=0, s=None, c=None, o=None, table=None, cap=0, f=pkgmod.field(pkgmod.FIELD_UINT, 1))
    refused(one, 1, n=-1)
    refused(one, 1, s=None, c=None)
    refused(one, 1, s=None, o=None)
    # where's: a capacity without a table, a table inside the container;  aggregate's: no field, its pad_, its pair, its end behind the row
    refused(one, 1, table=None, aggregate=False)
    assert wp(2, cont, 64, off, 8, one, 1, vp(12288 + 56), 1, *wouts) < 0 and untouched()
    refused(one, 1, f=None, where=False)
    refused(one, 1, f=pkgmod.Field(0, 4, pkgmod.FIELD_UINT, 1), where=False)
    refused(one, 1, f=pkgmod.Field(0, 3, pkgmod.FIELD_UINT, 0), where=False)
    refused(one, 1, f=pkgmod.Field(6, 4, pkgmod.FIELD_UINT, 0), where=False)
    refused(None, 0, f=pkgmod.Field(6, 4, pkgmod.FIELD_UINT, 0), where=False)
    # an offset table that decreases, or ends behind the container
    for o, size in ((falls, 64), (beyond, 64), (off, 63)):
        assert wp(2, cont, size, o, 8, one, 1, None, 0, *wouts) < 0 and ap(2, cont, size, o, 8, C.byref(fld), one, 1, *aouts) < 0 and untouched()
    # no chunks: a total of 0, no unread row, no table entry written; the aggregate of nothing - with terms and without
    for call in (lambda: wb(0, None, 8, one, 1, None, 0, *wouts), lambda: wp(0, None, 0, None, 8, one, 1, idx, 4, *wouts)):
        fresh()
        assert call() == 0
        assert (list(rows), list(matches), total.value, unread.value) == ([-7, -7], [-8, -8], 0, 0)
    assert wb(0, None, 8, one, 1, None, 0, None, None, None, None, None) == 0
    for call in (lambda: ab(0, None, 8, C.byref(fld), None, 0, *aouts), lambda: ap(0, None, 0, None, 8, C.byref(fld), None, 0, *aouts),
                 lambda: ab(0, None, 8, C.byref(fld), one, 1, *aouts)):
        fresh()
        assert call() == 0
        a = agg_total
        assert (a.rows, a.count, a.nans, a.min_row, a.max_row, bytes(a.min), bytes(a.max), a.sum.u) == (0, 0, 0, -1, -1, bytes(8), bytes(8), 0)
        assert unread.value == 0 and (list(rows), list(status)) == ([-7, -7], [-9, -9]) and bytes(agg_chunks) == bytes([SENT]) * 128
    assert ab(0, None, 8, C.byref(fld), None, 0, None, None, None, None, None, None) == 0
