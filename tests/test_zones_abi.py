"""CPU: include/blosc_gpu_zones.h against the Python loader and the built library - the declared names, the exported symbols, the header as C,
and the whole-call answers that need no device: every refusal the header lists leaves every host output at its sentinel; the calls without
chunks answer 0 with totals of nothing."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_zones_abi", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def L(pkgmod):
    assert hasattr(pkgmod, "ZONES_SYMBOLS"), "the loader has no zone calls"
    so = os.path.join(ROOT, "c-blosc_amd", "libblosc_amd.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "c-blosc_amd")], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    assert hasattr(lib, "blosc_gpu_where_zoned_packed"), "the library has no zone calls"
    return pkgmod.declare_zones(lib)


def test_header_names_equal_the_loaders_list(pkgmod, L):
    text = open(os.path.join(ROOT, "include", "blosc_gpu_zones.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = re.findall(r"BLOSC_EXPORT\s+[\w\s\*]*?\b(blosc_gpu_\w+)\s*\(", text)
    assert sorted(declared) == sorted(pkgmod.ZONES_SYMBOLS) and len(set(declared)) == len(declared) == 7, declared
    others = (pkgmod.STOCK_SYMBOLS + pkgmod.GPU_SYMBOLS + pkgmod.PACKED_SYMBOLS + pkgmod.GETITEM_SYMBOLS + pkgmod.CHECKSUM_SYMBOLS + pkgmod.PARAMS_SYMBOLS
              + pkgmod.SELECT_SYMBOLS + pkgmod.TAKE_SYMBOLS + pkgmod.PUT_SYMBOLS + pkgmod.WHERE_SYMBOLS + pkgmod.AGGREGATE_SYMBOLS + pkgmod.CLAUSES_SYMBOLS)
    assert not set(pkgmod.ZONES_SYMBOLS) & set(others)
    for s in pkgmod.ZONES_SYMBOLS:
        assert hasattr(L, s) and s in pkgmod.SIGNATURES, s
    assert "BLOSC_GPU_MAX_ZONE_FIELDS = 16" in text and pkgmod.MAX_ZONE_FIELDS == 16
    assert '#include "blosc_gpu_clauses.h"' in text


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    aggs = "blosc_gpu_aggregate*, blosc_gpu_aggregate*, int*, int*, size_t*"
    flds = f"const blosc_gpu_field*, int, const blosc_gpu_term*, int, {aggs}, void*"
    zone = "const blosc_gpu_field*, int, const blosc_gpu_aggregate*"
    wz = f"const blosc_gpu_term*, int, {zone}, int64_t*, size_t, size_t*, int*, int*, size_t*, uint8_t*, void*"
    az = f"const blosc_gpu_field*, const blosc_gpu_term*, int, {zone}, {aggs}, uint8_t*, void*"
    src.write_text('#include "blosc.h"\n#include "blosc_gpu_zones.h"\n'
                   f'int (*fb)(int, const void* const*, size_t, {flds}) = blosc_gpu_aggregate_fields_batch;\n'
                   f'int (*fp)(int, const void*, size_t, const size_t*, size_t, {flds}) = blosc_gpu_aggregate_fields_packed;\n'
                   f'int (*ex)(const blosc_gpu_term*, int, {zone}, uint64_t) = blosc_gpu_zone_excludes;\n'
                   f'int (*wb)(int, const void* const*, size_t, {wz}) = blosc_gpu_where_zoned_batch;\n'
                   f'int (*wp)(int, const void*, size_t, const size_t*, size_t, {wz}) = blosc_gpu_where_zoned_packed;\n'
                   f'int (*ab)(int, const void* const*, size_t, {az}) = blosc_gpu_aggregate_zoned_batch;\n'
                   f'int (*ap)(int, const void*, size_t, const size_t*, size_t, {az}) = blosc_gpu_aggregate_zoned_packed;\n'
                   'int sizes[BLOSC_GPU_MAX_ZONE_FIELDS == 16 && sizeof(blosc_gpu_aggregate) == 64 ? 1 : -1];\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "use.o")])


SENT = 0xA5


def test_calls_that_need_no_device(pkgmod, L):
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    src, off = (vp * 2)(64, 64), (sz * 3)(0, 32, 64)
    rows, matches, status, total, unread = (i * 2)(-7, -7), (i * 2)(-8, -8), (i * 2)(-9, -9), sz(77), sz(78)
    pruned = (C.c_uint8 * 2)(SENT, SENT)
    totals, per_chunk = (pkgmod.Aggregate * 16)(), (pkgmod.Aggregate * 32)()
    idx, cont = vp(4096), vp(12288)      # addresses nobody reads: every call below is answered from its arguments
    fb, fp, ex, wb, wp, ab, ap = (getattr(L, s) for s in pkgmod.ZONES_SYMBOLS)
    F, T, P = pkgmod.Field, pkgmod.Term, pkgmod.Predicate
    fld = pkgmod.field(pkgmod.FIELD_UINT, 4, offset=0)
    good = pkgmod.term(pkgmod.predicate(pkgmod.FIELD_UINT, 4, pkgmod.WHERE_EQ, 1, offset=4), 0)
    one = (T * 1)(good)
    zones = (pkgmod.Aggregate * 32)()

    def fresh():
        C.memset(totals, SENT, 64 * 16)
        C.memset(per_chunk, SENT, 64 * 32)
        total.value, unread.value = 77, 78

    def untouched():
        return ((list(rows), list(matches), list(status), total.value, unread.value, list(pruned)) == ([-7, -7], [-8, -8], [-9, -9], 77, 78, [SENT, SENT])
                and bytes(totals) == bytes([SENT]) * 1024 and bytes(per_chunk) == bytes([SENT]) * 2048)

    def fields(*rows_):
        return ((F * len(rows_))(*rows_) if rows_ else None), len(rows_)

    def fields_refused(ftab, nf, terms=None, nterms=0, rb=8, n=2, s=src, c=cont, o=off, size=64):
        outs = (totals, per_chunk, status, rows, C.byref(unread), None)
        assert fb(n, s, rb, ftab, nf, terms, nterms, *outs) < 0
        assert fp(n, c, size, o, rb, ftab, nf, terms, nterms, *outs) < 0
        assert untouched()

    def zoned_refused(ztab, nz, zmap=zones, terms=one, nterms=1, rb=8, n=2, s=src, c=cont, o=off, size=64, f=fld, table=idx, cap=4, where=True, aggregate=True):
        if where:
            wouts = (table, cap, C.byref(total), matches, rows, C.byref(unread), pruned, None)
            assert wb(n, s, rb, terms, nterms, ztab, nz, zmap, *wouts) < 0
            assert wp(n, c, size, o, rb, terms, nterms, ztab, nz, zmap, *wouts) < 0
        if aggregate:
            aouts = (totals, per_chunk, status, rows, C.byref(unread), pruned, None)
            fptr = C.byref(f) if f is not None else None
            assert ab(n, s, rb, fptr, terms, nterms, ztab, nz, zmap, *aouts) < 0
            assert ap(n, c, size, o, rb, fptr, terms, nterms, ztab, nz, zmap, *aouts) < 0
        assert untouched()

    fresh()
    bad_fields = [F(0, 4, pkgmod.FIELD_UINT, 1), F(0, 3, pkgmod.FIELD_UINT, 0), F(6, 4, pkgmod.FIELD_UINT, 0), F(0, 4, pkgmod.FIELD_BFLOAT16, 0),
                  F(0, 1, pkgmod.FIELD_FLOAT, 0), F(0, 4, 4, 0), F(2 ** 32 - 2, 4, pkgmod.FIELD_UINT, 0)]
    # ---- the fields call: nfields outside 1 ... 16, fields NULL, a field or a term the clause call would refuse, its whole-call checks ----
    fields_refused(None, 1)
    fields_refused(*fields(), )
    fields_refused((F * 1)(fld), 0)
    fields_refused((F * 1)(fld), -1)
    fields_refused((F * 17)(*[fld] * 17), 17)
    for bad in bad_fields:
        fields_refused(*fields(bad))
        fields_refused(*fields(*[fld] * 15, bad))
    ok = fields(fld, fld)
    fields_refused(*ok, terms=None, nterms=1)
    fields_refused(*ok, terms=one, nterms=0)
    fields_refused(*ok, terms=(T * 17)(*[good] * 17), nterms=17)
    for bad in (T(good.test, 16, 0), T(good.test, 0, 1), T(P(0, 4, pkgmod.FIELD_UINT, 6), 0, 0), T(P(0, 3, pkgmod.FIELD_UINT, 0), 0, 0),
                T(P(5, 4, pkgmod.FIELD_UINT, 0), 0, 0)):
        fields_refused(*ok, terms=(T * 2)(good, bad), nterms=2)
    for rb in (0, 65537):
        fields_refused(*fields(pkgmod.field(pkgmod.FIELD_UINT, 1)), rb=rb)
    fields_refused(*ok, n=-1)
    fields_refused(*ok, s=None, c=None)
    fields_refused(*ok, s=None, o=None)
    for o, size in (((sz * 3)(0, 40, 32), 64), ((sz * 3)(0, 32, 65), 64), (off, 63)):
        assert fp(2, cont, size, o, 8, *ok, None, 0, totals, per_chunk, status, rows, C.byref(unread), None) < 0 and untouched()
    # ---- the zoned calls: nzfields outside 0 ... 16, NULL tables with a count, a zone field the aggregate call would refuse ----
    zok = fields(fld)
    zoned_refused(zok[0], -1)
    zoned_refused((F * 17)(*[fld] * 17), 17)
    zoned_refused(None, 1)
    zoned_refused(zok[0], 1, zmap=None)
    for bad in bad_fields:
        zoned_refused(*fields(bad))
        zoned_refused(*fields(fld, bad))
    # ... and everything the clause calls refuse
    zoned_refused(*zok, terms=None, nterms=1)
    zoned_refused(*zok, terms=None, nterms=0, aggregate=False)
    zoned_refused(*zok, terms=one, nterms=0)
    zoned_refused(*zok, terms=(T * 1)(T(good.test, 16, 0)))
    zoned_refused(*zok, terms=(T * 1)(T(P(5, 4, pkgmod.FIELD_UINT, 0), 0, 0)))
    zoned_refused(*zok, rb=0)
    zoned_refused(*zok, n=-1)
    zoned_refused(*zok, s=None, c=None)
    zoned_refused(*zok, table=None, aggregate=False)
    zoned_refused(*zok, f=None, where=False)
    zoned_refused(*zok, f=F(6, 4, pkgmod.FIELD_UINT, 0), where=False)
    assert wp(2, cont, 64, off, 8, one, 1, *zok, zones, vp(12288 + 56), 1, C.byref(total), matches, rows, C.byref(unread), pruned, None) < 0 and untouched()
    # ---- no chunks: the totals of nothing, nothing else written ----
    for call in (lambda: fb(0, None, 8, *ok, None, 0, totals, per_chunk, status, rows, C.byref(unread), None),
                 lambda: fp(0, None, 0, None, 8, *ok, one, 1, totals, per_chunk, status, rows, C.byref(unread), None)):
        fresh()
        assert call() == 0
        for a in list(totals)[:2]:
            assert (a.rows, a.count, a.nans, a.min_row, a.max_row, bytes(a.min), bytes(a.max), a.sum.u) == (0, 0, 0, -1, -1, bytes(8), bytes(8), 0)
        assert bytes(totals)[128:] == bytes([SENT]) * (1024 - 128) and bytes(per_chunk) == bytes([SENT]) * 2048
        assert unread.value == 0 and (list(rows), list(status)) == ([-7, -7], [-9, -9])
    assert fb(0, None, 8, *ok, None, 0, None, None, None, None, None, None) == 0
    for call in (lambda: wb(0, None, 8, one, 1, *zok, zones, None, 0, C.byref(total), matches, rows, C.byref(unread), pruned, None),
                 lambda: wp(0, None, 0, None, 8, one, 1, None, 0, None, idx, 4, C.byref(total), matches, rows, C.byref(unread), pruned, None)):
        fresh()
        assert call() == 0
        assert (list(rows), list(matches), total.value, unread.value, list(pruned)) == ([-7, -7], [-8, -8], 0, 0, [SENT, SENT])
    for call in (lambda: ab(0, None, 8, C.byref(fld), None, 0, *zok, zones, totals, per_chunk, status, rows, C.byref(unread), pruned, None),
                 lambda: ap(0, None, 0, None, 8, C.byref(fld), one, 1, None, 0, None, totals, per_chunk, status, rows, C.byref(unread), pruned, None)):
        fresh()
        assert call() == 0
        a = totals[0]
        assert (a.rows, a.count, a.nans, a.min_row, a.max_row, bytes(a.min), bytes(a.max), a.sum.u) == (0, 0, 0, -1, -1, bytes(8), bytes(8), 0)
        assert bytes(totals)[64:] == bytes([SENT]) * (1024 - 64) and unread.value == 0 and (list(rows), list(status), list(pruned)) == ([-7, -7], [-9, -9], [SENT, SENT])
    assert wb(0, None, 8, one, 1, None, 0, None, None, 0, None, None, None, None, None, None) == 0


def test_the_rule_refuses_bad_arguments(pkgmod, L):
    F, T, P, A = pkgmod.Field, pkgmod.Term, pkgmod.Predicate, pkgmod.Aggregate
    ex = L.blosc_gpu_zone_excludes
    fld = pkgmod.field(pkgmod.FIELD_UINT, 4, offset=4)
    good = pkgmod.term(pkgmod.predicate(pkgmod.FIELD_UINT, 4, pkgmod.WHERE_EQ, 1, offset=4), 0)
    entry = A(10, 10, 0, 0, 9, (C.c_uint8 * 8)(5), (C.c_uint8 * 8)(9), pkgmod.AggregateSum(u=0))
    one, zf, e = (T * 1)(good), (F * 1)(fld), (A * 1)(entry)
    assert ex(one, 1, zf, 1, e, 10) == 1            # 1 lies outside 5 ... 9
    assert ex(one, 1, zf, 1, e, 11) == 0            # another chunk's entry: no information
    assert ex(None, 0, zf, 1, e, 10) == 0 and ex(one, 1, None, 0, None, 10) == 0 and ex(None, 0, None, 0, None, 0) == 0
    assert ex(one, -1, zf, 1, e, 10) < 0 and ex((T * 17)(*[good] * 17), 17, zf, 1, e, 10) < 0 and ex(None, 1, zf, 1, e, 10) < 0
    assert ex(one, 1, zf, -1, e, 10) < 0 and ex(one, 1, (F * 17)(*[fld] * 17), 17, (A * 17)(), 10) < 0
    assert ex(one, 1, None, 1, e, 10) < 0 and ex(one, 1, zf, 1, None, 10) < 0
    for bad in (T(good.test, 16, 0), T(good.test, 0, 1), T(P(4, 4, pkgmod.FIELD_UINT, 6), 0, 0), T(P(4, 3, pkgmod.FIELD_UINT, 0), 0, 0), T(P(4, 4, 7, 0), 0, 0)):
        assert ex((T * 2)(good, bad), 2, zf, 1, e, 10) < 0
    for bad in (F(4, 4, pkgmod.FIELD_UINT, 1), F(4, 3, pkgmod.FIELD_UINT, 0), F(4, 4, pkgmod.FIELD_BFLOAT16, 0)):
        assert ex(one, 1, (F * 1)(bad), 1, e, 10) < 0
