"""CPU, the built library, no device: blosc_gpu_zone_excludes (include/blosc_gpu_zones.h) against numpy brute force.

A chunk is 1 ... 5 values of a field; its entry is what an unfiltered aggregate answers for it (rows, count = rows, the NaNs, the first rows
that hold the extremes and their bytes).  For every op and constant the rule's answer is held two ways:
  soundness   whenever the answer is 1, numpy's own comparison finds no value of the chunk that passes;
  tightness   the answer equals the header's table, computed here from numpy's minimum and maximum of the values that are no NaN.
Term lists of 2 ... 16 terms over 1 ... 16 clauses and 1 ... 3 zone fields are drawn from a seed and held the same two ways (the table per
term, then "some clause without a term that can be true").  Every form of an entry that carries no information answers 0."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import where_checks as W
from where_checks import BFLOAT16, FLOAT, INT, UINT
from zones_checks import entry_of, is_nan, passes, table_says, values_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EQ, NE, LT, LE, GT, GE = range(6)


@pytest.fixture(scope="module")
def pkgmod():
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_zone_rule", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
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
    assert hasattr(lib, "blosc_gpu_zone_excludes"), "the library has no zone rule"
    return pkgmod.declare_zones(lib)


def neighbours(p, kind, nbytes):
    """the patterns next to p in the order of the keys: an integer's value - 1 and + 1 (wrapped inside the width), a floating-point
    pattern's magnitude - 1 and + 1 under its sign"""
    top = (1 << 8 * nbytes) - 1
    if kind in (UINT, INT):
        return [(p - 1) & top, (p + 1) & top]
    sign = 1 << (8 * nbytes - 1)
    mag = p & (sign - 1)
    return [(p & sign) | ((mag - 1) & (sign - 1)), (p & sign) | ((mag + 1) & (sign - 1))]


def float_set(kind, nbytes):
    """every class with both signs - zero, subnormals, normals, infinities, NaN patterns of both signs - and for binary64 the two pairs"""
    r, sign = W.regime(kind, nbytes), 1 << (8 * nbytes - 1)
    return W.regime_set(kind, nbytes) + [sign | r["quiet_nan"]] + (W.LOW_PAIR + W.HIGH_PAIR if nbytes == 8 else [])


def cases_of(kind, nbytes):
    """(the value set, the chunks, the constants) of one kind"""
    rng = np.random.default_rng(100 * kind + nbytes)
    if nbytes == 1:
        values = list(range(256))
    elif (kind, nbytes) == (INT, 2):
        values = [0x8000, 0x8001, 0x8002, 0xfffe, 0xffff, 0, 1, 2, 0x7ffd, 0x7ffe, 0x7fff]
    elif (kind, nbytes) == (UINT, 4):
        values = [0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1]
    else:
        values = float_set(kind, nbytes)
    nchunks = 40 if nbytes == 1 else 60
    chunks = [[int(values[i]) for i in rng.integers(0, len(values), int(n))] for n in rng.integers(1, 6, nchunks)]
    if kind in (FLOAT, BFLOAT16):
        r, sign = W.regime(kind, nbytes), 1 << (8 * nbytes - 1)
        nan, one = r["quiet_nan"], r["one"]
        chunks += [[nan], [nan, sign | r["first_nan"], nan], [one, nan, r["min_sub"]], [nan, sign | one], [one], [one, one, one], [one, nan, one],
                   [sign, 0], [0, sign], [sign], [r["inf"], sign | r["inf"]], [sign | r["max_sub"], r["min_sub"]]]
    else:
        chunks += [[values[0]], [values[-1]] * 3, [values[0], values[-1]]]
    constants = set(values)
    if nbytes > 1:
        for p in values:
            constants.update(neighbours(p, kind, nbytes))
    if kind in (FLOAT, BFLOAT16):
        constants.add(W.regime(kind, nbytes)["quiet_nan"])
    return values, chunks, sorted(constants)


RULE_KINDS = [(UINT, 1), (INT, 1), (INT, 2), (UINT, 4), (FLOAT, 2), (BFLOAT16, 2), (FLOAT, 4), (FLOAT, 8)]


@pytest.mark.parametrize("kind,nbytes", RULE_KINDS, ids=[W.kind_name(*k) for k in RULE_KINDS])
def test_single_terms_are_sound_and_tight(pkgmod, L, kind, nbytes):
    values, chunks, constants = cases_of(kind, nbytes)
    if kind in (FLOAT, BFLOAT16):      # the classes the issue names are all there
        nan = is_nan(values, kind, nbytes)
        v = values_of(values, kind, nbytes)
        assert nan.sum() >= 4 and np.isinf(v).sum() == 2 and (v[~nan] == 0).sum() == 2
    zf = (pkgmod.Field * 1)(pkgmod.field(kind, nbytes, offset=3))
    term = (pkgmod.Term * 1)(pkgmod.term(W.predicate(pkgmod, kind, nbytes, EQ, 0, 3), 7))
    answers = [0, 0]
    for chunk in chunks:
        entry = (pkgmod.Aggregate * 1)(entry_of(pkgmod, chunk, kind, nbytes))
        for constant in constants:
            raw = int(constant).to_bytes(nbytes, "little")
            for i in range(nbytes):
                term[0].test.value[i] = raw[i]
            for op in range(6):
                term[0].test.op = op
                got = L.blosc_gpu_zone_excludes(term, 1, zf, 1, entry, len(chunk))
                what = (W.kind_name(kind, nbytes), [hex(p) for p in chunk], W.OPS[op].__name__, hex(constant), got)
                assert got in (0, 1), what
                if got == 1:
                    assert not passes(chunk, kind, nbytes, op, constant).any(), ("unsound", what)
                assert got == (0 if table_says(chunk, kind, nbytes, op, constant) else 1), ("not the header's table", what)
                answers[got] += 1
    assert min(answers) > len(chunks), answers      # both answers occur, and often


def draw_list(rng, layout, sets):
    """(terms as (field number, op, constant pattern, clause), nclauses) of one seeded list"""
    nterms = int(rng.integers(2, 17))
    nclauses = int(rng.integers(1, min(nterms, 16) + 1))
    names = rng.permutation(16)[:nclauses]
    clauses = [int(names[i]) for i in range(nclauses)] + [int(names[i]) for i in rng.integers(0, nclauses, nterms - nclauses)]
    terms = []
    for clause in clauses:
        f = int(rng.integers(0, len(layout)))
        pool = sets[f]
        constant = int(pool[int(rng.integers(0, len(pool)))])
        if rng.integers(0, 3) == 0:
            constant = neighbours(constant, layout[f][1], layout[f][2])[int(rng.integers(0, 2))]
        terms.append((f, int(rng.integers(0, 6)), constant, clause))
    return terms


def test_term_lists_are_sound(pkgmod, L):
    """seeded lists of 2 ... 16 terms over 1 ... 16 clauses; the row has four fields, 1 ... 3 of which have a zone"""
    layout = [(0, UINT, 1), (2, FLOAT, 2), (4, INT, 2), (8, FLOAT, 8)]
    sets = [[0, 1, 2, 3, 250, 255], float_set(FLOAT, 2), [0x8000, 0xffff, 0, 1, 0x7fff], float_set(FLOAT, 8)]
    rng = np.random.default_rng(77)
    answers = [0, 0]
    for trial in range(1500):
        nrows = int(rng.integers(1, 6))
        narrow = trial % 3 == 0      # few distinct values: chunks that a list can exclude
        chunk = []
        for s in sets:
            pool = [s[int(i)] for i in rng.integers(0, len(s), 2)] if narrow else s
            chunk.append([int(pool[int(i)]) for i in rng.integers(0, len(pool), nrows)])
        zoned = sorted(int(f) for f in rng.permutation(4)[:int(rng.integers(1, 4))])
        terms = draw_list(rng, layout, sets)
        table = (pkgmod.Term * len(terms))(*[pkgmod.term(W.predicate(pkgmod, layout[f][1], layout[f][2], op, c, layout[f][0]), clause) for f, op, c, clause in terms])
        zf = (pkgmod.Field * len(zoned))(*[pkgmod.field(layout[f][1], layout[f][2], offset=layout[f][0]) for f in zoned])
        entry = (pkgmod.Aggregate * len(zoned))(*[entry_of(pkgmod, chunk[f], layout[f][1], layout[f][2]) for f in zoned])
        got = L.blosc_gpu_zone_excludes(table, len(terms), zf, len(zoned), entry, nrows)
        assert got in (0, 1), (trial, got)
        row_passes = np.ones(nrows, bool)
        excluded = False
        for clause in {t[3] for t in terms}:
            mine = [t for t in terms if t[3] == clause]
            hit = np.zeros(nrows, bool)
            for f, op, c, _ in mine:
                hit |= passes(chunk[f], layout[f][1], layout[f][2], op, c)
            row_passes &= hit
            excluded |= not any(f not in zoned or table_says(chunk[f], layout[f][1], layout[f][2], op, c) for f, op, c, _ in mine)
        if got == 1:
            assert not row_passes.any(), ("unsound", trial, terms, chunk, zoned)
        assert got == int(excluded), ("not the header's rule", trial, terms, chunk, zoned, got)
        answers[got] += 1
    assert min(answers) >= 100, answers


def test_entries_without_information_never_exclude(pkgmod, L):
    chunk = [5, 6, 9]
    zf = (pkgmod.Field * 1)(pkgmod.field(UINT, 4, offset=4))
    term = (pkgmod.Term * 1)(pkgmod.term(W.predicate(pkgmod, UINT, 4, EQ, 1, 4), 0))

    def ask(change=None, rows=3, fields=zf):
        e = entry_of(pkgmod, chunk, UINT, 4)
        if change: change(e)
        return L.blosc_gpu_zone_excludes(term, 1, fields, 1, (pkgmod.Aggregate * 1)(e), rows)

    assert ask() == 1      # the entry as it is excludes: 1 lies outside 5 ... 9
    assert ask(lambda e: setattr(e, "rows", 0)) == 0
    assert ask(lambda e: (setattr(e, "rows", 0), setattr(e, "count", 0)), rows=0) == 0
    assert ask(rows=4) == 0 and ask(rows=2) == 0 and ask(rows=0) == 0
    assert ask(lambda e: setattr(e, "count", 2)) == 0 and ask(lambda e: setattr(e, "count", 4)) == 0      # a filtered aggregate
    assert ask(lambda e: setattr(e, "min_row", -1)) == 0 and ask(lambda e: setattr(e, "max_row", -1)) == 0
    assert ask(lambda e: (setattr(e, "min_row", -1), setattr(e, "max_row", -1), setattr(e, "nans", 2))) == 0
    # the same bytes under another kind or width, and another offset: not this term's zone
    for other in (pkgmod.field(INT, 4, offset=4), pkgmod.field(FLOAT, 4, offset=4), pkgmod.field(UINT, 2, offset=4), pkgmod.field(UINT, 8, offset=4),
                  pkgmod.field(UINT, 4, offset=0)):
        assert ask(fields=(pkgmod.Field * 1)(other)) == 0
    # an entry without information in front of one that informs: the second is used
    two = (pkgmod.Field * 2)(zf[0], zf[0])
    blind = entry_of(pkgmod, chunk, UINT, 4)
    blind.count = 1
    assert L.blosc_gpu_zone_excludes(term, 1, two, 2, (pkgmod.Aggregate * 2)(blind, entry_of(pkgmod, chunk, UINT, 4)), 3) == 1
    # all NaN: nothing but NE can be true, and the rows of the extremes are -1
    nan = W.regime(FLOAT, 4)["quiet_nan"]
    ff = (pkgmod.Field * 1)(pkgmod.field(FLOAT, 4, offset=4))
    e = (pkgmod.Aggregate * 1)(entry_of(pkgmod, [nan, nan], FLOAT, 4))
    assert (e[0].min_row, e[0].max_row, e[0].nans) == (-1, -1, 2)
    for op in range(6):
        t = (pkgmod.Term * 1)(pkgmod.term(W.predicate(pkgmod, FLOAT, 4, op, 0x3f800000, 4), 0))
        assert L.blosc_gpu_zone_excludes(t, 1, ff, 1, e, 2) == (0 if op == NE else 1)
