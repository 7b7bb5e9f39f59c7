"""CPU, no library: aggregate_checks.tree_sum, the numpy model of the order of additions that include/blosc_gpu_aggregate.h documents, which
check_aggregate holds every chunk's floating-point sum against bit for bit.  Two things about the model itself: on the exact-sum windows,
where every order gives the same binary64, it is math.fsum; and on the rounding inputs of case_tall_chunks its bits differ from every rival
below - each a tree that a kernel could run in place of the documented one - so a kernel that ran a rival would fail that case.  The second
is a condition on the inputs: were a seed to leave a rival equal, the inputs change, never the list."""
import math

import numpy as np
import pytest

import aggregate_checks as A

TILE, LANES = A.TILE_ROWS, A.LANES


def padded(x, unit):
    out = np.zeros(-(-max(x.size, 1) // unit) * unit)
    out[:x.size] = x
    return out


def butterfly(v, ds):
    """[m, 64] -> [m]: lane l takes lane l ^ d for d in ds, the lower lane's operand in front; lane 0's result"""
    for d in ds:
        v = v + v[:, np.arange(64) ^ d]      # (both operands of an addition commute: the order in front / behind does not change the bits)
    return v[:, 0]


def workgroup(acc, ds=(32, 16, 8, 4, 2, 1)):
    """[m, 256] -> [m]: every wave by butterfly(ds), the four waves in order"""
    w = butterfly(acc.reshape(-1, 64), ds).reshape(-1, 4)
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def tiles_of(x, consecutive=False, ds=(32, 16, 8, 4, 2, 1)):
    """the tile partials: lane l adds rows l, l + 256, ... (consecutive: rows 4 l ... 4 l + 3)"""
    rows = padded(x, TILE).reshape(-1, TILE)
    rows = rows.reshape(-1, LANES, 4).transpose(0, 2, 1) if consecutive else rows.reshape(-1, 4, LANES)
    acc = np.zeros((rows.shape[0], LANES))
    for s in range(4):
        acc = acc + rows[:, s, :]
    return workgroup(acc, ds)


def chunk_of(partials, stride=LANES, ds=(32, 16, 8, 4, 2, 1)):
    """the chunk's sum from its tile partials: lane l of `stride` adds partials l, l + stride, ...; the other lanes hold +0.0"""
    turns = padded(partials, stride).reshape(-1, stride)
    acc = np.zeros((1, LANES))
    for t in range(turns.shape[0]):
        acc[0, :stride] = acc[0, :stride] + turns[t]
    return float(workgroup(acc, ds)[0])


def running(x):
    s = 0.0
    for v in x.tolist():
        s += v
    return s


RIVALS = {
    "one running sum in row order": running,
    "numpy.sum": lambda x: float(np.sum(x)),
    "the butterfly from d = 1 up to 32": lambda x: chunk_of(tiles_of(x, ds=(1, 2, 4, 8, 16, 32)), ds=(1, 2, 4, 8, 16, 32)),
    "four consecutive rows per lane": lambda x: chunk_of(tiles_of(x, consecutive=True)),
    "tile partials in tile order by one accumulator": lambda x: running(tiles_of(x)),
    "a chunk-level stride of 64": lambda x: chunk_of(tiles_of(x), stride=64),
    "a chunk-level stride of 128": lambda x: chunk_of(tiles_of(x), stride=128),
}


def test_the_rival_built_like_the_model_is_the_model():
    """tiles_of / chunk_of with the documented parameters - written with an explicit l ^ d butterfly, not the model's halving - give tree_sum's
    bits: the rivals differ from the model by their one changed parameter, not by how this file is written"""
    x = A.comparable(A.tall_patterns(), A.FLOAT, 8).astype(np.float64)
    for n in (1, 63, 1024, 1025, 262144, 262145, 524289):
        assert A.f64_bits(chunk_of(tiles_of(x[:n]))) == A.f64_bits(A.tree_sum(x[:n])), n


@pytest.mark.parametrize("kind,nbytes", A.FLOATS, ids=[A.kind_name(*k) for k in A.FLOATS])
def test_the_model_is_fsum_on_the_exact_sum_windows(kind, nbytes):
    for w, patterns in enumerate(A.WINDOWS[(kind, nbytes)]()):
        A.assert_exact_window(patterns, kind, nbytes)
        x = A.comparable(patterns, kind, nbytes).astype(np.float64)
        for sel in (x, np.where(x > 0, x, 0.0), np.where(x < 0, x, 0.0), x[:x.size * 3 // 8], x[:1]):
            assert A.tree_sum(sel) == math.fsum(sel.tolist()), (A.kind_name(kind, nbytes), w)


def test_zeros_nans_and_infinities():
    assert A.f64_bits(A.tree_sum(np.zeros(0))) == 0 and A.f64_bits(A.tree_sum(np.full(5000, -0.0))) == 0      # never -0.0
    assert A.f64_bits(A.tree_sum(np.array([-0.0, 1.5, -1.5]))) == 0
    assert A.tree_sum(np.array([1.0, np.inf, 2.0])) == np.inf and math.isnan(A.tree_sum(np.array([np.inf] + [0.0] * 2000 + [-np.inf])))
    assert A.tree_sum(np.full(3, 1.7e308)) == np.inf


def test_the_rounding_inputs_separate_every_rival():
    """every chunk of case_tall_chunks that is taller than 256 tiles, and the 256-tile one for the rivals that differ inside a tile,
    unfiltered and under GT +0"""
    x = A.comparable(A.tall_patterns(), A.FLOAT, 8).astype(np.float64)
    assert np.all(np.isfinite(x)) and (x > 0).any() and (x < 0).any()
    first = np.concatenate([[0], np.cumsum(A.TALL_ROWS)])
    for k, rows in enumerate(A.TALL_ROWS):
        if rows < 262144: continue
        for name, chunk in (("unfiltered", x[first[k]:first[k + 1]]), ("GT +0", np.where(x[first[k]:first[k + 1]] > 0, x[first[k]:first[k + 1]], 0.0))):
            model = A.tree_sum(chunk)
            want = A.float_sum(chunk)
            assert want[0] == "finite" and abs(A.Fraction(model) - A.Fraction(want[1])) <= want[2]
            assert model != want[1], (rows, name, "the model is fsum: the sum does not round")
            for rival, fn in RIVALS.items():
                assert A.f64_bits(fn(chunk)) != A.f64_bits(model), (rows, name, "not separated from", rival)
