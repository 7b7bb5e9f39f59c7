"""GPU: the device batch and row calls while other calls of the library are in flight - from several threads, on the NULL stream and on
streams of the callers' own (include/blosc_gpu.h, INTEGRATION.md 8: up to BLOSC_AMD_CONTEXTS callers side by side, the rest wait their
turn).  The workers, the recording proxy and the runner are tests/concurrent_checks.py's: every repetition is checked in full by its
family's checker and must equal, byte for byte, the serial call made before the threads existed.

The overlap condition of every in-process test: in at least half of its rounds two calls of different threads have logged intervals that
overlap.  With no more threads than contexts nobody waits for a context, a call holds its context from entry to return, and two overlapping
intervals are two contexts in use.  The counts seen go into the failure message (and are printed: -s shows them)."""
import os
import subprocess
import sys

import pytest

import concurrent_checks as cc
import where_checks as wh
from getitem_ranges_checks import SMALL, TorchMem, plain

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "BLOSC_CONCURRENT_CALLS_CHILD"      # set in the child process of test_two_contexts_only: it spawns no further one
PASS_BYTES = 16 << 10


@pytest.fixture(scope="module")
def env(pkg, lib, oracle, ref):
    made = cc.Env(pkg, cc.Recorder(lib), TorchMem(), oracle, ref)
    yield made
    made.close()      # (the global split mode, as it was found)


def streams(tid):
    import torch
    s = torch.cuda.Stream()
    return s, s.cuda_stream


def on_stream(s):
    import torch
    return torch.cuda.stream(s)      # the thread's torch work - fills, uploads, read-backs - is ordered on the same stream as the call


@pytest.fixture(scope="module")
def rows(env):
    """take, put, where, aggregate: four row sizes under the deterministic writers; a float32 and an int64 field"""
    tables, fields = cc.row_tables(env), cc.field_tables(env)
    return [cc.TakeWorker(env, tables).serial(), cc.PutWorker(env, tables).serial(), cc.WhereWorker(env, fields).serial(), cc.AggregateWorker(env, fields).serial()]


@pytest.fixture(scope="module")
def families(env, rows):
    """the eight families, one worker each, their serial answers taken"""
    return rows + [cc.PackedWorker(env).serial(), cc.ParamsSelectWorker(env).serial(), cc.GetitemChecksumWorker(env).serial(), cc.CtxWorker(env).serial()]


def overlap_condition(seen, rounds, what, entry_points=0):
    print(what, seen)
    assert 2 * seen.rounds_with_overlap() >= rounds, (what, "calls of different threads overlapped in fewer than half of the rounds", seen)
    assert len(seen.names) >= entry_points, (what, f"fewer than {entry_points} entry points took part in an overlap", seen)


def test_every_family_side_by_side(env, families):
    """8 threads, one family each, 6 rounds: the row calls alternate between their batch and packed entry points, device-pointer calls run on
    the NULL stream in even rounds and on a stream of the thread's own in odd rounds"""
    seen = cc.run_threads(env.lib, families, 6, streams, on_stream)
    overlap_condition(seen, 6, "every family side by side:", entry_points=4)


MANY_ROWS = [12, 17, 96, 4080, 24, 48]
MANY_CHUNKS = [3, 4, 5, 4, 5, 3]


def many_tables(env, family):
    """six workers of one family, a table each: another row size, another codec, another number of chunks - no answer fits two of them"""
    if family in ("take", "put"):
        kind = cc.TakeWorker if family == "take" else cc.PutWorker
        return [kind(env, [cc.RowTable(env, cc.PUT_SETTINGS[k % 3], rb, MANY_CHUNKS[k], turn=k)]) for k, rb in enumerate(MANY_ROWS)]
    kind = cc.WhereWorker if family == "where" else cc.AggregateWorker
    return [kind(env, cc.field_tables(env, [lay], [cc.FIELD_SETTINGS[k]], [MANY_CHUNKS[k]])) for k, lay in enumerate(wh.LAYOUTS)]


@pytest.mark.parametrize("family", ["take", "put", "where", "aggregate"])
def test_one_family_many_tables(env, family):
    """6 threads in the same entry point at the same time, each on a table of its own, 6 rounds: a chunk table, a scan state or a pinned carve
    shared between two contexts cannot hide behind different kernels"""
    workers = [w.serial() for w in many_tables(env, family)]
    assert len({w.tables[0].name for w in workers}) == 6 and {len(w.tables[0].chunks) for w in workers} == {3, 4, 5}
    seen = cc.run_threads(env.lib, workers, 6, streams, on_stream)
    assert seen.names <= set(workers[0].entry_points), seen
    overlap_condition(seen, 6, f"six tables of {family}:")


def test_alternating_geometries_across_contexts(env):
    """4 threads, 10 rounds: two write and read containers of geometry A (6 chunks of 40 KiB + 24 bytes, typesize 8), two of geometry B
    (4 chunks, typesize 4).  A caller lands on whichever context is free, so every context's table cache meets both geometries in an order
    no serial test gives; every container equals the serial one and is read back by the oracle"""
    hosts = [plain(SMALL, seed=20 + k) for k in range(6)]
    a = cc.PackedWorker(env, [(6, 8, "lz4", 5, 1)], hosts=hosts).serial()
    b = cc.PackedWorker(env, [(4, 4, "lz4", 5, 1)], hosts=hosts).serial()
    seen = cc.run_threads(env.lib, [a, b, a, b], 10, streams, on_stream)
    overlap_condition(seen, 10, "alternating geometries:")


def test_more_callers_than_contexts(env, families):
    """12 threads over the eight families (the pool holds at most 8 contexts), 4 rounds: callers wait in CtxGuard with row calls in front of
    them - the four row families run twice"""
    seen = cc.run_threads(env.lib, families + families[:4], 4, streams, on_stream)
    overlap_condition(seen, 4, "twelve callers:")


def test_passes_under_concurrency(env, rows):
    """take, put, where and aggregate under a pass bound of 16 KiB, set once before the threads start: every call is several passes with their
    synchronisations.  4 threads, 4 rounds; the answers are the one-pass serial ones"""
    seen = cc.run_threads(env.lib, rows, 4, streams, on_stream, pass_bytes=PASS_BYTES)
    overlap_condition(seen, 4, "16 KiB passes:")


def test_two_contexts_only():
    """test_every_family_side_by_side once more with BLOSC_AMD_CONTEXTS=2 - the switch is read once per process, so in a process of its own"""
    if os.environ.get(CHILD) == "1":
        return
    env = dict(os.environ, BLOSC_AMD_CONTEXTS="2")
    env[CHILD] = "1"
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__) + "::test_every_family_side_by_side", "-m", "gpu", "-q", "-x", "-s", "--no-header",
                        "-p", "no:cacheprovider"], env=env, timeout=900, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and " passed" in p.stdout and "failed" not in p.stdout, (p.stdout[-3000:], p.stderr[-2000:])
