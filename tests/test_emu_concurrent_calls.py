"""CPU: the workers and the runner of tests/concurrent_checks.py on the emulated library - take, put, where and aggregate from four threads.
The emulator has one context (engine.hip: ctx_count() is 1 under BAMD_WAVE_EMU), so every call queues on the same mutex: what runs here is
the workers' own bookkeeping - expectation, serial answer, byte equality - and the waiting path of CtxGuard under the row calls.  Two contexts
in use at once is what tests/test_gpu_concurrent_calls.py is for."""
import importlib.util
import os

import pytest

import concurrent_checks as cc
import where_checks as wh
from getitem_ranges_checks import NumpyMem
from test_emu_library import emulib  # noqa: F401  (the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THREADS, ROUNDS = 4, 2
LIGHT = ("blosclz", 17, 2)      # typesize 17: blocks of 8177 bytes at N bytes a chunk - what the emulator encodes in a second


@pytest.fixture(scope="module")
def env(emulib, oracle, ref):
    spec = importlib.util.spec_from_file_location("c_blosc_amd_for_emu_concurrent", os.path.join(ROOT, "c-blosc_amd", "__init__.py"))
    pkgmod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pkgmod)
    assert hasattr(emulib, "blosc_gpu_aggregate_batch"), "the library has no row calls"
    made = cc.Env(pkgmod, cc.Recorder(emulib), NumpyMem(), oracle, ref)
    yield made
    made.close()      # (the global split mode, as it was found)


@pytest.fixture(scope="module")
def workers(env):
    """the four row families on small tables, their serial answers taken"""
    rows = lambda rb, turn: [cc.RowTable(env, LIGHT, rb, turn=turn, random_rows=200)]
    fields = cc.field_tables(env, [wh.LAYOUTS[0]], [("blosclz", 17, 1, 1)]) + cc.field_tables(env, [wh.LAYOUTS[2]], [("lz4", 17, 2, 1)])
    made = [cc.TakeWorker(env, rows(17, 0) + rows(96, 1)), cc.PutWorker(env, rows(12, 2)), cc.WhereWorker(env, fields, ops=(0, 3, 4)),
            cc.AggregateWorker(env, fields)]
    return [w.serial() for w in made]


def test_row_calls_queue_on_the_one_context(env, workers):
    """4 threads, 2 rounds, every repetition checked in full and byte for byte against its serial call.  A caller's logged interval begins
    when it enters the library, so it holds the time spent waiting for the context as well: intervals of different threads do overlap here,
    and each such pair is a caller that went through CtxGuard's waiting path.  That no two calls held the context at once is not visible
    from outside the library; what is asserted is that every thread made its calls and that calls did wait on each other."""
    assert len(workers) == THREADS
    start = len(env.lib.log)
    seen = cc.run_threads(env.lib, workers, ROUNDS)
    print("emulator:", seen)
    log = env.lib.log[start:]
    for w, t in zip(workers, range(THREADS)):
        mine = {name for who, name, _, _ in log if who.startswith(f"t{t}-")}
        assert mine and mine <= set(w.entry_points), (t, mine)
    assert seen.pairs > 0, ("no caller ever waited for the context", seen)


def test_a_moved_serial_answer_is_noticed(env, workers):
    """the byte-equality bookkeeping has teeth: with another table's serial answer in its place, a repetition fails and names the thread,
    the case and the first differing byte"""
    take = workers[0]
    case_a, case_b = take.cases()[0], take.cases()[2]
    assert case_a[0] != case_b[0] and case_a[1] == "batch"
    kept = take.first[case_a]
    one_byte = dict(kept, status=kept["status"].copy())
    one_byte["status"].view("u1")[41] ^= 1
    for moved, where in ((take.first[case_b], "bytes for"), (one_byte, "first at byte 41")):
        take.first[case_a] = moved
        try:
            with pytest.raises(AssertionError) as failure:
                take.repeat(case_a, None, "t0")
        finally:
            take.first[case_a] = kept
        said = str(failure.value)
        assert "t0" in said and "blosc_gpu_take_batch" in said and "differs from the serial call" in said and where in said, said
    take.repeat(case_a, None, "t0")
