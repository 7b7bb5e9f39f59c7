"""Host logic without a GPU: the lead of a block's shuffle task over its streams in the encode queues (c-blosc_amd/csrc/queue_order.h) is
enc_lookahead() blocks - 96 since round 7, sized to the duration of a shuffle task - for every block of every XCD's queue, with and without
cost feedback.  tests/tools/enc_lookahead_check.cpp compiles the queue builder with g++ and checks it."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_shuffle_task_leads_its_streams_by_the_lookahead():
    with tempfile.TemporaryDirectory() as td:
        exe = os.path.join(td, "enc_lookahead_check")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "c-blosc_amd", "csrc"),
                               os.path.join(ROOT, "tests", "tools", "enc_lookahead_check.cpp"), "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "enc_lookahead_check OK" in out.stdout, out.stdout + out.stderr
