"""Writes tests/golden/abi_arguments.json: what tests/test_abi_arguments.py's calls answer on the emulated library
(tests/tools/libblosc_amd_emu.so, built by __graft_entry__.build() or by the first test_emu_* run).  The file pins the answers of ONE commit
(tests/golden/README.md names it) so that later changes of the ABI glue can be compared with it: regenerate it only when an answer is
meant to change.     python tests/golden/make_abi_arguments.py"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_abi_arguments import GOLDEN, collect_all  # noqa: E402

L = C.CDLL(os.environ.get("BLOSC_EMU_LIB", os.path.join(HERE, "..", "tools", "libblosc_amd_emu.so")))
answers = collect_all(L)
with open(GOLDEN, "w") as fh:
    json.dump(answers, fh, indent=1)
    fh.write("\n")
print(f"{len(answers['calls'])} calls, {len(answers['blpk'])} files -> {GOLDEN}")
