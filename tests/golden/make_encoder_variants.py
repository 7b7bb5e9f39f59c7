"""Writes tests/golden/encoder_variants.json: what blosc_compress_ctx answers under every combination of codec, clevel and encoder switch
of tests/encoder_variant_checks.py on the emulated library (tests/tools/libblosc_amd_emu.so, built by __graft_entry__.build() or by the
first test_emu_* run) - return value, sha256 of the chunk, launches per profile name.  The file pins the answers of ONE commit
(tests/golden/README.md names it): regenerate it only when an encoder's bytes are meant to change.
    python tests/golden/make_encoder_variants.py"""
import ctypes as C
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import encoder_variant_checks as ev  # noqa: E402

GOLDEN = os.path.join(HERE, "encoder_variants.json")

L = C.CDLL(os.environ.get("BLOSC_EMU_LIB", os.path.join(HERE, "..", "tools", "libblosc_amd_emu.so")))
answers = ev.collect(L)
cases = answers["cases"]
# what makes the file a check of the launch: all eleven modes are there, and two cases of different modes never wrote the same bytes for
# both inputs - the chunk of a wrong mode's kernel is not the recorded one
assert {c["mode"] for c in cases} == set(ev.MODES)
for a, b in itertools.combinations(cases, 2):
    if a["mode"] != b["mode"]:
        assert [r["sha256"] for r in a["runs"]] != [r["sha256"] for r in b["runs"]], (a["case"], b["case"])
for c in cases:
    for r in c["runs"]:
        assert r["ret"] > 0 and sum(r["launches"].values()) == 1 and r["launches"][ev.profile_name(c["mode"])] == 1, (c["case"], r)
with open(GOLDEN, "w") as fh:
    json.dump(answers, fh, indent=1)
    fh.write("\n")
print(f"{len(cases)} cases -> {GOLDEN}")
for c in cases:
    print(f"  {c['case']:48s} {c['mode']:16s} " + " ".join(f"{r['ret']:6d}" for r in c["runs"]))
