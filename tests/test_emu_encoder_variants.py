"""CPU: every encoder variant behind blosc_compress_ctx on the emulated library, against tests/golden/encoder_variants.json - the
return value, the chunk's bytes (sha256) and the profile name its one launch is counted under, per codec, clevel and encoder switch
(tests/encoder_variant_checks.py: CASES).  Every variant writes a valid stream, so only the bytes show that the switches still reach the
kernel they reached at the commit the file was generated at (tests/golden/README.md)."""
import json
import os

from test_emu_library import emulib  # noqa: F401  (the fixture)

import encoder_variant_checks as ev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_variants.json")


def test_every_switch_combination_writes_the_recorded_chunk(emulib):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    before = {k: os.environ.get(k) for k in ev.SWITCHES}
    got = ev.collect(emulib)
    assert {k: os.environ.get(k) for k in ev.SWITCHES} == before
    assert [c["case"] for c in got["cases"]] == [c["case"] for c in want["cases"]]
    for g, w in zip(got["cases"], want["cases"]):
        assert g == w, (g, w)
