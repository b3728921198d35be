"""The accumulator layout of the 32 x 32 x 16 MFMA lives in csrc/mfma32_rows.h only (rt_feat, rt_pack4): no other file of csrc/ spells
the register-to-feature map out or keeps a four-value pack of its own (no GPU needed)."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "deeplearningexamples_amd", "csrc")
HEADER = "mfma32_rows.h"
EIGHTS = r"8 \* \(\w+ >> 2\)"
# the map in either term order: `& 3` on the same line as `8 * (r >> 2)`
LITERAL_MAP = re.compile(r"& 3\b.*%s|%s.*& 3\b" % (EIGHTS, EIGHTS))


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert any(p.endswith(HEADER) for p in paths)
    return {os.path.basename(p): open(p).read() for p in paths}


def test_the_header_holds_the_map():
    assert LITERAL_MAP.search(_sources()[HEADER])


def test_literal_map_only_in_the_header():
    for name, src in _sources().items():
        if name == HEADER:
            continue
        for i, line in enumerate(src.splitlines(), 1):
            assert not LITERAL_MAP.search(line), "%s:%d spells the register-to-feature map out: use rt_feat (%s)" % (name, i, HEADER)


def test_no_private_pack4():
    found = {}
    for name, src in _sources().items():
        for m in re.finditer(r"\b(\w+_pack4)\s*\([^;{}]*\)\s*\{", src):      # a definition: parameter list, then a body
            found.setdefault(name, set()).add(m.group(1))
    assert found == {HEADER: {"rt_pack4"}}, "a *_pack4 is defined outside %s: %s (use rt_pack4)" % (HEADER, found)
