"""The row-tile family (csrc/tft.hip, ncf.hip, moflow.hip and what they share through csrc/mfma32_rows.h) and the kernels that take
only the index map from that header (transformer_xl.hip, dot_interact.hip, attention.hip) compute, bit for bit, what they computed
when tests/golden/rowtile_family_bits.json was recorded (tools/make_rowtile_family_bits.py, run on the commit in front of the one
that introduced the header).  The float64 bars of the kernels' own suites would let a reordered sum or a fused product pass; a
digest of the output bytes does not.  The cases and why each is there: tests/_rowtile_family_cases.py.  GPU only.
"""
import json
import os

import pytest

from tests import _rowtile_family_cases as K

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rowtile_family_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert set(GOLDEN) == set(K.DTYPES)
    for dn in K.DTYPES:
        assert set(GOLDEN[dn]) == set(K.CASES)
        assert GOLDEN[dn]["atom_wg1"] == GOLDEN[dn]["atom_wg0"]              # one workgroup over both tiles, or one per tile
        assert all(len(d) == 64 for v in GOLDEN[dn].values() for d in v.values())


@pytest.mark.parametrize("dn", sorted(K.DTYPES))
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_bits(name, dn):
    got = K.digests(name, K.DTYPES[dn])
    assert got == GOLDEN[dn][name]
