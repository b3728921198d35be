"""The conv1d family (csrc/hifigan.hip, fastpitch.hip, quartznet.hip, jasper.hip and what they share through csrc/conv1d_family.h)
computes, bit for bit, what it computed when tests/golden/conv1d_family_bits.json was recorded (tools/make_conv1d_family_bits.py,
run on the commit in front of the one that introduced the header).  The float64 bars of the kernels' own suites would let a reordered
sum or a fused product pass; a digest of the output bytes does not.  The cases and why each is there: tests/_conv1d_family_cases.py.
GPU only.
"""
import json
import os

import pytest

from tests import _conv1d_family_cases as K

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv1d_family_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert set(GOLDEN) == set(K.DTYPES)
    for dn in K.DTYPES:
        assert set(GOLDEN[dn]) == set(K.CASES)
        for v in ("s1d1", "s2", "d2", "b65"):                               # both forms of the chunk loop were recorded equal
            assert GOLDEN[dn]["qn_%s_pf0" % v] == GOLDEN[dn]["qn_%s_pf1" % v]


@pytest.mark.parametrize("dn", sorted(K.DTYPES))
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_bits(name, dn):
    got = K.digests(name, K.DTYPES[dn])
    assert got == GOLDEN[dn][name]
