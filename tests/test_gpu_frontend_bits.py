"""Every inference front end still sends the library what it sent when tests/golden/frontend_bits.json was recorded
(tools/make_frontend_bits.py, on an MI355X): one call per case of tests/_frontend_cases.py, the SHA-256 of the output bytes
equal to the recorded one.  A captured run (graphs=True, third call: the first replay) must give its eager case's digest.
GPU only.  The comparison is exact on purpose: the kernels on these paths have no atomics and no run-dependent order."""
import json
import os

import pytest

from tests import _frontend_cases as FC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_bits.json")) as f:
    GOLDEN = json.load(f)


def test_every_case_is_recorded():
    assert sorted(GOLDEN) == sorted(FC.CASES)


@pytest.mark.parametrize("name,graphs", FC.RUNS, ids=["%s-%s" % (k, "graphs" if g else "eager") for k, g in FC.RUNS])
def test_output_bits_are_the_recorded_ones(name, graphs):
    got = FC.digest(FC.CASES[name][0](graphs))
    print(name, graphs, got)
    assert got == GOLDEN[name]
