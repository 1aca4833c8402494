"""A scale word travels with its tensor (``ops.Scaled``) instead of beside it.  That moved every h2 word of the Python
layer and must have moved nothing else: each case of tests/step_parity_cases.py -- one train forward and backward per
head and product mode, a frozen step and an eval forward -- makes the launches the build BEFORE the change made, in
the same order with the same ``products`` and ``act16``, and leaves the same bits in the outputs, the gradient buffer
and the BatchNorm running statistics.  tests/golden/make_step_parity_golden.py recorded both on an MI355X with that
build (tests/golden/step_parity_parent.json)."""
import json
from pathlib import Path

import pytest

from tests import step_parity_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "step_parity_parent.json").read_text())


@pytest.fixture(scope="module")
def got(hip_device):
    """Every case once, as the golden file holds it (through JSON: tuples become lists)."""
    return json.loads(json.dumps(cases.run_cases(hip_device)))


def test_the_cases_are_the_recorded_ones():
    assert sorted(cases.CASES) == sorted(GOLDEN) and len(GOLDEN) == 22


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_launches_and_bits_are_the_parent_builds(got, name):
    g, want = got[name], GOLDEN[name]
    print(name, sum(g["counts"].values()), "launches", {k: v[:12] for k, v in g.items() if isinstance(v, str)})
    assert g["counts"] == want["counts"]
    assert g["calls"] == want["calls"]
    assert {k: v for k, v in g.items() if isinstance(v, str)} == {k: v for k, v in want.items() if isinstance(v, str)}
