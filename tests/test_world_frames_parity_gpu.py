"""CheapTrick and D4C take their frame plan, DC correction and interval mean from one place (csrc/world_frames.h), and
``resynthesize_ragged(ap="d4c")`` lays the rows out once for both.  What holds the outputs where they were: the bits the
two analyses and the resynthesis left BEFORE they shared any of it, recorded on an MI355X with the parent build by
tests/golden/make_world_frames_parent_golden.py as digests (tests/golden/world_frames_parent_bits.json), on the cases of
tests/world_frames_cases.py.  Equality is the condition: no tolerance, no case left out."""
import json
from pathlib import Path

import pytest

from tests import world_frames_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "world_frames_parent_bits.json").read_text())


@pytest.fixture(scope="module")
def got(hip_device):
    """Every case once: {case: {row: {what: digest}}}."""
    return cases.run_cases(hip_device)


def test_the_cases_are_the_recorded_ones(got):
    assert sorted(got) == sorted(GOLDEN) == cases.CASES
    for name in cases.CASES:
        assert sorted(got[name]) == sorted(GOLDEN[name]), name
        if not name.startswith("resynthesize"):
            assert sorted(got[name]) == sorted(cases.ROWS), name


@pytest.mark.parametrize("name", cases.CASES)
def test_the_bits_are_the_parent_builds(got, name):
    differ = [(row, what) for row, d in GOLDEN[name].items() for what in d if got[name][row][what] != d[what]]
    print(name, "rows that differ:", differ)
    assert got[name] == GOLDEN[name]
