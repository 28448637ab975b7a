"""The parameter-side kernels (csrc/pack.hip, rows.hip, optim.hip, stats.hip) against the bytes of the one file they were split from:
every case of tests/optim_forms.py, one sha256 over all of its output buffers, compared with tests/golden/optim_forms_sha256.json --
recorded by tools/optim_equivalence.py from the library of the commit BEFORE the split, never from the code under test.  These results
are documented as bit-reproducible (fixed-order sums, IEEE arithmetic without contraction), so a differing digest is a changed
operation order or a changed rounding, not noise."""
import json
import os

import pytest

import optim_forms as F
from hip_pass import L  # noqa: F401

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "optim_forms_sha256.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["sha256"]


def test_every_case_has_a_recorded_digest(golden):
    assert sorted(golden) == F.case_ids()


@pytest.mark.parametrize("case", F.case_ids())
def test_same_bytes_as_before_the_split(L, golden, case):
    assert F.run_case(L, case) == golden[case], case
