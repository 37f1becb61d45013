"""The device-resident LM loop enqueues the passes it enqueued when tests/golden/lm_pass_counts.json was recorded (the parent of the
commit that made the host's pass plan a value, csrc/pgo_lm_pass.hpp; tests/golden/make_lm_pass_counts.py records it).  What the host
predicts never changes a result, so no other test sees a slip in those rules: it costs passes, 50 - 100 us each.  Equality of passes,
trials, PCG iterations and LM iterations of every optimize of every case (tests/lm_pass_cases.py)."""
import json
import os

import pytest

import lm_pass_cases as LC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_pass_counts.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_the_cases():
    assert set(GOLDEN) <= set(LC.CASES) and len([k for k in GOLDEN if k[0] in "12345"]) == 6, sorted(GOLDEN)


@pytest.mark.parametrize("case", sorted(GOLDEN))
def test_pass_counts_are_the_recorded_ones(capi, case):
    got = LC.CASES[case](capi)
    print(case, got)
    assert got == GOLDEN[case]
