"""GPU: the refusals the Python layer makes once a panel exists -- row counts of Y, Z, B and the effects against the panel's, vector lengths,
unknown job keys -- are those tests/golden/api_refusals_parent.txt recorded on an MI355X before the layer was split by family: exception
class and message of every `device` case of tests/api_refusal_cases.py (16 x 8 int8 panels).  No case reaches a kernel."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import api_refusal_cases as R  # noqa: E402
from test_api_refusals_cpu import table  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("id_", [i for i, (t, _) in R.CASES.items() if t == "device"])
def test_refusal(id_):
    assert R.outcome(id_) == table()[id_][1]
