"""CPU: the refusals the Python layer makes before it touches the device are those tests/golden/api_refusals_parent.txt recorded before the
layer was split by family (tools/api_golden.py refusals): exception class and message of every `host` case of tests/api_refusal_cases.py.
The `device` rows are held by tests/test_gpu_api_refusals.py."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import api_refusal_cases as R  # noqa: E402

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_refusals_parent.txt")
TAG = "host"


@functools.lru_cache(None)
def table():
    return R.read_table(TABLE)


def test_the_table_covers_exactly_the_cases():
    with open(TABLE) as f:
        first = f.readline()
    assert first.startswith("#") and "commit" in first, first
    assert {i: t for i, (t, _) in table().items()} == {i: t for i, (t, _) in R.CASES.items()}
    assert all(what != "no refusal" for _, what in table().values())


@pytest.mark.parametrize("id_", [i for i, (t, _) in R.CASES.items() if t == TAG])
def test_refusal(id_):
    assert R.outcome(id_) == table()[id_][1]
