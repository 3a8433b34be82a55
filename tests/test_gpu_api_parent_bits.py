"""GPU: the entries of the Python layer give the bits they gave before the layer was split by family: every digest of tests/api_bits_cases.py
against tests/golden/api_parent_digests.txt, which tools/family_digest.py --cases api_bits_cases recorded through the Python layer of the
commit its first line names.  The library is the same on both sides, so a differing digest means a changed byte, argument or call order in
the layer: restore it, do not re-record."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import api_bits_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_parent_digests.txt")


@functools.lru_cache(None)
def _table():
    return B.read_table(TABLE)


def test_the_table_covers_exactly_the_cases():
    with open(TABLE) as f:
        first = f.readline()
    assert first.startswith("#") and "commit" in first, first      # the first line names the commit the layer was recorded at
    assert {e.split(" / ")[0] for e in _table()} == set(B.CASES)


@pytest.mark.parametrize("name", list(B.CASES))
def test_parent_bits(name):
    got = B.digests(name)
    want = {e: h for e, h in _table().items() if e.split(" / ")[0] == name}
    assert [e for e, _ in got] == list(want), (got, want)
    differ = [e for e, h in got if h != want[e]]
    assert not differ, differ
