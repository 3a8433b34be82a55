"""GPU: the per-trait fits, panel_xb and the relationship kernels give the bits they gave before their host entries were split by family and
bwgr_uvbeta / bwgr_uvbeta2 moved onto the UvFit context: every digest of tests/uvb_bits_cases.py against tests/golden/uvb_parent_digests.txt,
which tools/uvb_digest.py recorded from the library built at the commit its first line names.  A differing digest of a host-computed scalar
(mu, ve, vb, cnv) means reordered host arithmetic or a changed contraction in bwgr_amd/csrc/uvb_tail.h: restore the expression, do not
re-record."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import uvb_bits_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uvb_parent_digests.txt")


@functools.lru_cache(None)
def _table():
    return B.read_table(TABLE)


def test_the_table_covers_exactly_the_cases():
    with open(TABLE) as f:
        first = f.readline()
    assert first.startswith("#") and "commit" in first, first      # the first line names the commit the library was built at
    assert {e.split(" / ")[0] for e in _table()} == set(B.CASES)


@pytest.mark.parametrize("name", list(B.CASES))
def test_parent_bits(name):
    got = B.digests(name)
    want = {e: h for e, h in _table().items() if e.split(" / ")[0] == name}
    assert [e for e, _ in got] == list(want), (got, want)
    differ = [e for e, h in got if h != want[e]]
    assert not differ, differ
