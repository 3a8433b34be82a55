"""GPU: the float samplers and every path of a sweep's planning and launching -- pairs, clones, block ranges, k_sweep3f, the fp64 redo, the
engine switches -- give the bits they gave before plan_sweep took a mode and carried its redo, the launch train was written once and
bwgr_hip.hip was split by role: every digest of tests/sampler_bits_cases.py against tests/golden/sampler_parent_digests.txt, which
tools/family_digest.py recorded from the library built at the commit its first line names.  A differing digest means a changed launch, launch
order or argument: restore it, do not re-record."""
import functools
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_bits_cases as B  # noqa: E402

pytestmark = pytest.mark.gpu
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sampler_parent_digests.txt")


@functools.lru_cache(None)
def _table():
    return B.read_table(TABLE)


def test_the_table_covers_exactly_the_cases():
    with open(TABLE) as f:
        first = f.readline()
    assert first.startswith("#") and "commit" in first, first      # the first line names the commit the library was built at
    assert {e.split(" / ")[0] for e in _table()} == set(B.CASES)


def test_a_paired_chain_is_the_chain_alone_in_the_table_itself():
    t = _table()
    pairs = [e for e in t if e.startswith("pair ") and " / pair " in e]
    assert len(pairs) >= 2 * 2 * 8
    for e in pairs:
        assert t[e] == t[e.replace(" / pair ", " / alone ")], e


@pytest.mark.parametrize("name", list(B.CASES))
def test_parent_bits(name):
    got = B.digests(name)
    want = {e: h for e, h in _table().items() if e.split(" / ")[0] == name}
    assert [e for e, _ in got] == list(want), (got, want)
    differ = [e for e, h in got if h != want[e]]
    assert not differ, differ
