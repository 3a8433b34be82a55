"""One SHA-256 per output array of the float samplers and of every path of a sweep's planning and launching, for the table of calls in
tests/sampler_bits_cases.py.  These families draw from a counter-based generator and reduce in a fixed order, so equal inputs give equal
bits: two builds of the library that print the same table compute the same thing.

    python tools/family_digest.py                              # the library of this tree
    python tools/family_digest.py --cases api_bits_cases --out tests/golden/api_parent_digests.txt --commit 0123abc
    BWGR_LIB=/path/to/libbwgr_hip.so python tools/family_digest.py --out table.txt --commit 0123abc

Every case runs twice; a table is written only if the two runs agree entry by entry.  Nothing outside the repository is read."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--cases", default="sampler_bits_cases", help="the module under tests/ that holds CASES and digests() (default: %(default)s)")
    ap.add_argument("--out", help="also write the table to this file")
    ap.add_argument("--commit", default="unknown", help="the commit the library was built at: the table's first line names it")
    a = ap.parse_args()
    import importlib
    B = importlib.import_module(a.cases)
    lines, differ = [], []
    for name in B.CASES:
        first, second = B.digests(name), B.digests(name)
        for (entry, h1), (_, h2) in zip(first, second):
            lines.append("%s  %s" % (h1, entry))
            print(lines[-1], flush=True)
            if h1 != h2:
                differ.append(entry)
    if differ:
        sys.exit("two runs of the same call differ, no table written: " + "; ".join(differ))
    if a.out:
        with open(a.out, "w") as f:
            f.write("# sha256 of every output array of tests/%s.py, recorded on an MI355X with tools/family_digest.py from the library built at commit %s\n" % (a.cases, a.commit))
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
