"""Every field of a sweep's plan (plan_sweep through bwgr_debug_sweep_plan: host arithmetic, no GPU) for the table of sweeps in
tests/sweep_plan_cases.py.  tools/uvb_digest.py's scheme for a plan: two builds of the library that print the same table decide every sweep alike.

    python tools/sweep_plan_table.py                              # the library of this tree
    BWGR_LIB=/path/to/libbwgr_hip.so python tools/sweep_plan_table.py --out tests/golden/sweep_plan_parent.txt --commit 0123abc

Nothing outside the repository is read."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="also write the table to this file")
    ap.add_argument("--commit", default="unknown", help="the commit the library was built at: the table's first line names it")
    ap.add_argument("--quiet", action="store_true", help="print the counts only")
    a = ap.parse_args()
    import sweep_plan_cases as S
    tab = S.table()
    if not a.quiet:
        for k, v in tab.items():
            print("%s  %s" % (k, " ".join(str(x) for x in v) if v is not None else "refused"))
    print("%d cases, %d refused" % (len(tab), sum(v is None for v in tab.values())), file=sys.stderr)
    if a.out:
        S.write_table(a.out, tab, a.commit)


if __name__ == "__main__":
    main()
