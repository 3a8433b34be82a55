"""Writes the tables that hold the Python layer's surface and refusals (tests/test_api_surface_cpu.py, tests/test_api_refusals_cpu.py,
tests/test_gpu_api_refusals.py) from the layer of this tree:

    python tools/api_golden.py surface --out tests/golden/api_surface_parent.txt --commit 0123abc
    python tools/api_golden.py refusals --tags host --out host.txt --commit 0123abc          # needs no GPU
    python tools/api_golden.py refusals --tags device --out device.txt --commit 0123abc      # on the GPU

The refusal table is the two parts one after the other under one first line.  Nothing outside the repository is read."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=("surface", "refusals"))
    ap.add_argument("--tags", default="host,device")
    ap.add_argument("--out", required=True)
    ap.add_argument("--commit", default="unknown", help="the commit of the layer: the table's first line names it")
    a = ap.parse_args()
    if a.what == "surface":
        from test_api_surface_cpu import surface
        head, lines = "signature and sha256 of the docstring of bwgr_amd's public names, repr of its constants", surface()
    else:
        import api_refusal_cases as R
        head = "the refusals of tests/api_refusal_cases.py (tag  id  outcome; the device rows recorded on an MI355X)"
        lines = ["%s  %s  %s" % (tag, id_, R.outcome(id_)) for id_, (tag, _) in R.CASES.items() if tag in a.tags.split(",")]
    with open(a.out, "w") as f:
        f.write("# %s, recorded with tools/api_golden.py from the Python layer at commit %s\n" % (head, a.commit))
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
