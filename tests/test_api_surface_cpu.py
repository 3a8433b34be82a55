"""CPU: the package's public surface is what tests/golden/api_surface_parent.txt recorded before the Python layer was split by family
(tools/api_golden.py surface): for every name of bwgr_amd.__all__ and every public method of Panel, Chain, Group, dense and sparse the
signature and the SHA-256 of the docstring, for every constant its repr.  Importing the package must not import torch."""
import hashlib
import inspect
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "api_surface_parent.txt")
CLASSES = ("Panel", "Chain", "Group", "dense", "sparse")
CONSTANTS = ("MRR_KEYS", "PEGS_KEYS", "PEGSX_KEYS", "UVB_KEYS", "UVB2_KEYS", "UVB_VARIANTS", "KERNELS", "KERNELS2", "SWEEP_PLAN_FIELDS", "MODELS",
             "X_I8", "X_F32", "X_F64", "HOST", "DEVICE")     # reached as bwgr_amd.api.NAME


def _doc(obj):
    d = getattr(obj, "__doc__", None)
    return "none" if d is None else hashlib.sha256(d.encode()).hexdigest()


def _callable_line(name, obj):
    return "%s  %s  doc %s" % (name, inspect.signature(obj), _doc(obj))


def surface():
    """the table's lines, without its first"""
    import bwgr_amd
    from bwgr_amd import api
    lines = ["__all__  %s" % " ".join(sorted(bwgr_amd.__all__)), "bwgr_amd  doc %s" % _doc(bwgr_amd), "bwgr_amd.api  doc %s" % _doc(api)]
    for name in sorted(bwgr_amd.__all__):
        obj = getattr(bwgr_amd, name)
        lines.append(_callable_line(name, obj) if callable(obj) else "%s  = %r" % (name, obj))
    for cls in CLASSES:
        for name, member in sorted(vars(getattr(bwgr_amd, cls)).items()):
            if name.startswith("_"):
                continue
            if isinstance(member, property):
                lines.append("%s.%s  property  doc %s" % (cls, name, _doc(member)))
            else:
                lines.append(_callable_line("%s.%s" % (cls, name), member))
    for name in CONSTANTS:
        lines.append("api.%s  = %r" % (name, getattr(api, name)))
    return lines


def test_surface_is_the_parents():
    with open(TABLE) as f:
        first, want = f.readline(), f.read().splitlines()
    assert first.startswith("#") and "commit" in first, first
    got = surface()
    assert [l.split("  ")[0] for l in got] == [l.split("  ")[0] for l in want]
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w]


def test_importing_the_package_does_not_import_torch():
    code = "import sys; sys.path.insert(0, %r); import bwgr_amd, bwgr_amd.api; sys.exit(1 if 'torch' in sys.modules else 0)" % ROOT
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0
