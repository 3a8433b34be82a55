"""The float64 fits of the three PEGS restatements on every case of tests/pegsx_cases.py, tests/pegs_cases.py and tests/pegs_sparse_cases.py,
flattened to fields: path -> array, one per array or scalar anywhere in a fit's dict (lists, tuples and nested dicts by index and key, a set
as its sorted names, None as an empty array); and the bounds of tests/mt_tight.py on its first 49 cases.  tests/test_mt_tight_cpu.py holds both
to the commit PARENT, the last one before the restatements learnt long double: field by field with np.array_equal against that commit's
files, which it reads from git into a temporary directory and runs there; where the tree is no git checkout that has the commit, against
tests/golden/mt_tight_parent_bits.json, recorded from them.

Run as a program beside a commit's tests (python restatement_fields.py OUT.pkl) it writes that commit's fields and bounds; with --record
OUT.json their digests, with a probe: the digest of a few products, an eigen-decomposition and a solve in numpy.  BLAS libraries choose their
kernels by the processor, and another summation order is other last bits: the recorded digests say something only on a machine that gives the
probe's bits."""
import hashlib
import json
import os
import pickle
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PARENT = "2fa350f6899eeb142d2873152c7172f9106a8c99"
RECORDED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt_tight_parent_bits.json")
N_OLD = 49


def flatten(obj, path="", out=None):
    out = {} if out is None else out
    if isinstance(obj, dict):
        for key in sorted(obj, key=str):
            flatten(obj[key], "%s/%s" % (path, key), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            flatten(v, "%s/%d" % (path, i), out)
    elif isinstance(obj, (set, frozenset)):
        out[path] = np.array(sorted(obj), dtype="U16")
    elif obj is None:
        out[path] = np.zeros(0)
    else:
        out[path] = np.asarray(obj)
        assert out[path].dtype != object, path
    return out


def all_fields():
    """"<cases module>/<case id>/<path>" -> array, for every case of the three tables"""
    import pegs_cases as PC
    import pegs_sparse_cases as SC
    import pegsx_cases as XC
    out = {}
    for c in XC.CASES:
        flatten(XC.restate(c)[3], "pegsx_cases/" + c["id"], out)
    for c in PC.CASES:
        flatten(PC.restate(c)[2], "pegs_cases/" + c["id"], out)
    for c in SC.CASES:
        flatten(SC.restate(c)[1], "pegs_sparse_cases/" + c["id"], out)
    return out


def old_bounds():
    """case -> key -> the bound as a hexadecimal float, for mt_tight's first 49 cases"""
    import mt_tight as T
    import mt_tight_cases as TC
    return {name: {key: float(v).hex() for key, v in T.bound(name).items()} for name in TC.NAMES[:N_OLD]}


def _sha(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def digests(fields):
    """"<cases module>/<case id>" -> (number of fields, their digest: names, dtypes, shapes and bytes)"""
    cases = {}
    for path in sorted(fields):
        cases.setdefault("/".join(path.split("/")[:2]), []).append(path)
    return {case: [len(paths), _sha([np.array(paths)] + [fields[p] for p in paths])] for case, paths in cases.items()}


def probe():
    rng = np.random.default_rng(2025)
    A, B, v = rng.normal(size=(700, 132)), rng.normal(size=(700, 5)), rng.normal(size=700)
    S = A[:, :70].T @ A[:, :70]
    return _sha([A.T @ B, A.T @ v, (A ** 2).sum(0), S, np.linalg.eigh(S)[0], np.linalg.solve(S[:16, :16], B[:16]), np.linalg.pinv(S[:5, :5])])


if __name__ == "__main__":
    if sys.argv[1] == "--record":
        with open(sys.argv[2], "w") as fh:
            json.dump(dict(commit=PARENT, probe=probe(), fields=digests(all_fields()), bounds=old_bounds()), fh, indent=0, sort_keys=True)
    else:
        with open(sys.argv[1], "wb") as fh:
            pickle.dump(dict(fields=all_fields(), bounds=old_bounds()), fh)
