"""CPU: the ABI table of bwgr_amd/_lib.py against the prototypes of include/bwgr.h -- the same names, every argtypes list as long as its
prototype, every scalar parameter bound to its ctypes type and every pointer parameter to a pointer type.  A wrong entry on a call such as
bwgr_pegsx (29 arguments) would corrupt memory silently.  The table is read, not the loaded library: nothing here needs the build."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}


def _split_top(s):
    """s split at the commas that lie outside every bracket"""
    out, depth, cur = [], 0, ""
    for ch in s:
        depth += ch in "(["
        depth -= ch in ")]"
        if ch == "," and depth == 0:
            out.append(cur); cur = ""
        else:
            cur += ch
    return [p.strip() for p in out + [cur] if p.strip()]


def prototypes():
    """{name: (return type, [parameter kind])} of the header; a kind is a scalar's type name or "pointer" (`T *x`, `T x[N]`)"""
    src = open(os.path.join(ROOT, "include", "bwgr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("#"))
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(bwgr_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", src):
        kinds = []
        for p in _split_top(params):
            if p == "void":
                continue
            if "*" in p or "[" in p:
                kinds.append("pointer")
            else:
                kinds.append(" ".join(t for t in p.split()[:-1] if t != "const"))
        assert name not in out, name
        out[name] = (" ".join(ret.split()), kinds)
    return out


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def test_the_parser_reads_the_header():
    protos = prototypes()
    assert protos["bwgr_abi_version"] == ("int", []) and protos["bwgr_last_error"] == ("const char *", [])
    assert protos["bwgr_debug_live"] == ("int", ["pointer"])                                     # int64_t out[3]
    assert protos["bwgr_em_order"] == ("int", ["int64_t", "int", "pointer"])
    assert len(protos["bwgr_pegsx"][1]) == 29
    assert {k for _, kinds in protos.values() for k in kinds} <= set(SCALARS) | {"pointer"}


def test_names_are_the_headers():
    from bwgr_amd import _lib
    assert set(prototypes()) == set(_lib.ABI) == set(_lib.EXPORTS)
    assert len(_lib.EXPORTS) == len(set(_lib.EXPORTS)) == len(_lib.ABI)


def test_argtypes_match_the_prototypes():
    from bwgr_amd import _lib
    wrong = []
    for name, (ret, kinds) in prototypes().items():
        argtypes = _lib.ABI[name]
        if len(argtypes) != len(kinds):
            wrong.append((name, "has %d argtypes, the prototype %d parameters" % (len(argtypes), len(kinds))))
            continue
        for i, (t, kind) in enumerate(zip(argtypes, kinds)):
            if not (_is_pointer(t) if kind == "pointer" else t is SCALARS[kind]):
                wrong.append((name, i, kind, t))
        want = C.c_int if ret == "int" else C.c_char_p if ret == "const char *" else None
        if _lib.RESTYPE.get(name, C.c_int) is not want:
            wrong.append((name, "returns", ret))
    assert not wrong, wrong
