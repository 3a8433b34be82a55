"""Every refusal the Python layer makes by itself, as tests/golden/api_refusals_parent.txt records it (exception class and message):
tests/test_api_refusals_cpu.py holds the `host` rows, tests/test_gpu_api_refusals.py the `device` rows.

A case is `host` when its path ends before Panel(...) creates a panel and before any library entry that needs the device, so that it
behaves alike with and without a GPU; `device` cases are the checks made once a panel exists (16 x 8 int8 panels).

CASES maps an id to (tag, function); outcome(id) runs the function and returns "Class: 'message'" of what it raised."""
import ctypes as C

import numpy as np

X16 = (np.arange(16 * 8).reshape(16, 8) % 3).astype(np.int8)
Y16 = np.linspace(-1.0, 1.0, 32).reshape(16, 2)
Y15 = Y16[:15]


def _bw():
    import bwgr_amd
    return bwgr_amd


def _uv():
    from bwgr_amd import uvfit as M
    return M


def _mt():
    from bwgr_amd import mtfit as M
    return M


class _FloatTensor:
    """what the layer takes for a device tensor of floats, without torch"""
    dtype = "torch.float32"
    shape = (8, 16)

    def data_ptr(self):
        return 0


def _staged():
    P = _bw().Panel.__new__(_bw().Panel)      # a panel handle that was never created: the check comes before its first use
    P._h = C.c_void_p()
    return P


def _nan_y():
    y = np.ones(16); y[3] = np.nan
    return y


_K3 = np.arange(9.0).reshape(3, 3)
_KINF = np.eye(3); _KINF[1, 1] = np.inf
_EIG = {"values": np.ones(16), "vectors": np.eye(16)}

CASES = {
    # ---- before a panel exists ----
    "dense rank 3": ("host", lambda: _bw().dense(np.zeros((2, 2, 2)))),
    "sparse rank 3": ("host", lambda: _bw().sparse(np.zeros((2, 2, 2)))),
    "sparse csc without shape": ("host", lambda: _bw().sparse((np.ones(1), np.zeros(1), np.array([0, 1])))),
    "sparse arrays disagree": ("host", lambda: _bw().sparse((np.ones(2), np.zeros(1), np.array([0, 1])), shape=(4, 1))),
    "sparse index beyond 32 bits": ("host", lambda: _bw().sparse((np.ones(1), np.array([2 ** 31]), np.array([0, 1])), shape=(4, 1))),
    "K2X not square": ("host", lambda: _bw().K2X(np.zeros((3, 2)))),
    "K2X asymmetric": ("host", lambda: _bw().K2X(_K3)),
    "K2X not finite": ("host", lambda: _bw().K2X(_KINF)),
    "mrr dense panel keyword": ("host", lambda: _bw().mrr(Y16, _bw().dense(X16), nwg=3)),
    "mrr dense nrow(Y)": ("host", lambda: _bw().mrr(Y15, _bw().dense(X16))),
    "uvbeta unknown variant": ("host", lambda: _bw().uvbeta(Y16, X16, "Q")),
    "uvbeta_dense unknown variant": ("host", lambda: _bw().uvbeta_dense(Y16, X16, "Q")),
    "uvbeta_dense rank 3": ("host", lambda: _bw().uvbeta_dense(Y16, np.zeros((16, 2, 2)))),
    "uvbeta_dense nrow(Y)": ("host", lambda: _bw().uvbeta_dense(Y15, X16.astype(float))),
    "wgr bag with eigK": ("host", lambda: _bw().wgr(np.ones(16), X16, bag=0.8, eigK=_EIG)),
    "wgr missing y staged X": ("host", lambda: _bw().wgr(_nan_y(), _staged())),
    "kernel float tensor": ("host", lambda: _bw().GRM(_FloatTensor())),
    "kernel non-integer": ("host", lambda: _bw().GAU(X16 + 0.5)),
    "kernel out of range": ("host", lambda: _bw().crossprod(X16.astype(np.int32) + 200)),
    "kernel not finite": ("host", lambda: _bw().EigenGRM(np.where(X16 == 2, np.nan, 1.0))),
    "crossprod2 column mismatch": ("host", lambda: _bw().crossprod2(X16, X16[:, :7])),
    "EigenArcZ column mismatch": ("host", lambda: _bw().EigenArcZ(X16, X16[:, :7])),
    "Panel as_int8 non-integer": ("host", lambda: _bw().Panel(X16 + 0.5, as_int8=True)),
    "Panel as_int8 out of range": ("host", lambda: _bw().Panel(X16.astype(np.int32) + 200, as_int8=True)),
    "sem npc too large": ("host", lambda: _uv()._sem_npc(4, 3, "XSEMF")),
    "sem latent npc too large": ("host", lambda: _uv()._sem_latent(Y16, 3, "GSEM")),
    "pegs effect rank 3": ("host", lambda: _mt()._pegs_effect(np.zeros((2, 2, 2)), {})),
    "pegs no effects": ("host", lambda: _bw().PEGSZ(Y16, [])),
    "pegs dense effects rows": ("host", lambda: _bw().PEGSZ(Y16, [_bw().dense(np.ones((16, 2))), _bw().dense(np.ones((15, 2)))])),
    "pegsx not matrices": ("host", lambda: _bw().PEGSX(np.zeros((2, 2, 2)), np.ones((16, 1)), [])),
    "pegsx nrow(X) no effects": ("host", lambda: _bw().PEGSX(Y16, np.ones((15, 1)), [])),
    # ---- once a panel exists ----
    "mrr nrow(Y)": ("device", lambda: _bw().mrr(Y15, X16)),
    "uvbeta nrow(Y)": ("device", lambda: _bw().uvbeta(Y15, X16)),
    "uvbeta2 nrow(Y)": ("device", lambda: _bw().uvbeta2(Y15, np.ones((16, 1)), X16)),
    "uvbeta2 nrow(Z)": ("device", lambda: _bw().uvbeta2(Y16, np.ones((15, 1)), X16)),
    "pegs effects rows": ("device", lambda: _bw().PEGSZ(Y16, [X16, _bw().dense(np.ones((15, 2)))])),
    "pegs nrow(Y)": ("device", lambda: _bw().PEGS(Y15, X16)),
    "pegsx nrow(X)": ("device", lambda: _bw().PEGSX(Y16, np.ones((15, 1)), [X16])),
    "pegsx effects rows": ("device", lambda: _bw().PEGSX(Y15, np.ones((15, 1)), [X16])),
    "panel_xb nrow(B)": ("device", lambda: _bw().panel_xb(X16, np.ones((7, 2)))),
    "KMUP length": ("device", lambda: _bw().KMUP(X16, np.zeros(7), np.ones(8), np.ones(8), np.zeros(16), np.ones(8), 1.0, 0.5, seed=1)),
    "KMUP2 length": ("device", lambda: _bw().KMUP2(X16, [0, 1, 2], np.zeros(8), np.ones(8), np.ones(8), np.zeros(15), np.ones(8), 1.0, 0.5, seed=1)),
    "em length(y)": ("device", lambda: _bw().emRR(np.ones(15), X16)),
    "em length(D)": ("device", lambda: _bw().emML(np.ones(16), X16, D=np.ones(7))),
    "fused2 rows": ("device", lambda: _bw().BayesRR2(np.ones(16), X16, X16[:15], it=2, bi=0, seed=1)),
    "fused2 length(y)": ("device", lambda: _bw().BayesA2(np.ones(15), X16, X16, it=2, bi=0, seed=1)),
    "Chain length(y)": ("device", lambda: _bw().BayesB(np.ones(15), X16, it=2, bi=0, seed=1)),
    "wgr length(y)": ("device", lambda: _bw().wgr(np.ones(15), X16, it=2, bi=0, seed=1)),
    "fit_many unknown key": ("device", lambda: _bw().fit_many(X16, [dict(model="BayesB", y=np.ones(16), iters=3)])),
    "XSEMF npc": ("device", lambda: _bw().XSEMF(Y16, X16, npc=3)),
    "GSEM npc": ("device", lambda: _bw().GSEM(Y16, X16, npc=3)),
    "MEGA empty trait": ("device", lambda: _bw().MEGA(np.column_stack([Y16[:, 0], np.full(16, np.nan)]), X16, npc=1)),
    "crossprod2 not a panel": ("device", lambda: _panel_call(lambda P: P.crossprod2(X16))),
    "kernel2 column mismatch": ("device", lambda: _panel_call(lambda P: _panel_call(lambda Q: P.kernel2(Q, "ARC"), X16[:, :7]))),
}


def _panel_call(f, X=X16):
    P = _bw().Panel(X)
    try:
        return f(P)
    finally:
        P.close()


def outcome(id_):
    """what the case raised, as the table holds it; a case that raises nothing says so"""
    try:
        CASES[id_][1]()
    except Exception as ex:    # noqa: BLE001  (the class is what is recorded)
        return "%s: %r" % (type(ex).__name__, str(ex))
    return "no refusal"


def read_table(path):
    """{id: (tag, outcome)} of the table (lines `tag  id  outcome`; `#` starts a comment)"""
    out = {}
    with open(path) as f:
        for line in f:
            if line.strip() and not line.startswith("#"):
                tag, id_, what = line.rstrip("\n").split("  ", 2)
                out[id_] = (tag, what)
    return out
