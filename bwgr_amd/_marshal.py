"""What the families of the host layer share when they hand arrays to the C ABI: seeds, pointer casts, the codes of include/bwgr.h, matrices as
the library reads them, plan hooks.  Only what at least two families use lives here."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import BwgrError, c_f, c_d, check

X_I8, X_F32, X_F64 = 0, 1, 2
HOST, DEVICE = 0, 1


def _seed(seed):
    if seed is None:
        return int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _fp(a):
    return a.ctypes.data_as(c_f)


def _dp(a):
    return a.ctypes.data_as(c_d)


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _is_device_tensor(X):
    return type(X).__module__.split(".")[0] == "torch" and bool(getattr(X, "is_cuda", False))


def _matrix(A, who, nrow=None, single=False, what="Y"):
    """A as a float64 matrix, a vector as one column; `single`: rounded through float, as the reference's float entries receive it.  With
    nrow, anything but nrow x k is refused in `who`'s name; without, the caller checks the shape itself (the entries whose refusal is an
    assertion or has a text of its own).  The layout is A's: what goes to the library passes through np.asfortranarray."""
    Am = np.asarray(A, np.float64)
    if Am.ndim == 1:
        Am = Am[:, None]
    if single:
        Am = Am.astype(np.float32).astype(np.float64)
    if nrow is not None and (Am.ndim != 2 or Am.shape[0] != nrow):
        raise BwgrError(1, "%s: %s has shape %s; nrow(%s) must equal nrow(X) = %d" % (who, what, Am.shape, what, nrow))
    return Am


def _plan(entry, names, *args, ctype=C.c_int64):
    """A hook that writes len(names) integers behind its integer arguments (a handle passes as it is): dict(name -> value)."""
    out = (ctype * len(names))()
    check(getattr(_lib.lib(), entry)(*[a if isinstance(a, C.c_void_p) else int(a) for a in args], out))
    return dict(zip(names, [int(v) for v in out]))
