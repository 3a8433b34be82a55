"""The five numpy.linalg routines the multi-trait restatements use on their k x k tail (k <= 16) -- solve, inv, pinv, eigvalsh, eigh -- for
symmetric input, in plain numpy and generic in dtype: numpy.linalg has no long double, and tests/mt_tight.py runs the restatements in it.

solve and inv are a Cholesky factorisation with two triangular solves, for symmetric positive definite A, batched over leading axes: one call
per sweep inverts every marker's k x k system, as k_mrr_linv does.  eigh is the cyclic Jacobi method (Rutishauser's rotations, as in
Numerical Recipes' jacobi), with ascending eigenvalues as numpy.linalg.eigh orders them; eigvalsh is its values.  pinv is made of the
eigenpairs with numpy.linalg.pinv's relative cut-off: a symmetric matrix's singular values are |w|, and those at or below rcond max |w|
are dropped.  Everything is computed in the dtype of the input (integers and float16 / float32 excepted: the floor is float64, as numpy's).
tests/test_mt_tight_cpu.py holds the module to numpy at float64 and to residuals of k 2^-63 |A| at long double."""
import numpy as np

RCOND = 1e-15   # numpy.linalg.pinv's default


def _dtype(*arrays):
    t = np.result_type(*arrays)
    return t if t in (np.dtype(np.float64), np.dtype(np.longdouble)) else np.dtype(np.float64)


def cholesky(A):
    """L with L L' = A, over the leading axes; A symmetric positive definite (its lower triangle is read).  NaN where it is not."""
    A = np.asarray(A, _dtype(A))
    k = A.shape[-1]
    L = np.zeros_like(A)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(k):
            d = A[..., j, j] - (L[..., j, :j] ** 2).sum(-1)
            L[..., j, j] = np.sqrt(d)
            if j + 1 < k:
                L[..., j + 1:, j] = (A[..., j + 1:, j] - (L[..., j + 1:, :j] * L[..., j:j + 1, :j]).sum(-1)) / L[..., j:j + 1, j]
    return L


def solve(A, B):
    """x with A x = B by Cholesky.  A: (..., k, k); B: (..., k) or (..., k, m), as numpy.linalg.solve reads them (a B of A's rank less one is
    a stack of vectors)."""
    f = _dtype(A, B)
    A, B = np.asarray(A, f), np.asarray(B, f)
    vec = B.ndim == A.ndim - 1
    X = np.array(B[..., None] if vec else B, f, copy=True)
    X = np.broadcast_to(X, np.broadcast_shapes(X.shape[:-2], A.shape[:-2]) + X.shape[-2:]).copy()
    L = cholesky(A)
    k = A.shape[-1]
    for i in range(k):                                               # L y = B
        X[..., i, :] = (X[..., i, :] - (L[..., i, :i, None] * X[..., :i, :]).sum(-2)) / L[..., i, i, None]
    for i in range(k - 1, -1, -1):                                   # L' x = y
        X[..., i, :] = (X[..., i, :] - (L[..., i + 1:, i, None] * X[..., i + 1:, :]).sum(-2)) / L[..., i, i, None]
    return X[..., 0] if vec else X


def inv(A):
    """A^-1 by Cholesky, over the leading axes; symmetric to the last bit."""
    A = np.asarray(A, _dtype(A))
    X = solve(A, np.broadcast_to(np.eye(A.shape[-1], dtype=A.dtype), A.shape))
    return (X + np.swapaxes(X, -1, -2)) / 2


def eigh(A):
    """(w ascending, V) with A V = V diag(w) for one symmetric k x k matrix, by cyclic Jacobi; at the end V is brought back to V'V = I by
    one Newton step and w is read as the Rayleigh quotients of its columns."""
    f = _dtype(A)
    A = np.array(A, f, copy=True)
    assert A.ndim == 2 and A.shape[0] == A.shape[1], A.shape
    A = (A + A.T) / 2
    A0 = A.copy()
    k = A.shape[0]
    V = np.eye(k, dtype=f)
    for sweep in range(100):
        off = np.abs(A[np.triu_indices(k, 1)]).sum()
        if off == 0:
            break
        for p in range(k - 1):
            for q in range(p + 1, k):
                apq = A[p, q]
                if apq == 0:
                    continue
                g = 100 * abs(apq)
                if sweep > 3 and abs(A[p, p]) + g == abs(A[p, p]) and abs(A[q, q]) + g == abs(A[q, q]):
                    A[p, q] = A[q, p] = 0
                    continue
                h = A[q, q] - A[p, p]
                if abs(h) + g == abs(h):
                    t = apq / h
                else:
                    theta = h / (2 * apq)
                    t = 1 / (abs(theta) + np.sqrt(theta * theta + 1))
                    if theta < 0:
                        t = -t
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                app, aqq = A[p, p] - t * apq, A[q, q] + t * apq
                rp, rq = A[p].copy(), A[q].copy()
                A[p] = c * rp - s * rq
                A[q] = s * rp + c * rq
                A[:, p], A[:, q] = A[p], A[q]
                A[p, p], A[q, q] = app, aqq
                A[p, q] = A[q, p] = 0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq
    else:
        raise np.linalg.LinAlgError("Jacobi did not converge")
    V = V @ (3 * np.eye(k, dtype=f) - V.T @ V) / 2      # one Newton step to V'V = I: takes off what a hundred rotations' roundings left
    w = ((A0 @ V) * V).sum(0)      # the Rayleigh quotients v'Av: the rotated diagonal without the roundings of its hundred updates
    order = np.argsort(w, kind="stable")
    return w[order], V[:, order]


def eigvalsh(A):
    return eigh(A)[0]


def pinv(A, rcond=RCOND):
    """the Moore-Penrose inverse of one symmetric matrix: V diag(1 / w) V' over the eigenvalues with |w| > rcond max |w|"""
    w, V = eigh(A)
    keep = np.abs(w) > w.dtype.type(rcond) * np.abs(w).max(initial=0)
    P = (V[:, keep] / w[keep]) @ V[:, keep].T
    return (P + P.T) / 2
