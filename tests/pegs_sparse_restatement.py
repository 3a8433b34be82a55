"""What tests/pegs_restatement.py and tests/pegsx_restatement.py lack for the sparse effects (bWGR src/RcppEigenX20251203.cpp:811-1007,
:1010-1250): a column-compressed builder in numpy, so that the tests need no scipy, and PEGSZ_sparse's text.

The sparse functions are PEGS / PEGSZ with the designs held column-compressed: every sum runs over the stored entries and gives the numbers
of the dense copy, so PEGS_sparse is restated by pegs_restatement.pegs and a sparse effect in a PEGSZ / PEGSX list by pegsz / pegsx, each on
the dense copy (values rounded to float, as the reference casts S).  The text that differs is PEGSZ_sparse's intercept step, which
divides the residual sums by n_t (iN_mu, :1202) where PEGSZ divides by n_t - 1 (:760), and its 1 / (max(n_t, 1) - 1) (:1076): pegsz_sparse
below is pegs_restatement.pegsz(mu_div_n=True) on the float-rounded designs, always with pegsz's trace.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pegs_restatement as PR  # noqa: E402


def csc(A, stored=None):
    """(data, indices int32, indptr int64) of the 2-D array A, rows ascending within a column: its nonzeros, or the entries where the mask
    `stored` is set (a stored zero is an entry)"""
    A = np.asarray(A, np.float64)
    cols, rows = np.nonzero(A.T if stored is None else np.asarray(stored).T)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=A.shape[1]))]).astype(np.int64)
    return A[rows, cols].copy(), rows.astype(np.int32), indptr


def f32(A):
    return np.asarray(A, np.float64).astype(np.float32).astype(np.float64)


def row_disjoint(A):
    return bool(np.all((np.asarray(A) != 0).sum(1) <= 1))




def pegsz_sparse(Y, X_list, **kw):
    """PEGSZ_sparse (:1010-1250) on the dense copies X_list, rounded to float (:1028): pegs_restatement.pegsz under mu_div_n=True, with its
    trace; every option of pegsz (orders=, dtype=, dot=) passes through"""
    n = np.asarray(Y).shape[0]
    return PR.pegsz(Y, [f32(np.asarray(X, np.float64).reshape(n, -1)) for X in X_list], mu_div_n=True, trace=True, **kw)
