// bwgr_amd/csrc/csc.h -- the host-side work on a sparse effect of the multi-trait fits (PEGS_sparse / PEGSZ_sparse and sparse effects in
// PEGS / PEGSZ / PEGSX lists): a column-compressed (CSC) n x q matrix as the caller hands it over -- colptr int64[q + 1], rowidx int32[nnz],
// val double[nnz] -- is validated, tested for row-disjoint columns and copied row-major.  Plain C++17, no device runtime: tests/csc_check.cpp
// runs it as a program of its own under the sanitizers (tests/test_pegs_sparse_cpu.py).
//   csc_validate      colptr[0] == 0, colptr non-decreasing, nnz = colptr[q] <= 2^31 - 1, every row index in [0, n) and strictly increasing
//                     within its column (so no duplicates), every value finite (a stored zero is a value).  The fault names column and entry.
//   csc_row_disjoint  no row occurs in two columns (an incidence matrix: the columns of one factor).  O(nnz) with a bitmap of the rows.
//                     On such an effect Gauss-Seidel over the columns does not depend on their order, so the engine updates them all at once.
//   csc_to_csr        the row-major copy the fitted values read, columns ascending within a row
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

namespace bwgr {

enum : int { CSC_OK = 0, CSC_Q, CSC_PTR0, CSC_PTR_ORDER, CSC_NNZ, CSC_ROW_RANGE, CSC_ROW_ORDER, CSC_VALUE };
// what csc_validate found: col the column (CSC_PTR_ORDER: the column whose end lies before its start), entry the index into rowidx / val
struct CscFault { int what = CSC_OK; int64_t col = -1, entry = -1; };
static constexpr int64_t CSC_MAX_NNZ = 0x7FFFFFFFll;

inline const char *csc_why(int what) {
  switch (what) {
    case CSC_Q: return "q is below 1";
    case CSC_PTR0: return "colptr[0] is not 0";
    case CSC_PTR_ORDER: return "colptr decreases";
    case CSC_NNZ: return "colptr[q] exceeds 2^31 - 1 stored entries";
    case CSC_ROW_RANGE: return "a row index lies outside [0, n)";
    case CSC_ROW_ORDER: return "the row indices of a column do not strictly increase (unsorted or duplicated)";
    case CSC_VALUE: return "a value is not finite";
    default: return "";
  }
}

// (the pointers are not null; rowidx and val hold colptr[q] entries once colptr has passed)
inline bool csc_validate(int64_t n, int64_t q, const int64_t *colptr, const int32_t *rowidx, const double *val, CscFault &bad) {
  bad = CscFault();
  if (q < 1) { bad.what = CSC_Q; return false; }
  if (colptr[0] != 0) { bad.what = CSC_PTR0; bad.col = 0; return false; }
  for (int64_t j = 0; j < q; ++j)
    if (colptr[j + 1] < colptr[j]) { bad.what = CSC_PTR_ORDER; bad.col = j; return false; }
  if (colptr[q] > CSC_MAX_NNZ) { bad.what = CSC_NNZ; bad.col = q; return false; }
  for (int64_t j = 0; j < q; ++j)
    for (int64_t i = colptr[j]; i < colptr[j + 1]; ++i) {
      const int64_t r = rowidx[i];
      if (r < 0 || r >= n) { bad.what = CSC_ROW_RANGE; bad.col = j; bad.entry = i; return false; }
      if (i > colptr[j] && r <= (int64_t)rowidx[i - 1]) { bad.what = CSC_ROW_ORDER; bad.col = j; bad.entry = i; return false; }
      if (!std::isfinite(val[i])) { bad.what = CSC_VALUE; bad.col = j; bad.entry = i; return false; }
    }
  return true;
}

// the most stored entries of a column (a validated matrix)
inline int64_t csc_max_col_nnz(int64_t q, const int64_t *colptr) {
  int64_t m = 0;
  for (int64_t j = 0; j < q; ++j) m = std::max(m, colptr[j + 1] - colptr[j]);
  return m;
}

// true where no row occurs in two columns (a validated matrix: within a column no row repeats, so a row seen twice is seen in two columns)
inline bool csc_row_disjoint(int64_t n, int64_t q, const int64_t *colptr, const int32_t *rowidx) {
  std::vector<uint64_t> seen((size_t)((n + 63) / 64), 0);
  const int64_t nnz = colptr[q];
  for (int64_t i = 0; i < nnz; ++i) {
    const uint64_t r = (uint64_t)rowidx[i], bit = (uint64_t)1 << (r & 63);
    if (seen[(size_t)(r >> 6)] & bit) return false;
    seen[(size_t)(r >> 6)] |= bit;
  }
  return true;
}

// the matrix row-major: rowptr[n + 1], and per row its columns (ascending) and values
struct CsrCopy { std::vector<int64_t> rowptr; std::vector<int32_t> col; std::vector<double> val; };
inline void csc_to_csr(int64_t n, int64_t q, const int64_t *colptr, const int32_t *rowidx, const double *val, CsrCopy &out) {
  const int64_t nnz = colptr[q];
  out.rowptr.assign((size_t)n + 1, 0);
  out.col.resize((size_t)nnz); out.val.resize((size_t)nnz);
  for (int64_t i = 0; i < nnz; ++i) ++out.rowptr[(size_t)rowidx[i] + 1];
  for (int64_t r = 0; r < n; ++r) out.rowptr[(size_t)r + 1] += out.rowptr[(size_t)r];
  std::vector<int64_t> at(out.rowptr.begin(), out.rowptr.end() - 1);
  for (int64_t j = 0; j < q; ++j)
    for (int64_t i = colptr[j]; i < colptr[j + 1]; ++i) {
      const int64_t w = at[(size_t)rowidx[i]]++;
      out.col[(size_t)w] = (int32_t)j; out.val[(size_t)w] = val[i];
    }
}

}  // namespace bwgr
