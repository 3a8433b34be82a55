// tests/csc_check.cpp -- the host-side work on a sparse effect (bwgr_amd/csrc/csc.h) on hand-made matrices: every refusal of the
// validation with the column and entry it names, the row-disjointness verdicts, the longest column and the row-major copy entry by entry.
// A program of its own: built with -fsanitize=address,undefined and run by tests/test_pegs_sparse_cpu.py.  The arrays are heap vectors of
// exactly the stated lengths, so a read past colptr[q] or past the nnz entries is the sanitizer's to report.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../bwgr_amd/csrc/csc.h"

using namespace bwgr;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #c); ++g_failed; } } while (0)

struct Mat { int64_t n, q; std::vector<int64_t> p; std::vector<int32_t> i; std::vector<double> x; };

static CscFault validate(const Mat &M) {
  CscFault bad;
  const bool ok = csc_validate(M.n, M.q, M.p.data(), M.i.data(), M.x.data(), bad);
  CHECK(ok == (bad.what == CSC_OK));
  return bad;
}
static void refused(const Mat &M, int what, int64_t col, int64_t entry) {
  const CscFault bad = validate(M);
  CHECK(bad.what == what); CHECK(bad.col == col); CHECK(bad.entry == entry);
  CHECK(csc_why(bad.what)[0] != 0);
}

int main() {
  // 5 x 4: an incidence with an empty column (2) -- rows 0, 3 | 1 | - | 2, 4
  const Mat inc = {5, 4, {0, 2, 3, 3, 5}, {0, 3, 1, 2, 4}, {1, 1, 1, 1, 1}};
  CHECK(validate(inc).what == CSC_OK);
  CHECK(csc_row_disjoint(inc.n, inc.q, inc.p.data(), inc.i.data()));
  CHECK(csc_max_col_nnz(inc.q, inc.p.data()) == 2);
  // 4 x 3 with overlap (row 1 in columns 0 and 2), a stored zero and a negative value
  const Mat ovl = {4, 3, {0, 2, 3, 6}, {0, 1, 3, 1, 2, 3}, {0.5, -2.0, 0.0, 4.0, 1.5, -1.0}};
  CHECK(validate(ovl).what == CSC_OK);
  CHECK(!csc_row_disjoint(ovl.n, ovl.q, ovl.p.data(), ovl.i.data()));
  CHECK(csc_max_col_nnz(ovl.q, ovl.p.data()) == 3);
  // all columns empty; one column, one row; rows beyond a multiple of 64 (the bitmap's last word)
  const Mat none = {3, 2, {0, 0, 0}, {}, {}};
  CHECK(validate(none).what == CSC_OK && csc_row_disjoint(none.n, none.q, none.p.data(), none.i.data()) && csc_max_col_nnz(none.q, none.p.data()) == 0);
  const Mat one = {1, 1, {0, 1}, {0}, {3.0}};
  CHECK(validate(one).what == CSC_OK && csc_row_disjoint(one.n, one.q, one.p.data(), one.i.data()));
  const Mat wide = {130, 3, {0, 2, 4, 5}, {63, 64, 0, 129, 128}, {1, 1, 1, 1, 1}};
  CHECK(validate(wide).what == CSC_OK && csc_row_disjoint(wide.n, wide.q, wide.p.data(), wide.i.data()));
  const Mat wide2 = {130, 3, {0, 2, 4, 5}, {63, 129, 0, 64, 129}, {1, 1, 1, 1, 1}};
  CHECK(validate(wide2).what == CSC_OK && !csc_row_disjoint(wide2.n, wide2.q, wide2.p.data(), wide2.i.data()));

  // ---- every refusal, with what it names ----
  { Mat M = inc; M.q = 0; refused(M, CSC_Q, -1, -1); }
  { Mat M = inc; M.p[0] = 1; refused(M, CSC_PTR0, 0, -1); }
  { Mat M = inc; M.p[2] = 1; refused(M, CSC_PTR_ORDER, 1, -1); }                       // column 1 ends before it starts
  { Mat M = {5, 1, {0, (int64_t)1 << 31}, {0}, {1.0}}; refused(M, CSC_NNZ, 1, -1); }     // (refused before any entry is read)
  { Mat M = {5, 1, {0, CSC_MAX_NNZ + 1}, {0}, {1.0}}; refused(M, CSC_NNZ, 1, -1); }
  { Mat M = inc; M.i[4] = 5; refused(M, CSC_ROW_RANGE, 3, 4); }                        // row n
  { Mat M = inc; M.i[2] = -1; refused(M, CSC_ROW_RANGE, 1, 2); }
  { Mat M = inc; M.i[1] = 0; refused(M, CSC_ROW_ORDER, 0, 1); }                        // a duplicate
  { Mat M = ovl; M.i[4] = 3; M.i[5] = 2; refused(M, CSC_ROW_ORDER, 2, 5); }            // unsorted
  { Mat M = ovl; M.x[3] = NAN; refused(M, CSC_VALUE, 2, 3); }
  { Mat M = ovl; M.x[1] = INFINITY; refused(M, CSC_VALUE, 0, 1); }
  { Mat M = ovl; M.x[5] = -INFINITY; refused(M, CSC_VALUE, 2, 5); }
  // the first fault in column order is the one named
  { Mat M = ovl; M.x[5] = NAN; M.i[0] = 9; refused(M, CSC_ROW_RANGE, 0, 0); }

  // ---- the row-major copy, entry by entry ----
  {
    CsrCopy R;
    csc_to_csr(ovl.n, ovl.q, ovl.p.data(), ovl.i.data(), ovl.x.data(), R);
    const std::vector<int64_t> rp = {0, 1, 3, 4, 6};
    const std::vector<int32_t> rc = {0, 0, 2, 2, 1, 2};
    const std::vector<double> rv = {0.5, -2.0, 4.0, 1.5, 0.0, -1.0};
    CHECK(R.rowptr == rp); CHECK(R.col == rc); CHECK(R.val == rv);
    // and against the dense copy: every entry of both, both ways
    std::vector<double> A((size_t)(ovl.n * ovl.q), 0.0), B(A.size(), 0.0);
    for (int64_t j = 0; j < ovl.q; ++j) for (int64_t i = ovl.p[(size_t)j]; i < ovl.p[(size_t)j + 1]; ++i) A[(size_t)(j * ovl.n + ovl.i[(size_t)i])] += ovl.x[(size_t)i];
    for (int64_t r = 0; r < ovl.n; ++r) for (int64_t i = R.rowptr[(size_t)r]; i < R.rowptr[(size_t)r + 1]; ++i) B[(size_t)(R.col[(size_t)i] * ovl.n + r)] += R.val[(size_t)i];
    CHECK(A == B);
  }
  {
    CsrCopy R;
    csc_to_csr(inc.n, inc.q, inc.p.data(), inc.i.data(), inc.x.data(), R);
    const std::vector<int64_t> rp = {0, 1, 2, 3, 4, 5};
    const std::vector<int32_t> rc = {0, 1, 3, 0, 3};
    CHECK(R.rowptr == rp); CHECK(R.col == rc); CHECK(R.val == inc.x);
    csc_to_csr(none.n, none.q, none.p.data(), none.i.data(), none.x.data(), R);
    CHECK(R.rowptr == std::vector<int64_t>(4, 0) && R.col.empty() && R.val.empty());
  }
  if (g_failed) { fprintf(stderr, "csc_check: %d checks failed\n", g_failed); return 1; }
  printf("csc_check ok\n");
  return 0;
}
