// bwgr_amd/csrc/pegsx_setup.h -- what PEGSX (pegsx_host.hip.h) does on the host before a kernel runs (src/RcppEigenX20251203.cpp:227-260):
// the observed-row masks and their missingness patterns, per pattern M'M of the masked fixed design M = w o X and its pseudo-inverse, per
// trait b = (M'M)^+ M'Y and the projected y = (Y - M b) o w.  There is no intercept and no centring.  Plain C++17, no device runtime:
// tests/pegsx_tail_check.cpp runs it as a program of its own under the sanitizers (tests/test_pegsx_cpu.py).
#pragma once
#include "traits.h"
#include "pegs_tail.h"

namespace bwgr {

struct FixedSet {
  TraitSet S;                        // n, k, ld, nt, obs; y: k columns of stride ld, the projected traits, +0.0 on unobserved rows and the padding
  Patterns pat;                      // of all k traits
  int64_t f = 0;
  int64_t bad_row = -1, bad_col = -1;   // the first non-finite entry of X in column-major order, or -1
  std::vector<double> X;             // n x f without its padding
  std::vector<double> iXX;           // per pattern f x f (symmetric)
  std::vector<double> ratios;        // per pattern f values |lambda| / max |lambda| of M'M, ascending in lambda
  std::vector<int> rank;             // per pattern
  std::vector<double> b;             // f x k column-major
  std::vector<double> ssy;           // y_t'y_t
};

// Y: n x k column-major, NaN = missing; X: n x f, column stride ldx >= n.  S.bad: the first trait with fewer than two records.  Sums run in
// ascending row order.
inline FixedSet read_fixed(const double *Y, const double *X, int64_t n, int64_t k, int64_t f, int64_t ldx, int64_t ld) {
  FixedSet F;
  F.f = f;
  TraitSet &S = F.S;
  S.n = n; S.k = k; S.ld = ld;
  const size_t nk = (size_t)k, nn = (size_t)n, nf = (size_t)f;
  S.nt.assign(nk, 0.0); S.mu.assign(nk, 0.0); S.sumy.assign(nk, 0.0); S.vy.assign(nk, 0.0);
  S.y.assign(nk * (size_t)ld, 0.0); S.obs.assign(nk * nn, 0);
  if (!compact_z(X, n, f, ldx, F.X, &F.bad_row, &F.bad_col)) return F;
  for (int64_t t = 0; t < k; ++t) {
    double cnt = 0.0;
    for (int64_t r = 0; r < n; ++r)
      if (!std::isnan(Y[(size_t)t * nn + (size_t)r])) { S.obs[(size_t)t * nn + (size_t)r] = 1; cnt += 1.0; }
    S.nt[(size_t)t] = cnt;
    if (cnt < 2.0) { S.bad = t; return F; }
  }
  F.pat = find_patterns(S, 0, k);
  const size_t npat = F.pat.rep.size();
  F.iXX.assign(npat * nf * nf, 0.0); F.ratios.assign(npat * nf, 0.0); F.rank.assign(npat, 0);
  std::vector<double> A(nf * nf);
  for (size_t g = 0; g < npat; ++g) {
    const uint8_t *w = S.obs.data() + (size_t)F.pat.rep[g] * nn;
    for (size_t a = 0; a < nf; ++a)
      for (size_t c = a; c < nf; ++c) {
        const double *xa = F.X.data() + a * nn, *xc = F.X.data() + c * nn;
        double s = 0.0;
        for (size_t r = 0; r < nn; ++r) if (w[r]) s += xa[r] * xc[r];
        A[a * nf + c] = A[c * nf + a] = s;
      }
    F.rank[g] = pegsx_pinv((int)f, A.data(), F.iXX.data() + g * nf * nf, F.ratios.data() + g * nf);
  }
  F.b.assign(nf * nk, 0.0); F.ssy.assign(nk, 0.0);
  std::vector<double> rhs(nf);
  for (int64_t t = 0; t < k; ++t) {
    const uint8_t *w = S.obs.data() + (size_t)t * nn;
    const double *Yt = Y + (size_t)t * nn, *iA = F.iXX.data() + (size_t)F.pat.id[(size_t)t] * nf * nf;
    double *bt = F.b.data() + (size_t)t * nf, *yt = S.y.data() + (size_t)t * (size_t)ld;
    for (size_t c = 0; c < nf; ++c) {
      const double *xc = F.X.data() + c * nn;
      double s = 0.0;
      for (size_t r = 0; r < nn; ++r) if (w[r]) s += xc[r] * Yt[r];
      rhs[c] = s;
    }
    for (size_t a = 0; a < nf; ++a) { double s = 0.0; for (size_t c = 0; c < nf; ++c) s += iA[a * nf + c] * rhs[c]; bt[a] = s; }
    double ss = 0.0;
    for (size_t r = 0; r < nn; ++r) {
      if (!w[r]) continue;
      double fit = 0.0;
      for (size_t c = 0; c < nf; ++c) fit += F.X[c * nn + r] * bt[c];
      yt[r] = Yt[r] - fit; ss += yt[r] * yt[r];
    }
    F.ssy[(size_t)t] = ss;
  }
  return F;
}

}  // namespace bwgr
