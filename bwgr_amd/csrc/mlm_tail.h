// bwgr_amd/csrc/mlm_tail.h -- the k x k host work of MLM (src/RcppEigen20230423.cpp:1303-1391): the start values with their priors, the update
// of ve and vb after a sweep with its bending and pseudo-inverse, the convergence value, and h2 / GC at the end.  Plain C++17, no device
// runtime: tests/mlm_tail_check.cpp runs it as a program of its own under the sanitizers (tests/test_mlm_cpu.py).  The eigen-decomposition and
// the pseudo-inverse are pegs_tail.h's.
#pragma once
#include <math.h>
#include <vector>
#include "pegs_tail.h"   // mrr_eigh, mrr_pinv

namespace bwgr {

struct MlmState {
  int k = 0, numit = 0;
  double cnv = 10.0, inflate = 0.0, df0 = 0.0, minev = 0.0;      // :1328, :1315; minev: vb's smallest eigenvalue before the last bending
  std::vector<double> vy, ve, Se, iNp, Tr, Sb, vb, iG;           // Tr = TrZSZ; Sb: the prior's diagonal; vb, iG k x k row-major
};

// start values (:1303-1320): iN = 1 / (n_t - f), vy = y_t'y_t iN, ve = vy / 2, vb = diag(ve / (TrZSZ iN)), iG its inverse, Sb = df0 vb,
// Se = df0 ve, iNp = 1 / (n_t + df0 - f).  ssy[t] = y_t'y_t of the projected traits; Tr[t] = sum_j ZZ_jt.
inline void mlm_start(MlmState &S, int k, int f, double df0, const double *nt, const double *ssy, const double *Tr) {
  const size_t K = (size_t)k;
  S.k = k; S.numit = 0; S.cnv = 10.0; S.inflate = 0.0; S.df0 = df0; S.minev = 0.0;
  S.vy.resize(K); S.ve.resize(K); S.Se.resize(K); S.iNp.resize(K); S.Tr.assign(Tr, Tr + k); S.Sb.resize(K);
  S.vb.assign(K * K, 0.0); S.iG.assign(K * K, 0.0);
  for (int t = 0; t < k; ++t) {
    const double iN = 1.0 / (nt[t] - f);                                                           // :1278
    S.vy[t] = ssy[t] * iN;                                                                         // :1303
    S.ve[t] = S.vy[t] * 0.5;                                                                       // :1304
    S.vb[t * K + t] = S.ve[t] / (Tr[t] * iN);                                                      // :1307
    S.iG[t * K + t] = 1.0 / S.vb[t * K + t];                                                       // :1308 (the inverse of a diagonal matrix)
    S.Sb[t] = S.vb[t * K + t] * df0;                                                               // :1318
    S.Se[t] = S.ve[t] * df0;                                                                       // :1319
    S.iNp[t] = 1.0 / (nt[t] + df0 - f);                                                            // :1320
  }
}

// Everything after a sweep (:1354-1374).  ey[t] = e_t'y_t; TH = TildeHat, TH[s * k + t] = sum_j b_js tilde_jt; db2 = sum (delta b)^2 over all
// columns and traits.  inflate only grows: it becomes fabs(1.1 min) when vb's smallest eigenvalue is below 0.001 and that value exceeds it, and
// goes onto the diagonal in every sweep.  True when the bending raised inflate in this sweep.
inline bool mlm_after_sweep(MlmState &S, const double *ey, const double *TH, double db2) {
  const int k = S.k;
  for (int t = 0; t < k; ++t) S.ve[t] = (ey[t] + S.Se[t]) * S.iNp[t];                              // :1354-1355
  double *vb = S.vb.data();
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      if (i == j) vb[i * k + i] = (TH[i * k + i] + S.Sb[i]) / (S.Tr[i] + S.df0);                   // :1362
      else vb[i * k + j] = (TH[i * k + j] + TH[j * k + i]) / (S.Tr[i] + S.Tr[j]);                  // :1363
    }
  std::vector<double> w((size_t)k), V((size_t)k * k);
  mrr_eigh(k, vb, w.data(), V.data());                                                             // :1367
  S.minev = w[0];
  bool raised = false;
  if (w[0] < 0.001 && fabs(w[0] * 1.1) > S.inflate) { S.inflate = fabs(w[0] * 1.1); raised = true; }   // :1368
  for (int t = 0; t < k; ++t) vb[t * k + t] += S.inflate;                                          // :1369
  mrr_pinv(k, vb, S.iG.data());                                                                    // :1370
  ++S.numit;                                                                                       // :1373
  S.cnv = log10(db2);                                                                              // :1374
  return raised;
}

// on exit: h2 = 1 - ve / vy (:1385), GC = vb_ij / sqrt(vb_ii vb_jj) (:1391); GC k x k row-major
inline void mlm_finish(const MlmState &S, double *h2, double *GC) {
  const int k = S.k;
  for (int t = 0; t < k; ++t) h2[t] = 1.0 - S.ve[t] / S.vy[t];
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) GC[i * k + j] = S.vb[i * k + j] / sqrt(S.vb[i * k + i] * S.vb[j * k + j]);
}

}  // namespace bwgr
