// bwgr_amd/csrc/pegs_tail.h -- the k x k host work of the multi-trait fits: the symmetric eigen-decomposition and pseudo-inverse that mrr's tail
// (mrr.hip.h) and PEGS / PEGSZ share, and everything PEGS / PEGSZ do after a sweep (src/RcppEigenX20251203.cpp:122-171, :710-774): the
// residual variances, every effect's covariance from TildeHat and TrXSX, the XFA and NNC structures, bending with a carried inflate, the
// intercept step and the convergence value.  Plain C++17, no device runtime: tests/pegs_tail_check.cpp runs it as a program of its own under
// the sanitizers (tests/test_pegs_cpu.py).  At the end: the same for PEGSX (:336-365, :437-527), whose update has priors, floors, NNC before
// XFA and a stop rule of its own (tests/pegsx_tail_check.cpp, tests/test_pegsx_cpu.py).
#pragma once
#include <math.h>
#include <stddef.h>
#include <algorithm>
#include <vector>

namespace bwgr {

// Jacobi eigen-decomposition of a symmetric k x k matrix (row-major): w ascending, eigenvector i in column i of V.  The sweeps end when the
// off-diagonal part is below 1e-16 of the matrix in norm, or when a sweep no longer lowers it: a rotation never raises it but for rounding, and
// from about k = 17 on the rounding of k^2 entries keeps it above that bar (2.7e-31 of the squared norm at k = 256), where the loop used to
// run all its 100 sweeps (about ten seconds of host time at k = 256) for a result that the eleventh had reached.
inline void mrr_eigh(int k, const double *Ain, double *w, double *V) {
  std::vector<double> A(Ain, Ain + (size_t)k * k);
  std::vector<double> Vt((size_t)k * k, 0.0);          // the eigenvectors as rows while they are rotated: the update runs along a row
  for (int r = 0; r < k; ++r) Vt[(size_t)r * k + r] = 1.0;
  double prev = INFINITY;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (int r = 0; r < k; ++r) for (int c = 0; c < k; ++c) { tot += A[r * k + c] * A[r * k + c]; if (r != c) off += A[r * k + c] * A[r * k + c]; }
    if (off <= 1e-32 * tot || off == 0.0 || off >= prev) break;
    prev = off;
    for (int p = 0; p < k; ++p)
      for (int q = p + 1; q < k; ++q) {
        const double apq = A[p * k + q];
        if (apq == 0.0) continue;
        const double th = (A[q * k + q] - A[p * k + p]) / (2.0 * apq);
        const double t = (th >= 0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int r = 0; r < k; ++r) { const double arp = A[r * k + p], arq = A[r * k + q]; A[r * k + p] = c * arp - s * arq; A[r * k + q] = s * arp + c * arq; }
        for (int r = 0; r < k; ++r) { const double apr = A[p * k + r], aqr = A[q * k + r]; A[p * k + r] = c * apr - s * aqr; A[q * k + r] = s * apr + c * aqr; }
        for (int r = 0; r < k; ++r) { const double vrp = Vt[p * k + r], vrq = Vt[q * k + r]; Vt[p * k + r] = c * vrp - s * vrq; Vt[q * k + r] = s * vrp + c * vrq; }
      }
  }
  std::vector<int> idx(k);
  for (int i = 0; i < k; ++i) idx[i] = i;
  std::sort(idx.begin(), idx.end(), [&](int a, int b) { return A[a * k + a] < A[b * k + b]; });
  for (int i = 0; i < k; ++i) { w[i] = A[idx[i] * k + idx[i]]; for (int r = 0; r < k; ++r) V[r * k + i] = Vt[idx[i] * k + r]; }
}

// Moore-Penrose inverse of a symmetric matrix (singular values |lambda| below 1e-15 max |lambda| dropped)
inline void mrr_pinv(int k, const double *A, double *out) {
  std::vector<double> w(k), V((size_t)k * k);
  mrr_eigh(k, A, w.data(), V.data());
  double mx = 0.0;
  for (int i = 0; i < k; ++i) mx = std::max(mx, fabs(w[i]));
  for (int i = 0; i < k * k; ++i) out[i] = 0.0;
  for (int e = 0; e < k; ++e) {
    if (!(fabs(w[e]) > 1e-15 * mx)) continue;
    for (int r = 0; r < k; ++r) for (int c = 0; c < k; ++c) out[r * k + c] += V[r * k + e] * V[c * k + e] / w[e];
  }
}

// ---- PEGS / PEGSZ ----
// own_text: follow PEGS's own text where it differs from PEGSZ's -- the XFA branch whenever XFA > 0 (:139; PEGSZ: 0 < XFA < k, :734) and no
// guard on a zero TrXSX (:130-131; PEGSZ: :722-724).  XFA < 0 means k (:94, :679).  mu_div_n: the intercept step divides the residual sums
// by n_t, PEGSZ_sparse's text (iN_mu, :1202), where PEGS, PEGSZ and PEGS_sparse divide by n_t - 1 (:163-164, :760, :977).
struct PegsOpts { int maxit; double logtol, covbend, covMinEv; int XFA; bool NNC, own_text; bool mu_div_n = false; };
// what one covariance update did: vb's smallest and largest eigenvalue before bending (MinDVb, :157), whether inflate was added (:159), and
// where XFA truncated (0 < XFA < k) the gap between the last kept and the first dropped eigenvalue of GC (else -1)
struct PegsTrace { double MinDVb = 0, maxEv = 0, gap = -1; int inflated = 0; };
struct PegsEffect { std::vector<double> Tr, vb, iG; double inflate = 0.0; };   // TrXSX[k]; vb, iG k x k row-major
struct PegsState {
  int k = 0, numit = 0;
  double cnv = 10.0;                                       // :84
  std::vector<double> nt, vy, ve, mu;
  std::vector<PegsEffect> eff;
};

// nullptr, or why these options are refused
inline const char *pegs_refuses(int k, const PegsOpts &o) {
  if (o.maxit < 0) return "maxit is negative";
  if (std::isnan(o.logtol) || o.logtol == INFINITY) return "logtol is not a number below +inf";   // (-inf: run every sweep)
  if (!std::isfinite(o.covbend)) return "covbend is not finite";
  if (!std::isfinite(o.covMinEv)) return "covMinEv is not finite";
  if (o.XFA > k) return "XFA exceeds the number of traits (the reference takes the last XFA of k eigenvectors)";
  return nullptr;
}

// start values (:52-63, :634-649): TrXSX = n MSx, ve = vy / 2, vb = diag(ve / MSx), iG its inverse.  MSx: neff x k.  False where an
// effect's TrXSX is 0 for a trait (the start value is infinite there): *bad_eff, *bad_t say which.
inline bool pegs_init(PegsState &S, int k, int neff, const double *nt, const double *vy, const double *mu, const double *MSx, int *bad_eff, int *bad_t) {
  S.k = k; S.numit = 0; S.cnv = 10.0;
  S.nt.assign(nt, nt + k); S.vy.assign(vy, vy + k); S.mu.assign(mu, mu + k); S.ve.resize(k);
  for (int t = 0; t < k; ++t) S.ve[t] = vy[t] * 0.5;
  S.eff.assign((size_t)neff, PegsEffect());
  for (int e = 0; e < neff; ++e) {
    PegsEffect &E = S.eff[(size_t)e];
    E.Tr.resize(k); E.vb.assign((size_t)k * k, 0.0); E.iG.assign((size_t)k * k, 0.0);
    for (int t = 0; t < k; ++t) {
      const double ms = MSx[(size_t)e * k + t];
      E.Tr[t] = nt[t] * ms;
      if (!(E.Tr[t] != 0.0) || !std::isfinite(E.Tr[t])) { *bad_eff = e; *bad_t = t; return false; }
      E.vb[t * k + t] = S.ve[t] / ms; E.iG[t * k + t] = 1.0 / E.vb[t * k + t];
    }
  }
  return true;
}

// one effect's covariance after a sweep (:127-160, :717-756).  TH = TildeHat = b'tilde, k x k row-major.
inline void pegs_tail_vb(int k, const PegsOpts &o, const double *TH, PegsEffect &E, PegsTrace *tr) {
  const int XFA = o.XFA < 0 ? k : o.XFA;
  double *vb = E.vb.data();
  const double *Tr = E.Tr.data();
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      if (i == j) vb[i * k + i] = (o.own_text || Tr[i] != 0.0) ? TH[i * k + i] / Tr[i] : 0.0;
      else vb[i * k + j] = (o.own_text || Tr[i] + Tr[j] != 0.0) ? (TH[i * k + j] + TH[j * k + i]) / (Tr[i] + Tr[j]) : 0.0;
    }
  PegsTrace T;
  if (XFA == 0) {                                                                          // :134-138: the traits made independent
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) if (i != j) vb[i * k + j] = 0.0;
  } else if (o.own_text || XFA < k) {                                                      // :139-153, :734-747
    std::vector<double> sd(k), GC((size_t)k * k), w(k), V((size_t)k * k);
    for (int t = 0; t < k; ++t) { sd[t] = sqrt(vb[t * k + t]); if (sd[t] < 1e-12) sd[t] = 1e-12; }
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[i * k + j] = vb[i * k + j] / (sd[i] * sd[j]);
    mrr_eigh(k, GC.data(), w.data(), V.data());
    if (XFA < k) T.gap = w[k - XFA] - w[k - XFA - 1];
    for (int i = 0; i < k * k; ++i) GC[i] = 0.0;
    for (int e = k - XFA; e < k; ++e)
      for (int r = 0; r < k; ++r) for (int c = 0; c < k; ++c) GC[r * k + c] += w[e] * V[r * k + e] * V[c * k + e];
    for (int t = 0; t < k; ++t) GC[t * k + t] = 1.0;
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) vb[i * k + j] = sd[i] * GC[i * k + j] * sd[j];
  }
  if (o.NNC) for (int i = 0; i < k * k; ++i) vb[i] = std::max(vb[i], 0.0);                 // :156
  {
    std::vector<double> w(k), V((size_t)k * k);
    mrr_eigh(k, vb, w.data(), V.data());
    T.MinDVb = w[0]; T.maxEv = w[k - 1];
  }
  if (T.MinDVb < o.covMinEv) E.inflate = std::max(E.inflate, fabs(T.MinDVb * o.covbend));  // :158: carried as a running maximum
  if (k >= 5 || T.MinDVb < o.covMinEv) { for (int t = 0; t < k; ++t) vb[t * k + t] += E.inflate; T.inflated = 1; }   // :159
  mrr_pinv(k, vb, E.iG.data());                                                            // :160
  if (tr) *tr = T;
}

// Everything after a sweep.  ey[t] = e_t'y_t, ey[k + t] = sum(e_t); TH: every effect's TildeHat (neff x k x k); db2[e] = that effect's
// sum (delta b)^2.  Updates ve, every effect's vb / iG / inflate, mu, cnv and numit; d[t] is what the caller takes off e_t on its
// observed rows (:163-166, with 1 / (n_t - 1) as written there; 1 / n_t with o.mu_div_n).  True when the fit stops (cnv < logtol, :171).
inline bool pegs_after_sweep(PegsState &S, const PegsOpts &o, const double *ey, const double *TH, const double *db2, double *d, PegsTrace *tr) {
  const int k = S.k;
  for (int t = 0; t < k; ++t) S.ve[t] = ey[t] / (S.nt[t] - 1.0);                            // :123-124
  double s = 0.0;
  for (size_t e = 0; e < S.eff.size(); ++e) {
    pegs_tail_vb(k, o, TH + e * (size_t)k * k, S.eff[e], tr ? tr + e : nullptr);
    s += db2[e];
  }
  for (int t = 0; t < k; ++t) { d[t] = ey[k + t] / (o.mu_div_n ? S.nt[t] : S.nt[t] - 1.0); S.mu[t] += d[t]; }
  S.cnv = log10(s);                                                                        // :169, :766-770
  ++S.numit;
  return S.cnv < o.logtol;
}

// on exit: h2 = 1 - ve / vy (:175) and every effect's GC with the max(sd, 1e-12) floor (:180-183); GC: neff x k x k row-major
inline void pegs_finish(const PegsState &S, double *h2, double *GC) {
  const int k = S.k;
  for (int t = 0; t < k; ++t) h2[t] = 1.0 - S.ve[t] / S.vy[t];
  std::vector<double> sd(k);
  for (size_t e = 0; e < S.eff.size(); ++e) {
    const double *vb = S.eff[e].vb.data();
    for (int t = 0; t < k; ++t) { sd[t] = sqrt(vb[t * k + t]); if (sd[t] < 1e-12) sd[t] = 1e-12; }
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[e * (size_t)k * k + i * k + j] = vb[i * k + j] / (sd[i] * sd[j]);
  }
}

// ---- PEGSX (src/RcppEigenX20251203.cpp:197-573): fixed effects beside the random effects ----
// Moore-Penrose inverse of a symmetric m x m matrix for the fixed design's M'M: eigenvalues with |lambda| <= m 2^-23 max |lambda| are
// dropped -- the rank decision the reference's float decomposition takes, far from fp64 rounding noise, so that an exactly rank-deficient
// dummy coding loses the same directions whatever the last bits of M'M are.  On a full-rank matrix this is the inverse.  ratios (m values,
// or nullptr): |lambda_i| / max |lambda|, ascending in lambda; returns the rank.
inline int pegsx_pinv(int m, const double *A, double *out, double *ratios) {
  std::vector<double> w(m), V((size_t)m * m);
  mrr_eigh(m, A, w.data(), V.data());
  double mx = 0.0;
  for (int i = 0; i < m; ++i) mx = std::max(mx, fabs(w[i]));
  const double thr = (double)m * 0x1p-23 * mx;
  for (size_t i = 0; i < (size_t)m * m; ++i) out[i] = 0.0;
  int rank = 0;
  for (int e = 0; e < m; ++e) {
    if (ratios) ratios[e] = mx > 0.0 ? fabs(w[e]) / mx : 0.0;
    if (!(fabs(w[e]) > thr)) continue;
    ++rank;
    for (int r = 0; r < m; ++r) {
      const double vr = V[(size_t)r * m + e] / w[e];
      for (int c = 0; c < m; ++c) out[(size_t)r * m + c] += vr * V[(size_t)c * m + e];
    }
  }
  return rank;
}

struct PegsxOpts { int maxit; double logtol, covbend, covMinEv, df0; bool NNC, XFA; int NumXFA; };
// the floors of the reference's text, as bits of PegsxTrace::floors and of pegsx_init's *floors: which of them were active
enum : int {
  PEGSX_FL_DENOM = 1,      // max(n_t - f, 1) or max(n_t + df0 - f, 1)  (:338, :364)
  PEGSX_FL_VE = 2,         // max(ve, 1e-8)  (:341, :514)
  PEGSX_FL_TR = 4,         // max(Tr iN, 1e-8), max(Tr_i, 1e-8), max(Tr_i + Tr_j, 1e-8)  (:353, :441, :446)
  PEGSX_FL_SD = 8,         // max(sd, 1e-12), max(vb_ii, 1e-12) in the XFA branch  (:461, :481)
  PEGSX_FL_CNV = 16        // max(ss_max, 1e-20)  (:524)
};
struct PegsxTrace { double MinDVb = 0, maxEv = 0, gap = -1; int inflated = 0, floors = 0; };
struct PegsxEffect { std::vector<double> Tr, Sb, vb, iG; double inflate = 0.0; };   // TrZSZ[k], the prior's diagonal [k]; vb, iG k x k row-major
struct PegsxState {
  int k = 0, numit = 0;
  double cnv = 10.0;                                       // :370
  std::vector<double> nt, ve, Se, iNp;
  std::vector<PegsxEffect> eff;
};

inline const char *pegsx_refuses(const PegsxOpts &o) {
  if (o.maxit < 0) return "maxit is negative";
  if (std::isnan(o.logtol) || o.logtol == INFINITY) return "logtol is not a number below +inf";   // (-inf: run every sweep)
  if (!std::isfinite(o.covbend)) return "covbend is not finite";
  if (!std::isfinite(o.covMinEv)) return "covMinEv is not finite";
  if (!std::isfinite(o.df0) || o.df0 < 0.0) return "df0 is not a finite number >= 0";
  return nullptr;
}

// start values (:336-365): iN = 1 / max(n_t - f, 1), ve = max(ssy iN / 2, 1e-8), vb = diag(ve / max(Tr iN, 1e-8)), iG its inverse, the priors
// Sb = df0 vb and Se = df0 ve, iNp = 1 / max(n_t + df0 - f, 1).  ssy[t] = y_t'y_t of the projected traits; Tr: neff x k.
inline void pegsx_init(PegsxState &S, int k, int neff, int f, const PegsxOpts &o, const double *nt, const double *ssy, const double *Tr, int *floors) {
  int fl = 0;
  S.k = k; S.numit = 0; S.cnv = 10.0;
  S.nt.assign(nt, nt + k); S.ve.resize(k); S.Se.resize(k); S.iNp.resize(k);
  std::vector<double> iN(k);
  for (int t = 0; t < k; ++t) {
    if (nt[t] - f < 1.0) fl |= PEGSX_FL_DENOM;
    iN[t] = 1.0 / std::max(nt[t] - f, 1.0);
    S.ve[t] = 0.5 * ssy[t] * iN[t];
    if (S.ve[t] < 1e-8) { S.ve[t] = 1e-8; fl |= PEGSX_FL_VE; }
    S.Se[t] = o.df0 * S.ve[t];
    if (nt[t] + o.df0 - f < 1.0) fl |= PEGSX_FL_DENOM;
    S.iNp[t] = 1.0 / std::max(nt[t] + o.df0 - f, 1.0);
  }
  S.eff.assign((size_t)neff, PegsxEffect());
  for (int e = 0; e < neff; ++e) {
    PegsxEffect &E = S.eff[(size_t)e];
    E.Tr.assign(Tr + (size_t)e * k, Tr + (size_t)(e + 1) * k);
    E.Sb.resize(k); E.vb.assign((size_t)k * k, 0.0); E.iG.assign((size_t)k * k, 0.0);
    for (int t = 0; t < k; ++t) {
      double den = E.Tr[t] * iN[t];
      if (den < 1e-8) { den = 1e-8; fl |= PEGSX_FL_TR; }
      E.vb[t * k + t] = S.ve[t] / den; E.iG[t * k + t] = 1.0 / E.vb[t * k + t]; E.Sb[t] = o.df0 * E.vb[t * k + t];
    }
  }
  if (floors) *floors = fl;
}

// one effect's covariance after a sweep (:437-498): the update with its prior and floors, NNC, then XFA, bending with the carried inflate,
// iG = pinv(vb).  TH = TildeHat = u'tilde, k x k row-major.
inline void pegsx_tail_vb(int k, const PegsxOpts &o, const double *TH, PegsxEffect &E, PegsxTrace *tr) {
  double *vb = E.vb.data();
  const double *Tr = E.Tr.data();
  PegsxTrace T;
  for (int i = 0; i < k; ++i) {
    if (Tr[i] < 1e-8) T.floors |= PEGSX_FL_TR;
    vb[i * k + i] = (TH[i * k + i] + E.Sb[i]) / (std::max(Tr[i], 1e-8) + o.df0);
    for (int j = i + 1; j < k; ++j) {
      if (Tr[i] + Tr[j] < 1e-8) T.floors |= PEGSX_FL_TR;
      vb[i * k + j] = vb[j * k + i] = (TH[i * k + j] + TH[j * k + i]) / std::max(Tr[i] + Tr[j], 1e-8);
    }
  }
  if (o.NNC) for (int i = 0; i < k * k; ++i) vb[i] = std::max(vb[i], 0.0);                 // :453-457 (vb is symmetric already)
  if (o.XFA && o.NumXFA > 0) {                                                             // :459-485
    const int nf = std::min(o.NumXFA, k);
    std::vector<double> sd(k), sc(k), GC((size_t)k * k), w(k), V((size_t)k * k);
    for (int t = 0; t < k; ++t) {
      sd[t] = sqrt(vb[t * k + t]);
      if (sd[t] < 1e-12) { sd[t] = 1e-12; T.floors |= PEGSX_FL_SD; }
      if (vb[t * k + t] < 1e-12) T.floors |= PEGSX_FL_SD;
      sc[t] = sqrt(std::max(vb[t * k + t], 1e-12));
    }
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[i * k + j] = vb[i * k + j] / (sd[i] * sd[j]);
    mrr_eigh(k, GC.data(), w.data(), V.data());
    if (nf < k) T.gap = w[k - nf] - w[k - nf - 1];
    for (int i = 0; i < k * k; ++i) GC[i] = 0.0;
    for (int e = k - nf; e < k; ++e)
      for (int r = 0; r < k; ++r) for (int c = 0; c < k; ++c) GC[r * k + c] += w[e] * V[r * k + e] * V[c * k + e];
    for (int t = 0; t < k; ++t) GC[t * k + t] = 1.0;
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) vb[i * k + j] = GC[i * k + j] * (sc[i] * sc[j]);
  }
  {
    std::vector<double> w(k), V((size_t)k * k);
    mrr_eigh(k, vb, w.data(), V.data());
    T.MinDVb = w[0]; T.maxEv = w[k - 1];
  }
  if (T.MinDVb < o.covMinEv) E.inflate = std::max(E.inflate, fabs(T.MinDVb * o.covbend));  // :489-492: carried as a running maximum
  if (k >= 5 || T.MinDVb < o.covMinEv) { for (int t = 0; t < k; ++t) vb[t * k + t] += E.inflate; T.inflated = 1; }   // :494-496
  mrr_pinv(k, vb, E.iG.data());                                                            // :498
  if (tr) *tr = T;
}

// Everything after a sweep and its fixed step.  ey[t] = e_t'y_t; TH: every effect's TildeHat (neff x k x k); db2[e] = that effect's
// sum (delta u)^2.  Updates every effect's vb / iG / inflate, ve, cnv (the maximum over the effects, :519-524) and numit.  True when the
// fit stops: numit >= 5 and cnv < logtol, or cnv NaN (:527).
inline bool pegsx_after_sweep(PegsxState &S, const PegsxOpts &o, const double *ey, const double *TH, const double *db2, PegsxTrace *tr) {
  const int k = S.k;
  int fl = 0;
  double smax = 0.0;
  for (size_t e = 0; e < S.eff.size(); ++e) {
    pegsx_tail_vb(k, o, TH + e * (size_t)k * k, S.eff[e], tr ? tr + e : nullptr);
    smax = std::max(smax, db2[e]);                                                         // (a NaN is kept below)
    if (std::isnan(db2[e])) smax = db2[e];
  }
  for (int t = 0; t < k; ++t) {
    S.ve[t] = (ey[t] + S.Se[t]) * S.iNp[t];                                                // :512-514
    if (S.ve[t] < 1e-8) { S.ve[t] = 1e-8; fl |= PEGSX_FL_VE; }
  }
  if (smax < 1e-20) { smax = 1e-20; fl |= PEGSX_FL_CNV; }
  S.cnv = log10(smax);
  ++S.numit;
  if (tr) tr[0].floors |= fl;
  return S.numit >= 5 && (S.cnv < o.logtol || std::isnan(S.cnv));
}

// on exit: every effect's GC with the max(sd, 1e-12) floor (:549-552); GC: neff x k x k row-major
inline void pegsx_finish(const PegsxState &S, double *GC) {
  const int k = S.k;
  std::vector<double> sd(k);
  for (size_t e = 0; e < S.eff.size(); ++e) {
    const double *vb = S.eff[e].vb.data();
    for (int t = 0; t < k; ++t) { sd[t] = sqrt(vb[t * k + t]); if (sd[t] < 1e-12) sd[t] = 1e-12; }
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[e * (size_t)k * k + i * k + j] = vb[i * k + j] / (sd[i] * sd[j]);
  }
}

}  // namespace bwgr
