// bwgr_amd/csrc/uvb_tail.h -- the host algebra of the per-trait ridge fits (uvb_host.hip.h: bwgr_uvbeta, bwgr_uvbeta2, bwgr_uvbeta_dense): a
// trait's start values, what a sweep's sums make of its mu, variances, lambdas and cnv (src/RcppEigen20230423.cpp:1418-1423, :1433-1441,
// :1455-1462, :1478-1487, :1730, :1794-1802), its results, and the LDS slots of the solve workgroups.  Plain C++17, no device runtime:
// tests/uvb_tail_check.cpp runs it as a program of its own under the sanitizers (tests/test_uvb_tail_cpu.py).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <cmath>
#include <vector>
#include "../../include/bwgr.h"

namespace bwgr {

// what the kernels read of a trait (uvb.hip.h) and of its dense leg (uvb2.hip.h)
struct UvbTrait {
  double lam, nt;    // lambda of this sweep; observed rows
  int pat, slot;     // the trait's pattern within its group; the LDS slot its Gram matrix is staged in (-1: read from global memory)
  int active, pad_;
};
struct Uvb2Trait {
  double lam, nt;       // lambda_1 of this sweep; observed rows
  int64_t moff;         // where the trait's row mask (bytes, 0xFF = observed) starts in the masks' array
  int run, pad_;        // the leg runs this trait in this sweep
};

// trait t's results: a trait without rows gives mu = h2 = 0 and no variances; xsolver1xF (noVar) estimates none
struct UvbOut { double *mu, *h2, *ve, *vb, *cnv; int *its; };
inline void uvb_result(const UvbOut &o, int64_t t, bool none, int variant, double mu, double ve, double vb, double vy, double cnv, int its) {
  const bool noVar = variant == BWGR_UVB_X;
  if (o.mu) o.mu[t] = none ? 0.0 : mu;
  if (o.h2) o.h2[t] = none ? 0.0 : (noVar ? NAN : 1.0 - ve / vy);                                          // :1802
  if (o.ve) o.ve[t] = (none || noVar) ? NAN : ve;
  if (o.vb) o.vb[t] = (none || noVar) ? NAN : vb;
  if (o.cnv) o.cnv[t] = cnv;
  o.its[t] = its;
}

// the LDS slots of every solve workgroup: the first ngl distinct patterns among its ST traits (UvbTrait::slot; -1: read from global memory);
// W traits per group, nsolve = W / ST solve workgroups per group
struct UvbSlotDims { int64_t groups; int nsolve, ngl, W, ST; };
inline std::vector<int> uvb_slots(std::vector<UvbTrait> &tr, const UvbSlotDims &d) {
  std::vector<int> slotpat((size_t)d.groups * d.nsolve * d.ngl, -1);
  for (int64_t g = 0; g < d.groups; ++g)
    for (int sb = 0; sb < d.nsolve; ++sb) {
      int *sp = slotpat.data() + ((size_t)g * d.nsolve + sb) * d.ngl;
      int used = 0;
      for (int tl = 0; tl < d.ST; ++tl) {
        UvbTrait &u = tr[(size_t)(g * d.W + sb * d.ST + tl)];
        if (u.nt == 0.0) continue;
        for (int s = 0; s < used && u.slot < 0; ++s) if (sp[s] == u.pat) u.slot = s;
        if (u.slot < 0 && used < d.ngl) { sp[used] = u.pat; u.slot = used++; }
      }
    }
  return slotpat;
}

// a trait of a fit on the host; lam, lam1: the lambdas of the next sweep (UvbTrait::lam, Uvb2Trait::lam)
struct UvbState {
  double nt = 0, mu = 0, sumy = 0, vy = 0, TrXSX = 0, ve = NAN, vb = NAN, ve0 = 0, vb0 = 0, cnv = NAN, lam = 0; int its = 0; bool active = false;
  double TrXSX1 = 0, vb1 = NAN, vb01 = 0, lam1 = 0; bool skip1 = false, skip2 = false;   // (the dense design's; skip: TrXSX of that design is 0)
};
// The start values of a trait with rows, from TrXSX = sum_j XX_j over the p markers (TrXSX1 given: solver2x's, with the dense design's)
inline void uvb_start(UvbState &q, int variant, double df0, int64_t p, double TrXSX, const double *TrXSX1) {
  q.TrXSX = TrXSX;                                                                                       // :1418
  const double MSx = q.TrXSX / (q.nt - 1.0);                                                             // :1419
  if (variant == BWGR_UVB_X) { q.lam = q.TrXSX / (double)p; return; }                        // lambda = XX.mean(), :1730
  q.ve = q.vy * 0.5; q.vb = (q.vy * 0.5) / MSx;                                                          // :1420
  q.lam = q.ve / q.vb; q.vb0 = q.vb * df0; q.ve0 = q.ve * df0;                               // :1423
  if (!TrXSX1) return;
  // solver2x's set-up of the two designs (:1455-1462).  A design with TrXSX = 0 on this trait's rows is skipped: its lambda is never
  // formed and its vb stays NaN; every XX of it is 0, so the panel leg leaves such a trait's b and e as they are
  q.skip2 = q.TrXSX == 0.0;
  if (q.skip2) { q.vb = NAN; q.vb0 = 0.0; q.lam = 0.0; }
  q.TrXSX1 = *TrXSX1;
  q.skip1 = q.TrXSX1 == 0.0;
  if (q.skip1) return;
  q.vb1 = (q.vy * 0.5) / (q.TrXSX1 / (q.nt - 1.0));                                                      // :1456-1457
  q.lam1 = q.ve / q.vb1; q.vb01 = q.vb1 * df0;                                               // :1461-1462
}
// a sweep's sums for one trait: of e, e'y, e'e over its rows; b'b, tilde'b and sum (delta b)^2 over the markers; leg: the dense leg's (or null)
struct UvbSums { double se, ey, ee, bb, tb, db2; const double *leg; };
// The tail of a trait that ran (:1433-1441, :1636-1644, :1739-1741, :1794-1801; leg given: solver2x's, :1478-1486, over q1 dense columns):
// mu, the variances, the lambdas, cnv and whether it goes on.  Returns mu0 = mean(e), which the caller takes off e.
inline double uvb_update(UvbState &q, const UvbSums &s, int variant, int maxit, double logtol, double df0, int64_t p, int64_t q1) {
  const double m0 = s.se / q.nt;                                             // mu0 = mean(e); the sums below are those of e - mu0
  q.mu += m0;
  const double ey1 = s.ey - m0 * q.sumy, ee1 = s.ee - 2.0 * m0 * s.se + q.nt * m0 * m0;
  double d1 = 0.0;
  if (s.leg) {
    q.ve = (ee1 + ey1 + q.ve0) / (2.0 * q.nt - 1.0 + df0);                   // :1479-1481
    if (!q.skip1) {
      d1 = s.leg[0];
      q.vb1 = (s.leg[2] + s.leg[1] + q.vb01) / (q.TrXSX1 + (double)q1 + df0);   // :1482, :1484
      q.lam1 = q.ve / q.vb1;                                                 // :1485
    }
    if (!q.skip2) {
      q.vb = (s.tb + s.bb + q.vb0) / (q.TrXSX + (double)p + df0);            // :1483-1484
      q.lam = q.ve / q.vb;
    }
  } else if (variant == BWGR_UVB_D || variant == BWGR_UVB_F) {
    q.ve = (ey1 + ee1 + q.ve0) / (2.0 * q.nt - 1.0 + df0);                   // :1434-1436
    q.vb = (s.bb + s.tb + q.vb0) / (q.TrXSX + (double)p + df0);              // :1437-1439
    q.lam = q.ve / q.vb;
  } else if (variant == BWGR_UVB_Z) {
    q.ve = (ey1 + q.ve0) / (q.nt + df0);                                     // :1795-1796
    q.vb = (s.tb + q.vb0) / (q.TrXSX + df0);                                 // :1797-1798
    q.lam = q.ve / q.vb;
  }
  q.cnv = s.leg ? log10(d1 + s.db2) : log10(s.db2);                          // :1486; :1440
  ++q.its;
  if (q.cnv < logtol || q.its == maxit || std::isnan(q.cnv)) q.active = false;   // :1441, :1487
  return m0;
}

}  // namespace bwgr
