// bwgr_amd: the dense leg of the two-design per-trait ridge engine (bwgr_uvbeta2) -- solver2x (src/RcppEigen20230423.cpp:1446-1493), the
// solver of MEGA (:1542-1579) and GSEM (:1582-1610).
//
// solver2x walks two designs against one residual in every sweep: first the q columns of a small dense design Z (the latent spaces, :1470-1473),
// then the p markers of X (:1474-1477), each design with its own lambda.  The panel leg is uvb.hip.h's launch train as it stands; this header
// is the leg in front of it.  It is uvbd.hip.h's sweep cut out of its fit: one workgroup per trait of a 64-trait group, one launch per group
// and sweep, working on the trait's row of the engine's residual E ([trait][ld] doubles in global memory).
//   k_uvb2_setup   once per call, one workgroup per trait: zbar_jt, XX1_jt (two passes: the sum of squares of the centred column),
//                  tilde1_jt = sum_r z_rj y_rt on the raw column (:1451), TrXSX1_t = sum_j XX1_jt in column order
//   k_uvb2_leg     per sweep and group: loads the trait's row of E into LDS (LDS = true; uvbd_plan's rule, the same carve-up) or works on it in
//                  place (LDS = false), runs the q steps of uvbd.hip.h in the sweep's order with the thread-owns-its-rows rule and uvbd_sum's
//                  one-barrier sums, stores E back and leaves b1 and, summed by thread 0 in natural column order, sum (delta b1)^2, b1'b1 and
//                  tilde1'b1.  The panel leg's first pass forms its dots and sum e from E as stored, so it sees what this leg wrote.
// A trait that does not run this sweep (frozen, empty, or a dense design that is constant on its rows: run = 0) returns before it
// writes anything.  Per-column values live in the trait's slices of global arrays, so q has no limit.  Rows n .. ld - 1 of E are never touched.
#pragma once
#include "uvbd.hip.h"
#include "uvb_tail.h"

namespace bwgr {

// (Uvb2Trait, what the leg reads of a trait: uvb_tail.h)
static constexpr int UVB2_NLEG = 3;   // leg[t][.]: sum (delta b1)^2, b1'b1, tilde1'b1

struct Uvb2Args {
  const double *Z; int64_t n, q, ld;  // n x q, column-major, leading dimension n;  ld: the stride of y and e
  const double *y; double *e;         // [trait][ld]
  const uint8_t *zm;
  const Uvb2Trait *tr;
  const int32_t *order;               // [q]: this sweep's
  double *zbar, *XX, *tilde, *b, *dlt;   // [trait][q]
  double *trx;                        // [trait]: TrXSX1
  double *leg;                        // [trait][UVB2_NLEG]
};

// grid: the traits of the call; a trait without rows has nothing to set up
__global__ __launch_bounds__(UVBD_TMAX) void k_uvb2_setup(const Uvb2Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);
  const int t = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const Uvb2Trait tr = A.tr[t];
  if (tr.nt == 0.0) return;
  const int64_t n = A.n, q = A.q;
  const double *y = A.y + (size_t)t * A.ld;
  const uint8_t *m = A.zm + tr.moff;
  double *zbar = A.zbar + (size_t)t * q, *XX = A.XX + (size_t)t * q, *tilde = A.tilde + (size_t)t * q;
  int flip = 0;
  double trx = 0.0;   // (every thread holds the same bits)
  for (int64_t j = 0; j < q; ++j) {
    const double *z = A.Z + (size_t)j * n;
    double v[2] = {0.0, 0.0};
    for (int64_t r = tid; r < n; r += T) { const double zv = z[r]; if (m[r]) v[0] += zv; v[1] = fma(zv, y[r], v[1]); }   // :1451 (y is 0 off the trait's rows)
    uvbd_sum<2>(v, red, flip);
    const double zb = v[0] / tr.nt;                                                                                    // :1452
    double w[1] = {0.0};
    for (int64_t r = tid; r < n; r += T) if (m[r]) { const double c = z[r] - zb; w[0] = fma(c, c, w[0]); }
    uvbd_sum<1>(w, red, flip);                                                                                         // :1454
    if (tid == 0) { zbar[j] = zb; XX[j] = w[0]; tilde[j] = v[1]; }
    trx += w[0];                                                                                                       // :1455
  }
  if (tid == 0) A.trx[t] = trx;
}

// grid: the traits of one group, at most 64 (the arrays are offset to the group's first trait)
template <bool LDS> __global__ __launch_bounds__(UVBD_TMAX) void k_uvb2_leg(const Uvb2Args A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);
  const int t = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const Uvb2Trait tr = A.tr[t];
  if (!tr.run) return;
  const int64_t n = A.n, q = A.q;
  double *eg = A.e + (size_t)t * A.ld;
  double *e = LDS ? reinterpret_cast<double *>(smem + UVBD_LDS_FIXED) : eg;
  const uint8_t *m = A.zm + tr.moff;
  const double *zbar = A.zbar + (size_t)t * q, *XX = A.XX + (size_t)t * q, *tilde = A.tilde + (size_t)t * q;
  double *b = A.b + (size_t)t * q, *dlt = A.dlt + (size_t)t * q;
  int flip = 0;
  if (LDS) for (int64_t r = tid; r < n; r += T) e[r] = eg[r];   // (a row is only ever touched by its own thread: no barrier)
  for (int64_t s = 0; s < q; ++s) {                                                        // :1470
    const int J = A.order[s];
    const double *z = A.Z + (size_t)J * n;
    const double xx = XX[J], zb = zbar[J], b0 = b[J];
    double v[2] = {0.0, 0.0};
    for (int64_t r = tid; r < n; r += T) { const double ev = e[r]; v[0] = fma(z[r], ev, v[0]); v[1] += ev; }
    uvbd_sum<2>(v, red, flip);
    double b1 = 0.0, d = 0.0;
    if (xx > 0.0) {                                                                        // XX == 0: b_J = 0
      b1 = ((v[0] - zb * v[1]) + xx * b0) / (xx + tr.lam);                                 // :1472
      d = b1 - b0;
    }
    if (d != 0.0)
      for (int64_t r = tid; r < n; r += T) if (m[r]) e[r] = fma(-(z[r] - zb), d, e[r]);    // :1473
    if (tid == 0) { b[J] = b1; dlt[J] = d; }   // (b[J] is read again in a later sweep only: another launch)
  }
  if (LDS) for (int64_t r = tid; r < n; r += T) eg[r] = e[r];
  if (tid == 0) {   // thread 0 wrote b and dlt itself
    double d2 = 0.0, bb = 0.0, tb = 0.0;
    for (int64_t j = 0; j < q; ++j) { const double dv = dlt[j], bv = b[j]; d2 = fma(dv, dv, d2); bb = fma(bv, bv, bb); tb = fma(tilde[j], bv, tb); }
    double *leg = A.leg + (size_t)t * UVB2_NLEG;
    leg[0] = d2; leg[1] = bb; leg[2] = tb;
  }
}

}  // namespace bwgr
