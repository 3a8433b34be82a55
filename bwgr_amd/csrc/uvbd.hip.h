// bwgr_amd: the per-trait ridge engine on a small dense real-valued design (bwgr_uvbeta_dense), and the standalone X B on the int8 panel
// (bwgr_panel_xb) -- the second stage and the products of XSEMF / ZSEMF / YSEMF (src/RcppEigen20230423.cpp:1756-1769, :1819-1874).
//
// k_uvbd_fit: the solvers of uvb.hip.h (solver1x :1410-1443, solver1xF :1613-1646, xsolver1xF :1721-1743, zsolver1xF :1771-1804) on a design
// Z of n x q doubles with q small (a few dozen latent columns).  One workgroup per trait runs the trait's whole fit in one launch: set-up,
// every sweep, the tails and the stopping test; the traits do not couple, so the k fits run side by side with no host round trip.
//   rows      thread tid owns the rows r = tid, tid + T, ... in every loop of the kernel (set-up, dot, axpy, tails), so a row of e is only ever
//             touched by its own thread: e needs no barrier of its own, in LDS (LDS = true) or in the trait's global workspace (LDS = false)
//   mask      m[r] = 1 on the trait's observed rows; y and e are 0 elsewhere, so sums of z e, e and z y over all rows are the masked sums
//             (Z is finite: the host refuses anything else); only sum z, sum (z - zbar)^2 and the axpy read the mask
//   step J    q = sum_r z_rJ e_r - zbar_J sum_r e_r (the centred dot of the e actually stored, as uvb.hip.h carries it; no centred copy of Z);
//             b1 = (q + XX_J b0) / (XX_J + lambda) where XX_J > thr, else 0;  e_r -= (z_rJ - zbar_J)(b1 - b0) on observed rows
//   sums      uvbd_sum: each wave's shuffle tree, then the waves' partials in wave order, added by every thread alike -- one barrier per sum,
//             a fixed order, and every thread holds the same bits, so the scalar recurrence (b1, lambda, cnv, the stopping test) is computed
//             redundantly by all threads without a broadcast.  Two runs give the same bits.
// Per-column values (zbar, XX, tilde) live in the trait's slice of a global array and b in the output array: thread 0 writes them, every
// thread reads them after a later barrier (__syncthreads orders global memory within the workgroup).
//
// k_pxb / k_pxb_finish: out = X B for every row of the raw int8 panel, fp64.  The markers are split into chunks over workgroups; a thread
// carries four consecutive rows (one 32-bit load per marker) and 16 traits, the chunk's B tile is staged in LDS; the chunks' partials are
// added in chunk order.
#pragma once
#include "mrr.hip.h"

namespace bwgr {

static constexpr int UVBD_TMAX = 1024;                       // threads per workgroup at most
static constexpr int UVBD_NRED = 3;                          // values one uvbd_sum call reduces at most
static constexpr size_t UVBD_LDS_FIXED = sizeof(double) * 2 * UVBD_NRED * (UVBD_TMAX / 64);   // the sums' scratch, two alternating sets
static constexpr size_t UVBD_LDS_MAX = 160 * 1024;

struct UvbdTrait { double nt, mu, vy; };                     // observed rows; mean of Y over them (:1413); y'y / (nt - 1) (:1419)
// res[t][UVBD_NRES]: mu, ve, vb, cnv, its
static constexpr int UVBD_NRES = 5;

struct UvbdArgs {
  const double *Z; int64_t n, q;      // n x q, column-major, leading dimension n
  const double *y;                    // [k][n] centred, 0 on unobserved rows
  const uint8_t *m;                   // [k][n]
  const UvbdTrait *tr;
  const int32_t *order;               // [maxit][q]
  int variant, maxit; double logtol, df0, thr;
  double *cols;                       // [k][3][q]: zbar, XX, tilde
  double *e_ws;                       // [k][n] when e does not fit LDS
  double *b;                          // [q x k]
  double *res;                        // [k][UVBD_NRES]
};

// v[i] = the sum of v[i] over the workgroup, in every thread, i < N <= UVBD_NRED.  red: the two sets of scratch; flip alternates them, so that
// a call's writes cannot reach a set that a slower thread still reads (it last read that set two calls ago, before the previous barrier).
template <int N> __device__ __forceinline__ void uvbd_sum(double (&v)[N], double *red, int &flip) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  double *set = red + flip * (UVBD_NRED * (UVBD_TMAX / 64));
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const double s = mrr_wave_sum(v[i]);
    if (lane == 0) set[i * (UVBD_TMAX / 64) + w] = s;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = 0.0;
    for (int x = 0; x < nw; ++x) s += set[i * (UVBD_TMAX / 64) + x];
    v[i] = s;
  }
  flip ^= 1;
}

template <bool LDS> __global__ __launch_bounds__(UVBD_TMAX) void k_uvbd_fit(const UvbdArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *red = reinterpret_cast<double *>(smem);
  const int t = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int64_t n = A.n, q = A.q;
  const UvbdTrait tr = A.tr[t];
  double *res = A.res + (size_t)t * UVBD_NRES;
  if (tr.nt == 0.0) {   // no observed row: a zero column (the host zeroed b), its = 0 (:1510, :1713, :1811)
    if (tid == 0) { res[0] = 0.0; res[1] = NAN; res[2] = NAN; res[3] = NAN; res[4] = 0.0; }
    return;
  }
  double *e = LDS ? reinterpret_cast<double *>(smem + UVBD_LDS_FIXED) : A.e_ws + (size_t)t * n;
  const double *y = A.y + (size_t)t * n;
  const uint8_t *m = A.m + (size_t)t * n;
  double *zbar = A.cols + (size_t)t * 3 * q, *XX = zbar + q, *tilde = XX + q;
  double *b = A.b + (size_t)t * q;
  int flip = 0;
  // ---- set-up (:1415-1423): tilde on the raw columns, the trait's own column means, XX of the centred columns ----
  for (int64_t j = 0; j < q; ++j) {
    const double *z = A.Z + (size_t)j * n;
    double v[2] = {0.0, 0.0};
    for (int64_t r = tid; r < n; r += T) { const double zv = z[r]; if (m[r]) v[0] += zv; v[1] = fma(zv, y[r], v[1]); }
    uvbd_sum<2>(v, red, flip);
    const double zb = v[0] / tr.nt;
    double w[1] = {0.0};
    for (int64_t r = tid; r < n; r += T) if (m[r]) { const double c = z[r] - zb; w[0] = fma(c, c, w[0]); }
    uvbd_sum<1>(w, red, flip);
    if (tid == 0) { zbar[j] = zb; XX[j] = w[0]; tilde[j] = v[1]; }
  }
  for (int64_t r = tid; r < n; r += T) e[r] = y[r];                                  // :1422
  __syncthreads();
  double trx[1] = {0.0};
  for (int64_t j = tid; j < q; j += T) trx[0] += XX[j];
  uvbd_sum<1>(trx, red, flip);
  const double TrXSX = trx[0], MSx = TrXSX / (tr.nt - 1.0);                          // :1418-1419
  double mu = tr.mu, ve = tr.vy * 0.5, vb = (tr.vy * 0.5) / MSx, lam = ve / vb;      // :1420, :1423
  const double ve0 = ve * A.df0, vb0 = vb * A.df0;
  if (A.variant == BWGR_UVB_X) { lam = TrXSX / (double)q; ve = NAN; vb = NAN; }      // lambda = XX.mean(), :1730
  double cnv = NAN;
  int its = 0;
  // ---- sweeps ----
  while (its < A.maxit) {
    const int32_t *ord = A.order + (size_t)its * q;
    double acc2 = 0.0;
    for (int64_t s = 0; s < q; ++s) {
      const int J = ord[s];
      const double *z = A.Z + (size_t)J * n;
      const double xx = XX[J], zb = zbar[J], b0 = b[J];
      double v[2] = {0.0, 0.0};
      for (int64_t r = tid; r < n; r += T) { const double ev = e[r]; v[0] = fma(z[r], ev, v[0]); v[1] += ev; }
      uvbd_sum<2>(v, red, flip);
      double b1 = 0.0, d = 0.0;
      if (xx > A.thr) {                                                              // :1633-1635 (F); XX == 0 elsewhere: b_J = 0
        b1 = ((v[0] - zb * v[1]) + xx * b0) / (xx + lam);                            // :1431
        d = b1 - b0;
      }
      if (d != 0.0)
        for (int64_t r = tid; r < n; r += T) if (m[r]) e[r] = fma(-(z[r] - zb), d, e[r]);   // :1432
      if (tid == 0) b[J] = b1;
      acc2 = fma(d, d, acc2);
    }
    // the tail (:1433-1441, :1636-1644, :1739-1741, :1794-1801)
    double se[1] = {0.0};
    for (int64_t r = tid; r < n; r += T) se[0] += e[r];
    uvbd_sum<1>(se, red, flip);
    const double mu0 = se[0] / tr.nt;
    mu += mu0;
    double v[2] = {0.0, 0.0};
    for (int64_t r = tid; r < n; r += T)
      if (m[r]) { const double ev = e[r] - mu0; e[r] = ev; v[0] = fma(ev, y[r], v[0]); v[1] = fma(ev, ev, v[1]); }
    uvbd_sum<2>(v, red, flip);   // (its barrier also orders thread 0's b before the reads below)
    double c[2] = {0.0, 0.0};
    for (int64_t j = tid; j < q; j += T) { const double bv = b[j]; c[0] = fma(bv, bv, c[0]); c[1] = fma(tilde[j], bv, c[1]); }
    uvbd_sum<2>(c, red, flip);
    if (A.variant == BWGR_UVB_D || A.variant == BWGR_UVB_F) {
      ve = (v[0] + v[1] + ve0) / (2.0 * tr.nt - 1.0 + A.df0);                        // :1434-1436
      vb = (c[0] + c[1] + vb0) / (TrXSX + (double)q + A.df0);                        // :1437-1439
      lam = ve / vb;
    } else if (A.variant == BWGR_UVB_Z) {
      ve = (v[0] + ve0) / (tr.nt + A.df0);                                           // :1795-1796
      vb = (c[1] + vb0) / (TrXSX + A.df0);                                           // :1797-1798
      lam = ve / vb;
    }
    cnv = log10(acc2);                                                               // :1440
    ++its;
    if (cnv < A.logtol || isnan(cnv)) break;                                         // :1441 (its == maxit ends the loop)
  }
  if (tid == 0) { res[0] = mu; res[1] = ve; res[2] = vb; res[3] = cnv; res[4] = (double)its; }
}

// ---- X B on the raw panel ----
static constexpr int PXB_TS = 16;      // traits per workgroup
static constexpr int PXB_MT = 128;     // markers of B staged at a time
static constexpr int PXB_ROWS = 1024;  // rows per workgroup: 256 threads, four consecutive rows each
// part[(c * k + t) * n + r] = sum over chunk c's markers of x_rj B_jt     grid (row tiles, chunks, trait slices)
__global__ __launch_bounds__(256) void k_pxb(const int8_t *__restrict__ X, int R, int64_t p, int64_t ld, int64_t n, const double *__restrict__ B, int k,
                                             int64_t chunk, double *__restrict__ part) {
  __shared__ __attribute__((aligned(16))) double bs[PXB_MT * PXB_TS];
  const int tid = threadIdx.x, t0 = blockIdx.z * PXB_TS;
  const int64_t r0 = (int64_t)blockIdx.x * PXB_ROWS + 4 * tid;     // (R is a multiple of 128: the four rows share a slab)
  const int64_t c0 = (int64_t)blockIdx.y * chunk, c1 = c0 + chunk < p ? c0 + chunk : p;
  const bool rows = r0 < ld;                                       // (rows n .. ld - 1 of the panel are stored zeros)
  const int64_t w = rows ? r0 / R : 0;
  const int8_t *xp = X + (size_t)(w * p) * R + (rows ? r0 - w * R : 0);
  double acc[4][PXB_TS];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int i = 0; i < PXB_TS; ++i) acc[a][i] = 0.0;
  for (int64_t j0 = c0; j0 < c1; j0 += PXB_MT) {
    const int mlen = (int)(c1 - j0 < PXB_MT ? c1 - j0 : PXB_MT);
    __syncthreads();
    for (int o = tid; o < PXB_MT * PXB_TS; o += 256) {
      const int i = o / PXB_MT, jm = o - i * PXB_MT;
      bs[jm * PXB_TS + i] = (jm < mlen && t0 + i < k) ? B[(size_t)(t0 + i) * p + j0 + jm] : 0.0;
    }
    __syncthreads();
    if (!rows) continue;
#pragma unroll 2
    for (int jm = 0; jm < mlen; ++jm) {
      const int word = *reinterpret_cast<const int *>(xp + (size_t)(j0 + jm) * R);
      const double x0 = (double)(int)(int8_t)word, x1 = (double)(int)(int8_t)(word >> 8), x2 = (double)(int)(int8_t)(word >> 16), x3 = (double)(word >> 24);
      const double *bp = bs + jm * PXB_TS;
#pragma unroll
      for (int i = 0; i < PXB_TS; ++i) {
        const double bv = bp[i];
        acc[0][i] = fma(x0, bv, acc[0][i]); acc[1][i] = fma(x1, bv, acc[1][i]); acc[2][i] = fma(x2, bv, acc[2][i]); acc[3][i] = fma(x3, bv, acc[3][i]);
      }
    }
  }
  if (!rows) return;
#pragma unroll
  for (int i = 0; i < PXB_TS; ++i) {
    if (t0 + i >= k) continue;
    double *o = part + ((size_t)blockIdx.y * k + t0 + i) * n;
#pragma unroll
    for (int a = 0; a < 4; ++a) if (r0 + a < n) o[r0 + a] = acc[a][i];
  }
}
// out[i] = sum_c part[c][i] in chunk order, i over the n x k result
__global__ void k_pxb_finish(const double *__restrict__ part, int64_t nk, int chunks, double *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nk; i += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * nk + i];
    out[i] = s;
  }
}

}  // namespace bwgr
