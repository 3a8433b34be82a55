// bwgr_amd: the dense leg of PEGS / PEGSZ (src/RcppEigenX20251203.cpp:10-194, :576-808) -- a small real-valued design Z (n x q fp64, e.g.
// kernel principal components or environment covariates) swept for k correlated traits against the engine's residual.
//
// The panel legs of these fits are mrr.hip.h's launch train as it stands, in its uncentred mode; the k x k tail is pegs_tail.h.  Here:
//
//   k_pegs_dense_setup  once per call: XX_jt = sum_r z_rt Z_rj^2 (:43-45), XSX_jt = XX_jt / n_t - (sum_r z_rt Z_rj / n_t)^2 (:48-51) and
//                       tilde_jt = sum_r Z_rj y_rt (:66) for every column j and trait t, one wave per column
//   k_pegs_dense_leg    per sweep: the q columns in the sweep's order (:109-120), ONE workgroup -- the columns form a serial chain through
//                       the residual, and a design this small leaves nothing for a second workgroup to do that would repay a protocol between
//                       them.  Per column: the k dots Z_j'e_t, RHS_t = (Z_j'e_t + XX_jt b0_t) / ve_t, b1 = Linv_j RHS (the inverse k_mrr_linv
//                       made from this design's XX), e_rt -= z_rt Z_rj (b1_t - b0_t), and sum (delta b)^2.
//   k_pegs_zb, k_pegs_add   fitted values: hat += Z b, hat += a panel's X b
//
// E is the engine's [trait][ld] array in global memory, zero on unobserved rows: the next panel pass reads it as stored.  Every thread owns
// the same rows in every column, and every sum runs in a fixed order (lanes by shuffle, waves in order), so two runs agree bit for bit.
// The per-column values (XX, Linv, b) stay in global memory: q is not capped by LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mrr.hip.h"

namespace bwgr {

static constexpr int PEGS_TMAX = 1024;   // threads of k_pegs_dense_leg at most (16 waves)

__global__ __launch_bounds__(256) void k_pegs_dense_setup(const double *__restrict__ Z, int64_t n, int64_t q, int64_t ld, const uint32_t *__restrict__ zt,
                                                          const double *__restrict__ y, const MrrConst c, double *__restrict__ XX,
                                                          double *__restrict__ XSX, double *__restrict__ tilde) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < q; j += nw) {
    double sz[MRR_KMAX], sq[MRR_KMAX], xy[MRR_KMAX];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) { sz[t] = 0.0; sq[t] = 0.0; xy[t] = 0.0; }
    const double *zc = Z + (size_t)j * (size_t)n;
    for (int64_t r = lane; r < n; r += 64) {
      const double v = zc[r];
      const uint32_t z = zt[r];
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t)
        if (t < c.k) {
          if ((z >> t) & 1u) { sz[t] += v; sq[t] = fma(v, v, sq[t]); }
          xy[t] = fma(v, y[(size_t)t * ld + r], xy[t]);
        }
    }
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) {
      if (t >= c.k) continue;
      const double s = mrr_wave_sum(sz[t]), qq = mrr_wave_sum(sq[t]), xyt = mrr_wave_sum(xy[t]);
      if (lane == 0) {
        const double nt = c.nt[t];
        XX[j * c.k + t] = qq;
        XSX[j * c.k + t] = qq / nt - (s / nt) * (s / nt);
        tilde[j * c.k + t] = xyt;
      }
    }
  }
}

struct PegsLegArgs {
  const double *Z; int64_t n, ld; int q;
  const uint32_t *zt; double *e;
  const int32_t *order; const double *XX, *Linv;
  double *b, *db2;          // db2[t] = this sweep's sum_j (delta b_jt)^2 (written, not added to)
};
__host__ __device__ inline size_t pegs_leg_lds(int threads) { return sizeof(double) * (size_t)((threads / 64) * MRR_KMAX + 2 * MRR_KMAX); }
__global__ __launch_bounds__(PEGS_TMAX) void k_pegs_dense_leg(const PegsLegArgs A, const MrrConst c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = c.k, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwv = blockDim.x >> 6;
  double *red = reinterpret_cast<double *>(smem);          // [wave][16]
  double *rhs = red + nwv * MRR_KMAX, *dbl = rhs + MRR_KMAX;
  double acc2 = 0.0;
  for (int jj = 0; jj < A.q; ++jj) {
    const int J = A.order[jj];
    const double *zc = A.Z + (size_t)J * (size_t)A.n;
    double acc[MRR_KMAX];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
    for (int64_t r = tid; r < A.n; r += blockDim.x) {
      const double v = zc[r];
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(v, A.e[(size_t)t * A.ld + r], acc[t]);   // (e is 0 where z is)
    }
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t)
      if (t < k) { const double s = mrr_wave_sum(acc[t]); if (lane == 0) red[wave * MRR_KMAX + t] = s; }
    __syncthreads();
    if (wave == 0) {
      double b0 = 0.0;
      if (lane < k) {
        double s = 0.0;
        for (int w = 0; w < nwv; ++w) s += red[w * MRR_KMAX + lane];
        b0 = A.b[(size_t)J * k + lane];
        rhs[lane] = (s + A.XX[(size_t)J * k + lane] * b0) * c.iVe[lane];
      }
      mrr_wave_sync();
      if (lane < k) {
        double b1 = 0.0;
        for (int s = 0; s < k; ++s) b1 = fma(A.Linv[((size_t)J * k + lane) * k + s], rhs[s], b1);
        const double d = b1 - b0;
        dbl[lane] = d;
        acc2 = fma(d, d, acc2);
        A.b[(size_t)J * k + lane] = b1;
      }
    }
    __syncthreads();
    for (int64_t r = tid; r < A.n; r += blockDim.x) {
      const double v = zc[r];
      const uint32_t z = A.zt[r];
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t)
        if (t < k && ((z >> t) & 1u)) A.e[(size_t)t * A.ld + r] = fma(-v, dbl[t], A.e[(size_t)t * A.ld + r]);
    }
    // (red is written again only after this column's reads of it, which precede the barrier above; dbl after the next column's first barrier)
  }
  if (wave == 0 && lane < k) A.db2[lane] = acc2;
}

// hat[t][r] += sum_j Z_rj b_jt (hat: k columns of stride n)
__global__ __launch_bounds__(256) void k_pegs_zb(const double *__restrict__ Z, int64_t n, int64_t q, int k, const double *__restrict__ b, double *__restrict__ hat) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double acc[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
  for (int64_t j = 0; j < q; ++j) {
    const double v = Z[(size_t)j * (size_t)n + r];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(v, b[j * k + t], acc[t]);
  }
  for (int t = 0; t < k; ++t) hat[(size_t)t * n + r] += acc[t];
}
__global__ void k_pegs_add(double *__restrict__ hat, const double *__restrict__ part, int64_t count) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) hat[i] += part[i];
}

}  // namespace bwgr
