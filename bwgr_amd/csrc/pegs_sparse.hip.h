// bwgr_amd: the sparse leg of the multi-trait fits (PEGS_sparse, PEGSZ_sparse src/RcppEigenX20251203.cpp:811-1007, :1010-1250, and sparse
// effects in PEGS / PEGSZ / PEGSX lists) -- a column-compressed design S (n x q; the incidence matrix of environments, blocks or
// genotype-by-environment cells) swept for k correlated traits against the engine's residual.  The host side (validation, the row-disjointness
// test, the row-major copy) is csc.h; the k x k tail is pegs_tail.h.  Here:
//
//   k_pegs_sparse_setup         once per call: XX_jt = sum z_rt v^2 (:846-853), XSX_jt = XX_jt / n_t - (sum z_rt v / n_t)^2 (:856-860) and
//                               tilde_jt = sum v y_rt (:875) over the stored entries (r, v) of column j, one wave per column
//   pegs_sparse_column          the update of ONE column by ONE wave (:918-937), shared by both legs: the k dots sum v e_rt (lanes stride the
//                               column's entries, mrr_wave_sum), RHS_t = (dot_t + XX_jt b0_t) / ve_t, b1 = Linv_j RHS (the inverse k_mrr_linv
//                               made from this effect's XX), e_rt -= z_rt v (b1_t - b0_t) on the column's rows, (b1_t - b0_t)^2 into d2[j][t]
//   k_pegs_sparse_leg           the serial leg: one wave walks the q columns in the sweep's order; between two columns the wave's stores are
//                               made visible to its own later loads (another lane may read the row), a memory round trip per column
//   k_pegs_sparse_leg_disjoint  where no row occurs in two columns (csc_row_disjoint): the columns touch disjoint rows of e, so the sweep
//                               does not depend on their order and a grid of waves takes one column each, all at once, in trips of
//                               gridDim.x * 4 columns.  Each column reads and writes only its own rows through the same routine on the same
//                               lanes: the bits of the serial leg.
//   db2                         k_mrr_tilde (mode 2) / k_mrr_finish over d2 in column-index order, for either leg
//   k_pegs_sparse_hat           fitted values: hat += S b through the row-major copy, one thread per row, its entries in column order
//   k_pegsx_trace_sparse        PEGSX's sum_j v'A_g v with v = M_g'z_j over the column's entries; partials laid out as k_pegsx_trace_dense's
//
// E is the engine's [trait][ld] array in global memory, zero on unobserved rows, zt the row word of observed traits, as in k_pegs_dense_leg.
// Every sum runs in a fixed order (lanes by shuffle, entries by stride), there is no atomic, and two runs agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mrr.hip.h"
#include "pegsx.hip.h"

namespace bwgr {

static constexpr int PEGS_SPARSE_WG = 1024;   // workgroups of the disjoint leg at most, four waves (= columns) each per trip

__global__ __launch_bounds__(256) void k_pegs_sparse_setup(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx,
                                                           const double *__restrict__ val, int64_t q, int64_t ld, const uint32_t *__restrict__ zt,
                                                           const double *__restrict__ y, const MrrConst c, double *__restrict__ XX,
                                                           double *__restrict__ XSX, double *__restrict__ tilde) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < q; j += nw) {
    double sz[MRR_KMAX], sq[MRR_KMAX], xy[MRR_KMAX];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) { sz[t] = 0.0; sq[t] = 0.0; xy[t] = 0.0; }
    const int64_t i1 = colptr[j + 1];
    for (int64_t i = colptr[j] + lane; i < i1; i += 64) {
      const double v = val[i];
      const int64_t r = rowidx[i];
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

struct PegsSparseArgs {
  const int64_t *colptr; const int32_t *rowidx; const double *val;
  int64_t ld, q;
  const uint32_t *zt; double *e;
  const int32_t *order; const double *XX, *Linv;
  double *b, *d2;           // d2[j * k + t] = this sweep's (delta b_jt)^2 (written, not added to)
};

// One column, one wave (every lane of it calls this, with the same J).  Lane t < k carries trait t's dot, RHS, b0 and b1; the k values
// travel between the lanes by shuffle, so the routine needs no LDS.
__device__ __forceinline__ void pegs_sparse_column(const PegsSparseArgs &A, const MrrConst &c, int64_t J, int lane) {
  const int k = c.k;
  const int64_t i0 = A.colptr[J], i1 = A.colptr[J + 1];
  double acc[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
  for (int64_t i = i0 + lane; i < i1; i += 64) {
    const double v = A.val[i];
    const int64_t r = A.rowidx[i];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(v, A.e[(size_t)t * A.ld + r], acc[t]);   // (e is 0 where z is)
  }
  double dot = 0.0;
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t)
    if (t < k) { const double s = __shfl(mrr_wave_sum(acc[t]), 0, 64); if (lane == t) dot = s; }
  double b0 = 0.0, rhs = 0.0;
  if (lane < k) {
    b0 = A.b[(size_t)J * k + lane];
    rhs = (dot + A.XX[(size_t)J * k + lane] * b0) * c.iVe[lane];
  }
  double b1 = 0.0;
  for (int s = 0; s < k; ++s) {
    const double rs = __shfl(rhs, s, 64);
    if (lane < k) b1 = fma(A.Linv[((size_t)J * k + lane) * k + s], rs, b1);
  }
  const double d = b1 - b0;
  if (lane < k) {
    A.b[(size_t)J * k + lane] = b1;
    A.d2[(size_t)J * k + lane] = d * d;
  }
  double dl[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) dl[t] = t < k ? __shfl(d, t, 64) : 0.0;
  for (int64_t i = i0 + lane; i < i1; i += 64) {
    const double v = A.val[i];
    const int64_t r = A.rowidx[i];
    const uint32_t z = A.zt[r];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t)
      if (t < k && ((z >> t) & 1u)) A.e[(size_t)t * A.ld + r] = fma(-v, dl[t], A.e[(size_t)t * A.ld + r]);
  }
}

// the serial leg: ONE wave, the columns in the sweep's order
__global__ __launch_bounds__(64) void k_pegs_sparse_leg(const PegsSparseArgs A, const MrrConst c) {
  const int lane = threadIdx.x & 63;
  for (int64_t jj = 0; jj < A.q; ++jj) {
    pegs_sparse_column(A, c, (int64_t)A.order[jj], lane);
    __threadfence();                     // the next column may read, on another lane, a row this one wrote
    __builtin_amdgcn_wave_barrier();
  }
}

// the disjoint leg: one column per wave, every column's rows its own
__global__ __launch_bounds__(256) void k_pegs_sparse_leg_disjoint(const PegsSparseArgs A, const MrrConst c) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t J = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); J < A.q; J += nw) pegs_sparse_column(A, c, J, lane);
}

// hat[t][r] += sum over row r's entries (j, v) of v b_jt (hat: k columns of stride n), every row, its entries in column order
__global__ __launch_bounds__(256) void k_pegs_sparse_hat(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ colidx, const double *__restrict__ rval,
                                                         int64_t n, int k, const double *__restrict__ b, double *__restrict__ hat) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double acc[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
  const int64_t i1 = rowptr[r + 1];
  for (int64_t i = rowptr[r]; i < i1; ++i) {
    const double v = rval[i];
    const int64_t j = colidx[i];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(v, b[j * k + t], acc[t]);
  }
  for (int t = 0; t < k; ++t) hat[(size_t)t * n + r] += acc[t];
}

// part[workgroup][g] = sum over the workgroup's columns j of v'A_g v, v = M_g'z_j (k_pegsx_trace_dense's partials; its LDS size too, of
// which a wave uses the first f doubles of its region).  One column per wave and trip: lane c carries v_c, c + 64, ... and walks the
// column's entries in order, so v needs no reduction; the quadratic form is pegsx_trace_body's.
__global__ __launch_bounds__(256) void k_pegsx_trace_sparse(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowidx, const double *__restrict__ val,
                                                            int64_t q, const double *__restrict__ X, int64_t n, int f, const uint32_t *__restrict__ zb,
                                                            int npat, const double *__restrict__ iXX, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *v = reinterpret_cast<double *>(smem) + (size_t)wave * PEGSX_JC * f;          // [f]
  double *tots = reinterpret_cast<double *>(smem) + (size_t)4 * PEGSX_JC * f, *tot = tots + wave * MRR_KMAX;   // [wave][pattern]
  if (lane < MRR_KMAX) tot[lane] = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * 4 + wave; j < q; j += (int64_t)gridDim.x * 4) {
    const int64_t i0 = colptr[j], i1 = colptr[j + 1];
    for (int g = 0; g < npat; ++g) {
      for (int col = lane; col < f; col += 64) {
        double s = 0.0;
        for (int64_t i = i0; i < i1; ++i) {
          const int64_t r = rowidx[i];
          if ((zb[r] >> g) & 1u) s = fma(val[i], X[(size_t)col * (size_t)n + (size_t)r], s);
        }
        v[col] = s;
      }
      mrr_wave_sync();
      const double *Ag = iXX + (size_t)g * f * f;
      double qf = 0.0;
      for (int col = lane; col < f; col += 64) {
        double s = 0.0;
        for (int c2 = 0; c2 < f; ++c2) s = fma(Ag[(size_t)c2 * f + col], v[c2], s);   // A_g is symmetric: row col read as column col
        qf = fma(v[col], s, qf);
      }
      qf = mrr_wave_sum(qf);
      if (lane == 0) tot[g] += qf;
      mrr_wave_sync();                                                   // (v is rewritten by the next pattern)
    }
  }
  __syncthreads();
  if (tid < npat) part[(size_t)blockIdx.x * npat + tid] = (tots[tid] + tots[MRR_KMAX + tid]) + (tots[2 * MRR_KMAX + tid] + tots[3 * MRR_KMAX + tid]);
}

}  // namespace bwgr
