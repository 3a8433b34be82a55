// bwgr_amd: the device work PEGSX (src/RcppEigenX20251203.cpp:197-573) adds to the PEGS / PEGSZ engine -- a fixed design X (n x f fp64,
// f <= PEGSX_MAXF) fitted beside the random effects.  The legs of a sweep are mrr.hip.h's and pegs.hip.h's as they stand; the k x k tail is
// pegs_tail.h.  Here:
//
//   k_pegsx_fixed      per sweep, after the last effect (:502-509): per trait d = (M'M)^+ M'e, b += d, e = (e - M d) o w, M = w o X.
//                      One workgroup per trait (the traits are independent here), nothing returns to the host.
//   k_pegsx_trace_*    once per call: for every column z_j of an effect and every missingness pattern g the f-vector v = M_g'z_j and the
//                      quadratic form v'A_g v, A_g = (M_g'M_g)^+, summed over j (:292-323 without the n-vectors the reference forms): the
//                      host takes the sum off sum_j ZZ_jt to get TrZSZ_t.  One for int8 panels in the slab layout, one for dense effects.
//
// X lives on the device once, unmasked (n x f, stride n); a pattern's mask is its bit of the row word zb, so traits that share a pattern
// share the work and no masked copy of X is made.  E is the engine's [trait][ld] array, zero on unobserved rows.  Every sum runs in a fixed
// order (lanes by shuffle, waves and workgroups in order), so two runs agree bit for bit.  The f-vectors live in LDS: no register array is
// sized by f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mrr.hip.h"

namespace bwgr {

static constexpr int PEGSX_MAXF = 256;      // columns of X at most (BWGR_PEGSX_MAXF)
static constexpr int PEGSX_TMAX = 1024;     // threads of k_pegsx_fixed at most (16 waves)
static constexpr int PEGSX_JC = 4;          // columns of an effect a wave of the trace kernels carries at once
static constexpr int PEGSX_FC = 4;          // columns of X per register tile of the trace kernels
static constexpr int PEGSX_TRACE_WG = 1024; // workgroups of the trace kernels at most (= partials per pattern), four waves each

struct PegsxFixedArgs {
  const double *X; int64_t n, ld; int f;
  const uint32_t *zt; double *e;
  const double *iXX;      // [pattern][f][f]
  double *b;              // [f][k], added to
};
__host__ __device__ inline size_t pegsx_fixed_lds(int f) { return sizeof(double) * 2 * (size_t)f; }
__global__ __launch_bounds__(PEGSX_TMAX) void k_pegsx_fixed(const PegsxFixedArgs A, const MrrConst c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *rhs = reinterpret_cast<double *>(smem), *d = rhs + A.f;
  const int t = blockIdx.x, f = A.f, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwv = blockDim.x >> 6;
  double *et = A.e + (size_t)t * A.ld;
  // phase 1: rhs_c = X_c'e_t (e is 0 on unobserved rows), one wave per column
  for (int col = wave; col < f; col += nwv) {
    const double *xc = A.X + (size_t)col * (size_t)A.n;
    double s = 0.0;
    for (int64_t r = lane; r < A.n; r += 64) s = fma(xc[r], et[r], s);
    s = mrr_wave_sum(s);
    if (lane == 0) rhs[col] = s;
  }
  __syncthreads();
  // phase 2: d = iXX_pattern(t) rhs (iXX is symmetric: row a is read as column a, lanes along it), b += d
  const double *iA = A.iXX + (size_t)c.pt[t] * f * f;
  for (int a = tid; a < f; a += blockDim.x) {
    double s = 0.0;
    for (int col = 0; col < f; ++col) s = fma(iA[(size_t)col * f + a], rhs[col], s);
    d[a] = s;
    A.b[(size_t)a * c.k + t] += s;
  }
  __syncthreads();
  // phase 3: e_rt -= sum_c X_rc d_c on the observed rows
  for (int64_t r = tid; r < A.n; r += blockDim.x) {
    if (!((A.zt[r] >> t) & 1u)) continue;
    double s = 0.0;
    for (int col = 0; col < f; ++col) s = fma(A.X[(size_t)col * (size_t)A.n + r], d[col], s);
    et[r] -= s;
  }
}

// four consecutive rows r .. r + 3 (r a multiple of 4) of column j of an effect, as doubles
struct PegsxPanelCols {
  const int8_t *X; int R; int64_t p;     // the panel's slab layout; its padding rows are zero and r + 3 < ld
  __device__ __forceinline__ void load(int64_t j, int64_t r, int64_t, double z[4]) const {
    const int word = *reinterpret_cast<const int *>(X + mrr_xoff(r, j, R, p));
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = (double)(int)(int8_t)(word >> (8 * i));
  }
};
struct PegsxDenseCols {
  const double *Z;                       // n x q, stride n
  __device__ __forceinline__ void load(int64_t j, int64_t r, int64_t n, double z[4]) const {
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = r + i < n ? Z[(size_t)j * (size_t)n + (size_t)(r + i)] : 0.0;
  }
};

// part[workgroup][g] = sum over the workgroup's columns j of v'A_g v, v = M_g'z_j.  A wave carries PEGSX_JC columns at once; per pattern it
// walks X in tiles of PEGSX_FC columns (JC x FC sums in registers, a lane four rows per trip), leaves v in its LDS region and takes the
// quadratic forms from there with A_g read from global memory.  No workgroup barrier inside the column loop: the waves' trip counts differ.
__host__ __device__ inline size_t pegsx_trace_lds(int f) { return sizeof(double) * (size_t)(4 * PEGSX_JC * f + 4 * MRR_KMAX); }
template <class Cols>
__device__ __forceinline__ void pegsx_trace_body(const Cols Zc, int64_t m, const double *__restrict__ X, int64_t n, int64_t nrows, int f,
                                                 const uint32_t *__restrict__ zb, int npat, const double *__restrict__ iXX, double *__restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *v = reinterpret_cast<double *>(smem) + (size_t)wave * PEGSX_JC * f;          // [jc][f]
  double *tots = reinterpret_cast<double *>(smem) + (size_t)4 * PEGSX_JC * f, *tot = tots + wave * MRR_KMAX;   // [wave][pattern]
  if (lane < MRR_KMAX) tot[lane] = 0.0;
  const int64_t ngrp = (m + PEGSX_JC - 1) / PEGSX_JC, nwv = (int64_t)gridDim.x * 4;
  for (int64_t grp = (int64_t)blockIdx.x * 4 + wave; grp < ngrp; grp += nwv) {
    const int64_t j0 = grp * PEGSX_JC;
    for (int g = 0; g < npat; ++g) {
      for (int c0 = 0; c0 < f; c0 += PEGSX_FC) {
        double acc[PEGSX_JC][PEGSX_FC];
#pragma unroll
        for (int a = 0; a < PEGSX_JC; ++a)
#pragma unroll
          for (int b = 0; b < PEGSX_FC; ++b) acc[a][b] = 0.0;
        for (int64_t r = 4 * (int64_t)lane; r < nrows; r += 256) {
          const uint4 zw = *reinterpret_cast<const uint4 *>(zb + r);      // (zb has nrows words, a multiple of 4; those past n are 0)
          const uint32_t w[4] = {(zw.x >> g) & 1u, (zw.y >> g) & 1u, (zw.z >> g) & 1u, (zw.w >> g) & 1u};
          if (!(w[0] | w[1] | w[2] | w[3])) continue;
          double z[PEGSX_JC][4], x[PEGSX_FC][4];
#pragma unroll
          for (int a = 0; a < PEGSX_JC; ++a) {
            if (j0 + a < m) Zc.load(j0 + a, r, n, z[a]);
            else { z[a][0] = 0.0; z[a][1] = 0.0; z[a][2] = 0.0; z[a][3] = 0.0; }
          }
#pragma unroll
          for (int b = 0; b < PEGSX_FC; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) x[b][i] = (c0 + b < f && w[i] && r + i < n) ? X[(size_t)(c0 + b) * (size_t)n + (size_t)(r + i)] : 0.0;
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int a = 0; a < PEGSX_JC; ++a)
#pragma unroll
              for (int b = 0; b < PEGSX_FC; ++b) acc[a][b] = fma(z[a][i], x[b][i], acc[a][b]);
        }
#pragma unroll
        for (int a = 0; a < PEGSX_JC; ++a)
#pragma unroll
          for (int b = 0; b < PEGSX_FC; ++b) {
            const double s = mrr_wave_sum(acc[a][b]);
            if (lane == 0 && c0 + b < f) v[a * f + c0 + b] = s;
          }
      }
      mrr_wave_sync();
      const double *Ag = iXX + (size_t)g * f * f;
      double q = 0.0;
      for (int col = lane; col < f; col += 64) {
        double s[PEGSX_JC];
#pragma unroll
        for (int a = 0; a < PEGSX_JC; ++a) s[a] = 0.0;
        for (int c2 = 0; c2 < f; ++c2) {
          const double av = Ag[(size_t)c2 * f + col];                    // A_g is symmetric: row col read as column col
#pragma unroll
          for (int a = 0; a < PEGSX_JC; ++a) s[a] = fma(av, v[a * f + c2], s[a]);
        }
#pragma unroll
        for (int a = 0; a < PEGSX_JC; ++a) q = fma(v[a * f + col], s[a], q);
      }
      q = mrr_wave_sum(q);
      if (lane == 0) tot[g] += q;
      mrr_wave_sync();                                                   // (v is rewritten by the next pattern)
    }
  }
  __syncthreads();
  if (tid < npat) part[(size_t)blockIdx.x * npat + tid] = (tots[tid] + tots[MRR_KMAX + tid]) + (tots[2 * MRR_KMAX + tid] + tots[3 * MRR_KMAX + tid]);
}
__global__ __launch_bounds__(256) void k_pegsx_trace_panel(const int8_t *__restrict__ Xp, int R, int64_t p, int64_t ld, const double *__restrict__ X, int64_t n,
                                                           int f, const uint32_t *__restrict__ zb, int npat, const double *__restrict__ iXX,
                                                           double *__restrict__ part) {
  const PegsxPanelCols Zc = {Xp, R, p};
  pegsx_trace_body(Zc, p, X, n, ld, f, zb, npat, iXX, part);
}
__global__ __launch_bounds__(256) void k_pegsx_trace_dense(const double *__restrict__ Z, int64_t q, int64_t ld, const double *__restrict__ X, int64_t n, int f,
                                                           const uint32_t *__restrict__ zb, int npat, const double *__restrict__ iXX,
                                                           double *__restrict__ part) {
  const PegsxDenseCols Zc = {Z};
  pegsx_trace_body(Zc, q, X, n, ld, f, zb, npat, iXX, part);
}

}  // namespace bwgr
