// bwgr_amd: the multi-trait ridge engine of mrr.hip.h on a dense fp64 design -- mrr(Y, dense(X)), mkr(Y, K) = MRR3(Y, K2X(K))
// (R/mix.R:1275, src/RcppEigen20230423.cpp:318-700, :1942-1948).  DESIGN.md section 4.13.
//
// The launch train is mrr's: per-sweep block Grams, one pass over the rows per 64-column block, a serial solve on the reduced dots.  Only the
// kernels that read X differ.  The design is the engine's own n x r copy, column-major with a column stride of ld rows (ld a multiple of 128,
// the rows from n on are zero), centred ONCE and explicitly by its all-rows column means (:763-765), so everything after k_mrrd_centre runs
// in mrr's centre = 0 mode: xbar = 0, no Gram correction, no offset in the fitted values.
//
//   k_mrrd_centre  once per call: column mean over the n rows, x - mean into the engine's copy, zeros into its padding rows
//   k_mrrd_setup   once per call: per-pattern masked sums and squares, X'y -> XX, XSX, tilde (one wave per column)
//   k_mrrd_gram    per sweep: G_g = X_B' diag(z_g) X_B in fp64 for every 64-column block of the sweep's order and every pattern g
//   k_mrrd_pass    per block: E -= (X_B-1 dB_B-1) o Z for the rows of a tile, then the partial dots X_B' E of the next block
//   k_mrrd_solve   per block: k_mrr_solve's recurrence on an fp64 Gram, without the centring terms
//   k_mrrd_hat     fitted values X_c b + mu for every row
// k_mrr_linv, k_mrr_ey, k_mrr_tilde, k_mrr_finish and k_mrr_mu_shift serve unchanged.
//
// The columns of a block are read through the sweep's order array: a column of a column-major matrix is contiguous wherever it stands, so a
// gathered copy (the int8 train's k_permute_cols) would cost a read and a write of the whole design per sweep and buy nothing.
// Every sum has a fixed order (lanes by shuffle, rows ascending within a thread, partials in index order), and nothing is accumulated by
// atomics, so two runs give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mrr.hip.h"

namespace bwgr {

static constexpr int MRRD_GT = 32;   // rows per LDS tile of k_mrrd_gram
static constexpr int MRRD_GP = 66;   // doubles per row of that tile (16-byte aligned rows, and a stride that spreads the transposing writes)
static constexpr int MRRD_XP = 65;   // doubles per column of k_mrrd_pass's tile (conflict-free in both directions)

// ---- once per call: dst[:, j] = src[:, j] - mean(src[0..n, j]), zero on the rows n .. ld-1; one wave per column.  dst may be src (in place:
// every lane rewrites the elements it read) ----
__global__ __launch_bounds__(256) void k_mrrd_centre(const double *src, int64_t ldsrc, int64_t n, int64_t r, int64_t ld, double *dst) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < r; j += nw) {
    const double *s = src + (size_t)j * (size_t)ldsrc;
    double *d = dst + (size_t)j * (size_t)ld;
    double a = 0.0;
    for (int64_t i = lane; i < n; i += 64) a += s[i];
    const double m = __shfl(mrr_wave_sum(a), 0, 64) / (double)n;
    for (int64_t i = lane; i < ld; i += 64) d[i] = i < n ? s[i] - m : 0.0;
  }
}

// ---- once per call: the dense twin of k_mrr_setup_cols in its centre = 0 mode, one wave per column ----
// S_g(j) = sum_r z_rg x_rj and Q_g(j) = sum_r z_rg x_rj^2 per pattern; XX[j][t] = Q_pt(t) (:769-770), XSX[j][t] = XX/n_t - (S_pt(t)/n_t)^2
// (:774-776), tilde[j][t] = x_j'y_t (:806; y is zero on unobserved rows).  zb[r]: bit g = row r observed in pattern g.
__global__ __launch_bounds__(256) void k_mrrd_setup(const double *__restrict__ X, int64_t n, int64_t r, int64_t ld, const uint32_t *__restrict__ zb,
                                                    const double *__restrict__ y, const MrrConst c, double *__restrict__ XX, double *__restrict__ XSX,
                                                    double *__restrict__ tilde) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < r; j += nw) {
    double sg[MRR_KMAX], qg[MRR_KMAX], xy[MRR_KMAX];
#pragma unroll
    for (int g = 0; g < MRR_KMAX; ++g) { sg[g] = 0.0; qg[g] = 0.0; xy[g] = 0.0; }
    const double *xc = X + (size_t)j * (size_t)ld;
    for (int64_t i = lane; i < n; i += 64) {
      const double v = xc[i];
      const uint32_t z = zb[i];
#pragma unroll
      for (int g = 0; g < MRR_KMAX; ++g)
        if (g < c.npat && ((z >> g) & 1u)) { sg[g] += v; qg[g] = fma(v, v, qg[g]); }
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t)
        if (t < c.k) xy[t] = fma(v, y[(size_t)t * ld + i], xy[t]);
    }
    double sgs[MRR_KMAX], qgs[MRR_KMAX];
#pragma unroll
    for (int g = 0; g < MRR_KMAX; ++g) {
      sgs[g] = 0.0; qgs[g] = 0.0;
      if (g < c.npat) { sgs[g] = __shfl(mrr_wave_sum(sg[g]), 0, 64); qgs[g] = __shfl(mrr_wave_sum(qg[g]), 0, 64); }
    }
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) {
      const double xyt = (t < c.k) ? mrr_wave_sum(xy[t]) : 0.0;
      if (lane == 0 && t < c.k) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int g = 0; g < MRR_KMAX; ++g) if (g == c.pt[t]) { s = sgs[g]; q = qgs[g]; }
        const double nt = c.nt[t];
        XX[j * c.k + t] = q;
        XSX[j * c.k + t] = q / nt - (s / nt) * (s / nt);
        tilde[j * c.k + t] = xyt;
      }
    }
  }
}

// ---- per sweep: the block Gram matrices, one workgroup per (block b, pattern g) ----
// The rows go through LDS in tiles of MRRD_GT: xt[row][col] holds the block's 64 columns (zero past the design's edge), xm the same values
// with the pattern's unobserved rows zeroed.  Thread (ti, tj) of the 16 x 16 owns the 4 x 4 entries G(4ti.., 4tj..) and adds the rows in
// ascending order, so a sum's order depends on nothing but ld; G(i, j) and G(j, i) add the same products in the same order and agree bit
// for bit.  Out: G[(b * npat + g) * 4096 + i * 64 + j].
__global__ __launch_bounds__(256) void k_mrrd_gram(const double *__restrict__ X, int64_t ld, int64_t r, const int32_t *__restrict__ order,
                                                   const uint32_t *__restrict__ zb, int npat, double *__restrict__ G) {
  __shared__ __attribute__((aligned(16))) double xt[MRRD_GT * MRRD_GP];
  __shared__ __attribute__((aligned(16))) double xm[MRRD_GT * MRRD_GP];
  __shared__ int Jl[MRR_MB];
  const int b = blockIdx.x, g = blockIdx.y, tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
  const int64_t j0 = (int64_t)b * MRR_MB;
  if (tid < MRR_MB) Jl[tid] = j0 + tid < r ? order[j0 + tid] : -1;
  __syncthreads();
  double acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;
  const int rr = tid & (MRRD_GT - 1), cq = tid / MRRD_GT;   // 8 column groups
  for (int64_t r0 = 0; r0 < ld; r0 += MRRD_GT) {
    const bool on = ((zb[r0 + rr] >> g) & 1u) != 0;
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int J = Jl[cq + 8 * i];
      v[i] = J >= 0 ? X[(size_t)J * (size_t)ld + (size_t)(r0 + rr)] : 0.0;
    }
    __syncthreads();   // the previous tile is consumed
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      xt[rr * MRRD_GP + cq + 8 * i] = v[i];
      xm[rr * MRRD_GP + cq + 8 * i] = on ? v[i] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < MRRD_GT; ++q) {
      const double2 a0 = *reinterpret_cast<const double2 *>(xt + q * MRRD_GP + 4 * ti), a1 = *reinterpret_cast<const double2 *>(xt + q * MRRD_GP + 4 * ti + 2);
      const double2 b0 = *reinterpret_cast<const double2 *>(xm + q * MRRD_GP + 4 * tj), b1 = *reinterpret_cast<const double2 *>(xm + q * MRRD_GP + 4 * tj + 2);
      const double a[4] = {a0.x, a0.y, a1.x, a1.y}, bb[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fma(a[i], bb[j], acc[i][j]);
    }
  }
  double *out = G + ((size_t)b * npat + g) * (MRR_MB * MRR_MB);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<double4 *>(out + (size_t)(4 * ti + i) * MRR_MB + 4 * tj) = double4{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
}

// ---- per block: the residual update of block `prev` and the partial dots of block `next` in one pass over the rows ----
// The dense twin of k_mrr_pass: tiles of 64 rows, workgroup w takes tiles w, w + G, ...  For a tile:
//   update (prev >= 0): e_rt -= z_rt sum_j x_rj dB_jt                                                          -- :900-901
//   dots   (next >= 0): part[w][j][t] += sum_r x_rj e_rt over the tile
// E is [t][ld] fp64; the padding rows have z = 0 and x = 0 and stay 0.  zt[r]: bit t = row r observed for trait t.
struct MrrdPassArgs {
  const double *X; int64_t r, ld;
  const int32_t *order; const uint32_t *zt; double *e;
  const double *dB;     // [64][16]
  double *part;         // [G][64][16]
  int prev, next, k;
};
__global__ __launch_bounds__(256) void k_mrrd_pass(const MrrdPassArgs A) {
  __shared__ double xt[MRR_MB * MRRD_XP];      // [column][row]
  __shared__ double et[64 * MRR_KMAX];         // [row][t]
  __shared__ double dBl[MRR_MB * MRR_KMAX];
  __shared__ int Jp[MRR_MB], Jn[MRR_MB];
  const int tid = threadIdx.x, k = A.k;
  const int rr = tid & 63, tq = tid >> 6;
  const int64_t ntiles = A.ld / 64;
  if (tid < MRR_MB) {
    const int64_t jp = (int64_t)A.prev * MRR_MB + tid, jn = (int64_t)A.next * MRR_MB + tid;
    Jp[tid] = (A.prev >= 0 && jp < A.r) ? A.order[jp] : -1;
    Jn[tid] = (A.next >= 0 && jn < A.r) ? A.order[jn] : -1;
  }
  if (A.prev >= 0)
    for (int i = tid; i < MRR_MB * MRR_KMAX; i += 256) dBl[i] = A.dB[i];
  double dacc[4] = {0.0, 0.0, 0.0, 0.0};
  // a tile goes global -> registers -> LDS in two steps, so that the next block's tile is in flight while the update runs
  auto fetch_tile = [&](const int *Jl, int64_t r0, double (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int J = Jl[tq + 4 * i];
      v[i] = J >= 0 ? A.X[(size_t)J * (size_t)A.ld + (size_t)(r0 + rr)] : 0.0;
    }
  };
  auto store_tile = [&](const double (&v)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) xt[(tq + 4 * i) * MRRD_XP + rr] = v[i];
  };
  double xv[16];
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * 64, r = r0 + rr;
    __syncthreads();
    if (A.prev >= 0) {
      fetch_tile(Jp, r0, xv);
      store_tile(xv);
      __syncthreads();
      if (A.next >= 0) fetch_tile(Jn, r0, xv);
      const uint32_t z = A.zt[r];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = tq + 4 * i;
        if (t < k) {
          double s = 0.0;
          for (int jm = 0; jm < MRR_MB; ++jm) s = fma(xt[jm * MRRD_XP + rr], dBl[jm * MRR_KMAX + t], s);
          double ev = A.e[(size_t)t * A.ld + r];
          if ((z >> t) & 1u) ev -= s;
          A.e[(size_t)t * A.ld + r] = ev;
          et[rr * MRR_KMAX + t] = ev;
        }
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) et[rr * MRR_KMAX + t] = A.e[(size_t)t * A.ld + r]; }
      if (A.next >= 0) fetch_tile(Jn, r0, xv);
    }
    if (A.next < 0) continue;
    store_tile(xv);
    __syncthreads();
    const int jm = tid & 63;
    for (int row = 0; row < 64; ++row) {
      const double x = xt[jm * MRRD_XP + row];
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) dacc[i] = fma(x, et[row * MRR_KMAX + t], dacc[i]); }
    }
  }
  if (A.next < 0) return;
  double *pw = A.part + (size_t)blockIdx.x * MRR_MB * MRR_KMAX;
  const int jm = tid & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) pw[jm * MRR_KMAX + t] = dacc[i]; }
}

// ---- per block: the serial recurrence of the block's columns (:869-901) on an fp64 Gram ----
// k_mrr_solve without its centring terms (xbar = 0).  Phase 1 (256 threads): dc[j][t] = sum_w part[w][j][t], the dots x_J'e_t at the block's
// start; the block's Gram matrices (the first ngl patterns; the rest are read from global memory), the columns' inverses (linv_lds: when
// 64 k^2 doubles fit beside them), XX and b0 staged into LDS.  Phase 2 (wave 0 alone, no workgroup barriers), column j in order:
//   lanes t < k:  RHS_t = (dc[j][t] + XX_Jt b0_t) / ve_t;   b1 = Linv_J RHS;   dB_jt = b1_t - b0_t;   b[J] = b1
//   lanes l > j:  dc[l][t] -= G_pt(t)(j, l) dB_jt
// Afterwards dB goes out for the next pass, and sum_j dB_jt^2 is added to db2[t].
struct MrrdSolveArgs {
  const double *part; int G;
  const int32_t *order; int blk; int64_t r;
  const double *gram, *XX, *Linv;
  double *b, *dB, *db2;
  int ngl, linv_lds;
};
__host__ __device__ inline size_t mrrd_solve_lds(int ngl, int linv_doubles) {
  return sizeof(double) * ((size_t)ngl * MRR_MB * MRR_MB + (size_t)linv_doubles + (size_t)(MRR_MB * 17 + 3 * MRR_MB * MRR_KMAX + MRR_KMAX)) + 64 * 4;
}
__global__ __launch_bounds__(256) void k_mrrd_solve(const MrrdSolveArgs A, const MrrConst c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = c.k, npat = c.npat, ngl = A.ngl, tid = threadIdx.x;
  double *gl = reinterpret_cast<double *>(smem);
  double *linvl = gl + (size_t)ngl * MRR_MB * MRR_MB;                    // [64][k][k] when linv_lds
  double *dc = linvl + (A.linv_lds ? MRR_MB * k * k : 0);               // [64][17]
  double *xxl = dc + MRR_MB * 17, *b0l = xxl + MRR_MB * MRR_KMAX, *dbl = b0l + MRR_MB * MRR_KMAX, *rhs = dbl + MRR_MB * MRR_KMAX;
  int *Jl = reinterpret_cast<int *>(rhs + MRR_KMAX);
  const int64_t j0 = (int64_t)A.blk * MRR_MB;
  const int mB = (int)(A.r - j0 < MRR_MB ? A.r - j0 : MRR_MB);
  const double *gglob = A.gram + (size_t)A.blk * npat * MRR_MB * MRR_MB;
  if (tid < MRR_MB) Jl[tid] = tid < mB ? A.order[j0 + tid] : 0;
  {
    const double2 *src = reinterpret_cast<const double2 *>(gglob);
    double2 *dst = reinterpret_cast<double2 *>(gl);
    for (int i = tid; i < ngl * MRR_MB * MRR_MB / 2; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  for (int o = tid; o < MRR_MB * k; o += 256) {
    const int jm = o / k, t = o - jm * k;
    double s = 0.0;
    int w = 0;
    for (; w + 8 <= A.G; w += 8) {   // eight requests in flight; added in index order as before
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = A.part[((size_t)(w + i) * MRR_MB + jm) * MRR_KMAX + t];
#pragma unroll
      for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; w < A.G; ++w) s += A.part[((size_t)w * MRR_MB + jm) * MRR_KMAX + t];
    const int J = Jl[jm];
    dc[jm * 17 + t] = s;
    xxl[jm * MRR_KMAX + t] = jm < mB ? A.XX[(size_t)J * k + t] : 0.0;
    b0l[jm * MRR_KMAX + t] = jm < mB ? A.b[(size_t)J * k + t] : 0.0;
  }
  if (A.linv_lds)
    for (int i = tid; i < mB * k * k; i += 256) { const int jm = i / (k * k); linvl[i] = A.Linv[(size_t)Jl[jm] * k * k + (i - jm * k * k)]; }
  __syncthreads();
  if (tid >= 64) return;
  const int l = tid;
  double acc2 = 0.0;
  double lrow[MRR_KMAX];
#pragma unroll
  for (int s = 0; s < MRR_KMAX; ++s) lrow[s] = 0.0;
  if (!A.linv_lds && l < k && mB > 0) {
#pragma unroll
    for (int s = 0; s < MRR_KMAX; ++s) if (s < k) lrow[s] = A.Linv[((size_t)Jl[0] * k + l) * k + s];
  }
  for (int j = 0; j < mB; ++j) {
    if (l < k) rhs[l] = (dc[j * 17 + l] + xxl[j * MRR_KMAX + l] * b0l[j * MRR_KMAX + l]) * c.iVe[l];
    mrr_wave_sync();
    if (l < k) {
      double b1 = 0.0;
#pragma unroll
      for (int s = 0; s < MRR_KMAX; ++s) if (s < k) b1 = fma(A.linv_lds ? linvl[(j * k + l) * k + s] : lrow[s], rhs[s], b1);
      const double d = b1 - b0l[j * MRR_KMAX + l];
      dbl[j * MRR_KMAX + l] = d;
      acc2 = fma(d, d, acc2);
      b0l[j * MRR_KMAX + l] = b1;   // (b0 of column j is not read again; written back after the loop)
      if (!A.linv_lds && j + 1 < mB) {   // the next column's row of its inverse: requested a step ahead
#pragma unroll
        for (int s = 0; s < MRR_KMAX; ++s) if (s < k) lrow[s] = A.Linv[((size_t)Jl[j + 1] * k + l) * k + s];
      }
    }
    mrr_wave_sync();
    if (l > j && l < mB) {
      for (int t = 0; t < k; ++t) {
        const int g = c.pt[t];
        const double gv = g < ngl ? gl[(g * MRR_MB + j) * MRR_MB + l] : gglob[(g * MRR_MB + j) * MRR_MB + l];   // row j, lanes along it
        dc[l * 17 + t] -= gv * dbl[j * MRR_KMAX + t];
      }
    }
    mrr_wave_sync();
  }
  for (int i = l; i < MRR_MB * MRR_KMAX; i += 64) {
    const int jm = i / MRR_KMAX, t = i - jm * MRR_KMAX;
    A.dB[i] = (jm < mB && t < k) ? dbl[i] : 0.0;
  }
  for (int i = l; i < mB * k; i += 64) { const int jm = i / k, t = i - jm * k; A.b[(size_t)Jl[jm] * k + t] = b0l[jm * MRR_KMAX + t]; }
  if (l < k) A.db2[l] += acc2;
}

// ---- fitted values (:1054-1055): hat[t][r] = sum_j x_rj b_jt + mu_t for every row, the columns in index order; hat is n x k column-major ----
__global__ __launch_bounds__(256) void k_mrrd_hat(const double *__restrict__ X, int64_t n, int64_t r, int64_t ld, int k, const double *__restrict__ b,
                                                  const double *__restrict__ mu, double *__restrict__ hat) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double acc[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
  for (int64_t j = 0; j < r; ++j) {
    const double v = X[(size_t)j * (size_t)ld + (size_t)i];
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(v, b[j * k + t], acc[t]);
  }
  for (int t = 0; t < k; ++t) hat[(size_t)t * n + i] = acc[t] + mu[t];
}

}  // namespace bwgr
