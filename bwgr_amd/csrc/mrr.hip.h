// bwgr_amd: the multi-trait ridge regression engine -- MRR3 / MRR3F (src/RcppEigen20230423.cpp:318-700, :704-1080), mrr / mrr_float.
//
// One randomized Gauss-Seidel sweep over the markers updates the k-vector b_J of every marker J against the n x k residual E
// (:866-902).  The k x k tail (variance components, GC structure, bending, pinv) runs on the host in double (bwgr_mrr in
// bwgr_hip.hip); everything that reads X, E or a p x k array runs here:
//
//   k_mrr_setup_cols  once per call: column mean, per-pattern masked sums S_g = X'z_g and squares, X'y -> xbar, XX, XSX, tilde
//   k_mrr_gram        per sweep: G_g = X_B' diag(z_g) X_B for every 64-marker block of the gathered panel and every
//                     missingness pattern g (v_mfma_i32_16x16x64_i8 on operands whose unobserved rows are masked to zero)
//   k_mrr_linv        per sweep: (iG + diag(XX_J / ve))^-1 for every marker (Gauss-Jordan in LDS, one thread per marker)
//   k_mrr_pass        per block: E -= X_c,B-1 dB_B-1 o Z for the rows of a tile, then the partial dots X_B' E of the next block
//   k_mrr_solve       per block: the serial recurrence of the block's markers on the reduced dots (one workgroup)
//   k_mrr_ey, k_mrr_tilde, k_mrr_hat*   the tail's O(n k) and O(p k^2) reductions and the fitted values
//
// Centring is implicit: the panel stays int8 and x_c,j = x_j - xbar_j is applied as scalars.  E is zero on
// unobserved rows (y o Z, and every update is masked), so X_c,j'e_t = X_j'e_t - xbar_j sum(e_t), and the block's masked, centred Gram is
// G_g(j,i) - xbar_i S_g(j) - xbar_j S_g(i) + n_t xbar_i xbar_j.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bwgr {

static constexpr int MRR_MB = 64;        // markers per block of the sweep
static constexpr int MRR_KMAX = 16;      // traits
static constexpr int MRR_PASS_WG = 32;   // workgroups of k_mrr_pass (= partial dot sets the solve reduces)

typedef int mrr_v4i __attribute__((ext_vector_type(4)));

struct MrrConst {
  int k, npat;
  int pt[MRR_KMAX];        // missingness pattern of trait t
  double nt[MRR_KMAX];     // observed rows of trait t
  double iVe[MRR_KMAX];    // 1 / ve_t of this sweep
};

__device__ __forceinline__ size_t mrr_xoff(int64_t i, int64_t j, int R, int64_t p) {
  const int64_t w = i / R;
  return (size_t)((w * p + j) * R + (i - w * R));
}

__device__ __forceinline__ double mrr_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// LDS ordering between the lanes of one wave (the solve's serial phase runs on wave 0 alone).  A wave's LDS operations execute in order,
// so wavefront scope only has to keep the compiler from moving them; a workgroup-scope fence would also wait for every outstanding global
// load and store of the wave (vmcnt), once per marker.
__device__ __forceinline__ void mrr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- once per call: per-column statistics of the resident panel (natural order), one wave per column ----
// xbar_j = mean over all n rows (:763-765); S_g(j) = sum_r z_rg x_rj; XX[j][t] = sum_r z_rt (x_rj - xbar_j)^2 (:769-770);
// XSX[j][t] = XX/n_t - ((X_c,j'z_t)/n_t)^2 (:774-776); tilde[j][t] = X_c,j'y_t (:806).  zb[r]: bit g = row r observed in pattern g.
// centre = 0 (PEGS, which never centres X): xbar = 0, so XX is the raw masked sum of squares, XSX and tilde those of the raw columns, and
// the solve's Gram correction and the fitted values' offset vanish with no other change.
__global__ __launch_bounds__(256) void k_mrr_setup_cols(const int8_t *__restrict__ X, int R, int n, int64_t p, int64_t ld,
                                                        const uint32_t *__restrict__ zb, const double *__restrict__ y, const double *__restrict__ sumy,
                                                        const MrrConst c, int centre, double *__restrict__ xbar, double *__restrict__ S,
                                                        double *__restrict__ XX, double *__restrict__ XSX, double *__restrict__ tilde) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); j < p; j += nw) {
    int sx = 0, sg[MRR_KMAX], qg[MRR_KMAX];
    double xy[MRR_KMAX];
#pragma unroll
    for (int g = 0; g < MRR_KMAX; ++g) { sg[g] = 0; qg[g] = 0; xy[g] = 0.0; }
    for (int r = lane; r < n; r += 64) {
      const int x = (int)X[mrr_xoff(r, j, R, p)];
      const uint32_t z = zb[r];
      sx += x;
#pragma unroll
      for (int g = 0; g < MRR_KMAX; ++g)
        if (g < c.npat && ((z >> g) & 1u)) { sg[g] += x; qg[g] += x * x; }
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t)
        if (t < c.k) xy[t] = fma((double)x, y[(size_t)t * ld + r], xy[t]);
    }
    const double xb = mrr_wave_sum((double)sx) / (double)n;
    const double xbs = centre ? __shfl(xb, 0, 64) : 0.0;
    double sgs[MRR_KMAX], qgs[MRR_KMAX];
#pragma unroll
    for (int g = 0; g < MRR_KMAX; ++g) {
      sgs[g] = 0.0; qgs[g] = 0.0;
      if (g < c.npat) { sgs[g] = __shfl(mrr_wave_sum((double)sg[g]), 0, 64); qgs[g] = __shfl(mrr_wave_sum((double)qg[g]), 0, 64); }
    }
#pragma unroll
    for (int t = 0; t < MRR_KMAX; ++t) {
      const double xyt = (t < c.k) ? mrr_wave_sum(xy[t]) : 0.0;
      if (lane == 0 && t < c.k) {
        double s = 0.0, q = 0.0;
#pragma unroll
        for (int g = 0; g < MRR_KMAX; ++g) if (g == c.pt[t]) { s = sgs[g]; q = qgs[g]; }
        const double nt = c.nt[t];
        const double xxv = q - 2.0 * xbs * s + nt * xbs * xbs;          // sum z (x - xbar)^2
        const double xz = s - nt * xbs;                                 // X_c,j' z_t
        XX[j * c.k + t] = xxv;
        XSX[j * c.k + t] = xxv / nt - (xz / nt) * (xz / nt);
        tilde[j * c.k + t] = xyt - xbs * sumy[t];
      }
    }
    if (lane == 0) {
      xbar[j] = xbs;
#pragma unroll
      for (int g = 0; g < MRR_KMAX; ++g) if (g < c.npat) S[(size_t)g * p + j] = sgs[g];
    }
  }
}

// ---- per sweep: the block Gram matrices of the gathered panel, one per missingness pattern ----
// Workgroup (block b, pattern group): wave w builds G[b][g], g = 4 * blockIdx.y + w, as k_gram_mfma_i8 does for the plain Gram: lane
// (m16, grp) feeds the 16 bytes of marker 16a + m16 at rows r0 + 16grp .. +15; the B operand is the same bytes ANDed with the pattern's
// row mask zm[g][r] (0 or 0xFF), so the product sums over the pattern's observed rows only.  Exact in int32 (n |x|^2 < 2^31, checked
// by the host when the panel is made).  Out: G[(b * npat + g) * 4096 + i * 64 + j].
__global__ __launch_bounds__(256) void k_mrr_gram(const int8_t *__restrict__ Xs, int R, int64_t p, int64_t ld, const uint8_t *__restrict__ zm,
                                                  int npat, int32_t *__restrict__ G) {
  const int b = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m16 = lane & 15, grp = lane >> 4;
  const int g = 4 * blockIdx.y + wave;
  if (g >= npat) return;
  const int64_t j0 = (int64_t)b * MRR_MB;
  int64_t col[4]; bool ok[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { const int64_t j = j0 + 16 * a + m16; ok[a] = j < p; col[a] = ok[a] ? j : p - 1; }
  mrr_v4i acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = mrr_v4i{0, 0, 0, 0};
  const mrr_v4i zero = {0, 0, 0, 0};
  const uint8_t *zg = zm + (size_t)g * ld;
  for (int64_t r0 = 0; r0 < ld; r0 += 64) {
    const int64_t sl = r0 / R;
    const size_t roff = (size_t)(r0 - sl * R) + 16 * grp;
    const int8_t *sb = Xs + (size_t)sl * p * R + roff;
    const mrr_v4i mk = *reinterpret_cast<const mrr_v4i *>(zg + r0 + 16 * grp);
    mrr_v4i av[4], bv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      av[a] = ok[a] ? *reinterpret_cast<const mrr_v4i *>(sb + (size_t)col[a] * R) : zero;
      bv[a] = av[a] & mk;
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[a], bv[c], acc[a][c], 0, 0, 0);
  }
  int32_t *out = G + ((size_t)b * npat + g) * (MRR_MB * MRR_MB);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) out[(size_t)(16 * a + 4 * grp + reg) * MRR_MB + 16 * c + m16] = acc[a][c][reg];
}

// ---- per sweep: Linv[J] = (iG + diag(XX[J] / ve))^-1 for every marker (:884), natural order ----
// LHS_J depends only on XX_J, ve and iG, all fixed during the sweep, so the p inverses come off the serial chain.  One thread per
// marker; its k x k matrix lives in LDS as a[e * 64 + tid] (conflict-free).  Gauss-Jordan without pivoting (LHS is SPD).
__global__ __launch_bounds__(64) void k_mrr_linv(const double *__restrict__ XX, const double *__restrict__ iG, const MrrConst c, int64_t p,
                                                 double *__restrict__ Linv) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *a = reinterpret_cast<double *>(smem);
  const int k = c.k, tid = threadIdx.x;
  const int64_t J = (int64_t)blockIdx.x * 64 + tid;
  if (J >= p) return;
  for (int r = 0; r < k; ++r)
    for (int s = 0; s < k; ++s) a[(r * k + s) * 64 + tid] = iG[r * k + s] + (r == s ? XX[J * k + r] * c.iVe[r] : 0.0);
  for (int piv = 0; piv < k; ++piv) {
    const double d = 1.0 / a[(piv * k + piv) * 64 + tid];
    a[(piv * k + piv) * 64 + tid] = 1.0;
    for (int s = 0; s < k; ++s) a[(piv * k + s) * 64 + tid] *= d;
    for (int r = 0; r < k; ++r) {
      if (r == piv) continue;
      const double f = a[(r * k + piv) * 64 + tid];
      a[(r * k + piv) * 64 + tid] = 0.0;
      for (int s = 0; s < k; ++s) a[(r * k + s) * 64 + tid] -= f * a[(piv * k + s) * 64 + tid];
    }
  }
  double *o = Linv + (size_t)J * k * k;
  for (int e = 0; e < k * k; ++e) o[e] = a[e * 64 + tid];
}

// ---- per block: the residual update of block `prev` and the partial dots of block `next` in one pass over the rows ----
// Tiles of 64 rows (one slab each: R is a multiple of 128); workgroup w takes tiles w, w + G, ...  For a tile:
//   update (prev >= 0): e_rt -= z_rt (sum_j x_rj dB_jt - c_t), c_t = sum_j xbar_j dB_jt (written by the solve)  -- :900-901
//   dots   (next >= 0): part[w][j][t] += sum_r x_rj e_rt over the tile; part[w][64][t] += sum_r e_rt
// E is [t][ld] fp64; padding rows have z = 0 and stay 0.
struct MrrPassArgs {
  const int8_t *Xs; int R; int64_t p, ld; int nblk;
  const uint32_t *zb; double *e;
  const double *dB;     // [64][16] + c[16] at [64 * 16]
  double *part;         // [G][65][16]
  int prev, next, k;
};
__global__ __launch_bounds__(256) void k_mrr_pass(const MrrPassArgs A) {
  __shared__ __attribute__((aligned(16))) int8_t xt[MRR_MB * 68];   // [marker][row], 68-byte rows (conflict-free dword reads)
  __shared__ double et[64 * MRR_KMAX];                              // [row][t]
  __shared__ double dBl[MRR_MB * MRR_KMAX + MRR_KMAX];
  const int tid = threadIdx.x, k = A.k;
  const int rr = tid & 63, tq = tid >> 6;
  const int64_t ntiles = A.ld / 64;
  if (A.prev >= 0)
    for (int i = tid; i < MRR_MB * MRR_KMAX + MRR_KMAX; i += 256) dBl[i] = A.dB[i];
  double dacc[4] = {0.0, 0.0, 0.0, 0.0}, eacc = 0.0;
  auto load_tile = [&](int blk, int64_t r0) {
    const int jm = tid >> 2, q = tid & 3;
    const int64_t j = (int64_t)blk * MRR_MB + jm;
    mrr_v4i v = {0, 0, 0, 0};
    if (j < A.p) v = *reinterpret_cast<const mrr_v4i *>(A.Xs + mrr_xoff(r0 + 16 * q, j, A.R, A.p));
    int *dst = reinterpret_cast<int *>(xt + jm * 68 + 16 * q);
    dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
  };
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t r0 = tile * 64, r = r0 + rr;
    __syncthreads();
    if (A.prev >= 0) {
      load_tile(A.prev, r0);
      __syncthreads();
      const uint32_t z = A.zb[r];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int t = tq + 4 * i;
        if (t < k) {
          double s = 0.0;
          for (int jm = 0; jm < MRR_MB; ++jm) s = fma((double)xt[jm * 68 + rr], dBl[jm * MRR_KMAX + t], s);
          double ev = A.e[(size_t)t * A.ld + r];
          if ((z >> t) & 1u) ev -= s - dBl[MRR_MB * MRR_KMAX + t];
          A.e[(size_t)t * A.ld + r] = ev;
          et[rr * MRR_KMAX + t] = ev;
        }
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) et[rr * MRR_KMAX + t] = A.e[(size_t)t * A.ld + r]; }
    }
    if (A.next < 0) continue;
    load_tile(A.next, r0);
    __syncthreads();
    const int jm = tid & 63;
    const int *xw = reinterpret_cast<const int *>(xt + jm * 68);
    for (int w4 = 0; w4 < 16; ++w4) {
      const int word = xw[w4];
#pragma unroll
      for (int by = 0; by < 4; ++by) {
        const double x = (double)(int)(int8_t)(word >> (8 * by));
        const int row = 4 * w4 + by;
#pragma unroll
        for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) dacc[i] = fma(x, et[row * MRR_KMAX + t], dacc[i]); }
      }
    }
    if (tid < k) for (int row = 0; row < 64; ++row) eacc += et[row * MRR_KMAX + tid];
  }
  if (A.next < 0) return;
  double *pw = A.part + (size_t)blockIdx.x * (MRR_MB + 1) * MRR_KMAX;
  const int jm = tid & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) { const int t = tq + 4 * i; if (t < k) pw[jm * MRR_KMAX + t] = dacc[i]; }
  if (tid < k) pw[MRR_MB * MRR_KMAX + tid] = eacc;
}

// ---- per block: the serial recurrence of the block's markers (:869-901) ----
// Phase 1 (256 threads): dc[j][t] = sum_w part[w][j][t] - xbar_J sum(e_t): the centred dots X_c,J'e_t at the block's start; the block's
// Gram matrices (the first ngl patterns; the rest are read from L2), the markers' inverses (linv_lds: when 64 k^2 doubles fit beside them),
// XX, b0, xbar, S staged into LDS.  New effects are kept in LDS and written back once, after the loop.  Phase 2 (wave 0 alone, no workgroup barriers), marker j in order:
//   lanes t < k:  RHS_t = (dc[j][t] + XX_Jt b0_t) / ve_t;   b1 = Linv_J RHS;   dB_jt = b1_t - b0_t;   b[J] = b1
//   lanes l > j:  dc[l][t] -= Gc_t(l, j) dB_jt, Gc_t the masked centred Gram (see the file head)
// Afterwards dB (and c_t = sum_j xbar_J dB_jt) go out for the next pass, and sum_j dB_jt^2 (the sweep's Delta b, each marker is visited
// once) is added to db2[t] for the convergence value.
struct MrrSolveArgs {
  const double *part; int G;
  const int32_t *order; int blk; int64_t p;
  const int32_t *gram; const double *xbar, *S, *XX, *Linv;
  double *b, *dB, *db2;
  int ngl, linv_lds;
};
__host__ __device__ inline size_t mrr_solve_lds(int ngl, int linv_doubles) {
  return (size_t)ngl * MRR_MB * MRR_MB * 4 + sizeof(double) * (size_t)linv_doubles +
         sizeof(double) * (size_t)(MRR_MB * 17 + 3 * MRR_MB * MRR_KMAX + MRR_MB + MRR_KMAX * MRR_MB + 2 * MRR_KMAX) + 64 * 4;
}
__global__ __launch_bounds__(256) void k_mrr_solve(const MrrSolveArgs A, const MrrConst c) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int k = c.k, npat = c.npat, ngl = A.ngl, tid = threadIdx.x;
  int32_t *gl = reinterpret_cast<int32_t *>(smem);
  double *linvl = reinterpret_cast<double *>(smem + (size_t)ngl * MRR_MB * MRR_MB * 4);   // [64][k][k] when linv_lds
  double *dc = linvl + (A.linv_lds ? MRR_MB * k * k : 0);                                  // [64][17]
  double *xxl = dc + MRR_MB * 17, *b0l = xxl + MRR_MB * MRR_KMAX, *dbl = b0l + MRR_MB * MRR_KMAX;
  double *xbl = dbl + MRR_MB * MRR_KMAX, *sl = xbl + MRR_MB, *rhs = sl + MRR_KMAX * MRR_MB, *se = rhs + MRR_KMAX;
  int *Jl = reinterpret_cast<int *>(se + MRR_KMAX);
  const int64_t j0 = (int64_t)A.blk * MRR_MB;
  const int mB = (int)(A.p - j0 < MRR_MB ? A.p - j0 : MRR_MB);
  if (tid < MRR_MB) {
    const int J = tid < mB ? A.order[j0 + tid] : 0;
    Jl[tid] = J;
    xbl[tid] = tid < mB ? A.xbar[J] : 0.0;
    for (int g = 0; g < npat; ++g) sl[g * MRR_MB + tid] = tid < mB ? A.S[(size_t)g * A.p + J] : 0.0;
  }
  if (tid < k) {
    double s = 0.0;
    for (int w = 0; w < A.G; ++w) s += A.part[((size_t)w * (MRR_MB + 1) + MRR_MB) * MRR_KMAX + tid];
    se[tid] = s;
  }
  {
    const int4 *src = reinterpret_cast<const int4 *>(A.gram + (size_t)A.blk * npat * MRR_MB * MRR_MB);
    int4 *dst = reinterpret_cast<int4 *>(gl);
    for (int i = tid; i < ngl * MRR_MB * MRR_MB / 4; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  for (int o = tid; o < MRR_MB * k; o += 256) {
    const int jm = o / k, t = o - jm * k;
    double s = 0.0;
    for (int w = 0; w < A.G; ++w) s += A.part[((size_t)w * (MRR_MB + 1) + jm) * MRR_KMAX + t];
    const int J = Jl[jm];
    dc[jm * 17 + t] = s - xbl[jm] * se[t];
    xxl[jm * MRR_KMAX + t] = jm < mB ? A.XX[(size_t)J * k + t] : 0.0;
    b0l[jm * MRR_KMAX + t] = jm < mB ? A.b[(size_t)J * k + t] : 0.0;
  }
  if (A.linv_lds)
    for (int i = tid; i < mB * k * k; i += 256) { const int jm = i / (k * k); linvl[i] = A.Linv[(size_t)Jl[jm] * k * k + (i - jm * k * k)]; }
  __syncthreads();
  if (tid >= 64) return;
  const int l = tid;
  const int32_t *gglob = A.gram + (size_t)A.blk * npat * MRR_MB * MRR_MB;
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
      b0l[j * MRR_KMAX + l] = b1;   // (b0 of marker j is not read again; written back after the loop)
      if (!A.linv_lds && j + 1 < mB) {   // the next marker's row of its inverse: requested a step ahead
#pragma unroll
        for (int s = 0; s < MRR_KMAX; ++s) if (s < k) lrow[s] = A.Linv[((size_t)Jl[j + 1] * k + l) * k + s];
      }
    }
    mrr_wave_sync();
    if (l > j && l < mB) {
      const double xl = xbl[l], xj = xbl[j];
      for (int t = 0; t < k; ++t) {
        const int g = c.pt[t];
        const double gv = (double)(g < ngl ? gl[(g * MRR_MB + j) * MRR_MB + l] : gglob[(g * MRR_MB + j) * MRR_MB + l]);   // G(l,j) = G(j,l): row j, lanes along it
        const double gc = gv - xj * sl[g * MRR_MB + l] - xl * sl[g * MRR_MB + j] + c.nt[t] * xl * xj;
        dc[l * 17 + t] -= gc * dbl[j * MRR_KMAX + t];
      }
    }
    mrr_wave_sync();
  }
  for (int i = l; i < MRR_MB * MRR_KMAX; i += 64) {
    const int jm = i / MRR_KMAX, t = i - jm * MRR_KMAX;
    A.dB[i] = (jm < mB && t < k) ? dbl[i] : 0.0;
  }
  for (int i = l; i < mB * k; i += 64) { const int jm = i / k, t = i - jm * k; A.b[(size_t)Jl[jm] * k + t] = b0l[jm * MRR_KMAX + t]; }
  if (l < k) {
    double cs = 0.0;
    for (int j = 0; j < mB; ++j) cs = fma(xbl[j], dbl[j * MRR_KMAX + l], cs);
    A.dB[MRR_MB * MRR_KMAX + l] = cs;
    A.db2[l] += acc2;
  }
}

// ---- tail reductions, deterministic (fixed partial order) ----
// out[t] = sum_r e_rt y_rt (:916), out[k + t] = sum_r e_rt (updateMu, :1031)
__global__ __launch_bounds__(256) void k_mrr_ey(const double *__restrict__ e, const double *__restrict__ y, int64_t ld, int k, double *__restrict__ part) {
  __shared__ double red[8];
  const int t = blockIdx.y;
  double s1 = 0.0, s2 = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < ld; r += (int64_t)gridDim.x * 256) {
    const double ev = e[(size_t)t * ld + r];
    s1 = fma(ev, y[(size_t)t * ld + r], s1); s2 += ev;
  }
  s1 = mrr_wave_sum(s1); s2 = mrr_wave_sum(s2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[w] = s1; red[4 + w] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    part[((size_t)blockIdx.x * 2 * k) + t] = red[0] + red[1] + red[2] + red[3];
    part[((size_t)blockIdx.x * 2 * k) + k + t] = red[4] + red[5] + red[6] + red[7];
  }
}
// mode 0: out[s*k + t] = sum_j b_js tilde_jt              (TildeHat = b'tilde, :938)
// mode 1: out[s*k + t] = sum_j b_js Dinv_jt tilde_jt, out[k*k + t] = sum_j XSXn_jt Dinv_jt, Dinv_jt = 1/(XSXn_jt/ve_t + iG_tt),
//         XSXn = n_t XSX  (TH, :806-810, :930-936)
// mode 2: out[t] = sum_j A_jt  (MSx = colSums(XSX), :776)
__global__ __launch_bounds__(256) void k_mrr_tilde(const double *__restrict__ b, const double *__restrict__ tilde, const double *__restrict__ XSX,
                                                   int64_t p, int mode, const MrrConst c, const double *__restrict__ iGd, double *__restrict__ part) {
  __shared__ double red[4];
  const int k = c.k, o = blockIdx.y;
  const int s = o / k, t = o - s * k;
  double acc = 0.0;
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < p; j += (int64_t)gridDim.x * 256) {
    if (mode == 2) { acc += XSX[j * k + o]; continue; }
    if (mode == 0) { acc = fma(b[j * k + s], tilde[j * k + t], acc); continue; }
    if (o < k * k) {
      const double xs = XSX[j * k + t] * c.nt[t];
      const double dinv = 1.0 / (xs * c.iVe[t] + iGd[t]);
      acc = fma(b[j * k + s], dinv * tilde[j * k + t], acc);
    } else {
      const int u = o - k * k;
      const double xs = XSX[j * k + u] * c.nt[u];
      acc = fma(xs, 1.0 / (xs * c.iVe[u] + iGd[u]), acc);
    }
  }
  acc = mrr_wave_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * gridDim.y + o] = red[0] + red[1] + red[2] + red[3];
}
// out[o] = sum over the nparts partials, in order
__global__ void k_mrr_finish(const double *__restrict__ part, int nparts, int nout, double *__restrict__ out) {
  for (int o = threadIdx.x; o < nout; o += blockDim.x) {
    double s = 0.0;
    for (int w = 0; w < nparts; ++w) s += part[(size_t)w * nout + o];
    out[o] = s;
  }
}
// updateMu (:1030-1036): e_t = (e_t - d_t) o z_t
__global__ void k_mrr_mu_shift(double *__restrict__ e, const uint32_t *__restrict__ zb, int64_t ld, int n, int k, const double *__restrict__ d) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t z = zb[r];
    for (int t = 0; t < k; ++t) e[(size_t)t * ld + r] = ((z >> t) & 1u) ? e[(size_t)t * ld + r] - d[t] : 0.0;
  }
}
// fitted values (:1054-1055): hpart[chunk][t][ld] = sum_{j in chunk} x_rj b_jt over the natural panel; the host adds mu_t - sum_j xbar_j b_jt
__global__ __launch_bounds__(256) void k_mrr_hat_part(const int8_t *__restrict__ X, int R, int64_t p, int64_t ld, int n, int k, const double *__restrict__ b,
                                                      int64_t cols_per_chunk, double *__restrict__ hpart) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t ja = (int64_t)blockIdx.y * cols_per_chunk, jb = ja + cols_per_chunk < p ? ja + cols_per_chunk : p;
  double acc[MRR_KMAX];
#pragma unroll
  for (int t = 0; t < MRR_KMAX; ++t) acc[t] = 0.0;
  if (r < n) {
    for (int64_t j = ja; j < jb; ++j) {
      const double x = (double)X[mrr_xoff(r, j, R, p)];
#pragma unroll
      for (int t = 0; t < MRR_KMAX; ++t) if (t < k) acc[t] = fma(x, b[j * k + t], acc[t]);
    }
  }
  if (r < ld)
    for (int t = 0; t < k; ++t) hpart[((size_t)blockIdx.y * k + t) * ld + r] = acc[t];
}
__global__ void k_mrr_hat_finish(const double *__restrict__ hpart, int nchunks, int64_t ld, int n, int k, const double *__restrict__ off, double *__restrict__ hat) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)n * k; i += (int64_t)gridDim.x * blockDim.x) {
    const int t = (int)(i / n);
    const int64_t r = i - (int64_t)t * n;
    double s = 0.0;
    for (int c = 0; c < nchunks; ++c) s += hpart[((size_t)c * k + t) * ld + r];
    hat[i] = s + off[t];
  }
}

}  // namespace bwgr

// ------------------------------------------------------------------------------------------------
// host side of the tail: the k x k work of one iteration (:916-1036), in double
// ------------------------------------------------------------------------------------------------
#include <vector>
#include <math.h>
#include <algorithm>
#include "pegs_tail.h"   // mrr_eigh, mrr_pinv

namespace bwgr {

// the leading NumXFA eigen-terms of GC: sum_i lambda_(k-1-i) v v' (:969-970, :983-984)
static void mrr_udu(int k, const double *GC, int nf, double *UDU) {
  std::vector<double> w(k), V((size_t)k * k);
  mrr_eigh(k, GC, w.data(), V.data());
  for (int i = 0; i < k * k; ++i) UDU[i] = 0.0;
  for (int i = 0; i < nf; ++i) {
    const int e = k - 1 - i;
    for (int r = 0; r < k; ++r) for (int c = 0; c < k; ++c) UDU[r * k + c] += w[e] * V[r * k + e] * V[c * k + e];
  }
}

struct MrrOpts {
  int maxit; double tol; bool TH, HCS, XFA, ACS; int NumXFA; double R2, gc0, df0; bool updateMu; double wph2, wpgc; bool OneVarB, OneVarE, verbose;
};

// variance components after the sweep (:916-1028).  vb / GC / iG are k x k row-major.  TH_ = TildeHat, Tr = TrDinvXSX (TH) or TrXSX.
static void mrr_tail_vb(int k, const MrrOpts &o, const double *TH_, const double *Tr, const double *Sb, const double *vbInit,
                        double *vb, double *GC, double *iG, int *bent) {
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {
      if (i == j) vb[i * k + i] = (TH_[i * k + i] + Sb[i * k + i]) / (Tr[i] + o.df0);                                 // :944-946
      else vb[i * k + j] = (TH_[i * k + j] + TH_[j * k + i] + Sb[i * k + j]) / (Tr[i] + Tr[j] + o.df0);                 // :950-952
    }
  if (o.wph2 > 0) for (int i = 0; i < k; ++i) vb[i * k + i] = vb[i * k + i] * (1 - o.wph2) + o.wph2 * vbInit[i];      // :957-958
  if (o.wpgc > 0) {                                                                                                    // :959-962
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j)
      GC[i * k + j] = (i != j) ? (1.0 - o.wpgc) * vb[i * k + j] / sqrt(vb[i * k + i] * vb[j * k + j]) + o.gc0 * o.wpgc : 1.0;
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) if (i != j) vb[i * k + j] = GC[i * k + j] * sqrt(vb[i * k + i] * vb[j * k + j]);
  } else {
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[i * k + j] = vb[i * k + j] / sqrt(vb[i * k + i] * vb[j * k + j]);   // :964
  }
  std::vector<double> U((size_t)k * k);
  if (o.ACS) {                                                                                                         // :967-973
    double s = 0.0; for (int i = 0; i < k * k; ++i) s += GC[i];
    const double gs = (s - k) / (double)(k * (k - 1)) / 2.0;
    mrr_udu(k, GC, o.NumXFA, U.data());
    for (int i = 0; i < k * k; ++i) GC[i] = (U[i] + gs) * 0.5;
    for (int i = 0; i < k; ++i) GC[i * k + i] = 1.0;
  } else if (o.HCS) {                                                                                                  // :974-981
    double gs = 0.0;
    for (int i = 0; i < k; ++i) for (int j = 0; j < i; ++j) gs += GC[i * k + j];
    gs = gs / (double)((k * (k - 1)) / 2);
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC[i * k + j] = (i != j) ? gs : 1.0;
  } else if (o.XFA) {                                                                                                  // :982-986
    mrr_udu(k, GC, o.NumXFA, U.data());
    for (int i = 0; i < k * k; ++i) GC[i] = U[i];
    for (int i = 0; i < k; ++i) GC[i * k + i] = 1.0;
  }
  // bending, always taken without NoInv (:1006-1021): the smallest eigenvalue below 0 -> A = (GC + inflate I) / (1 + inflate)
  {
    std::vector<double> w(k), V((size_t)k * k);
    mrr_eigh(k, GC, w.data(), V.data());
    *bent = 0;
    if (w[0] < 0.0) {
      const double inflate = fabs(w[0] * 1.1);
      for (int i = 0; i < k; ++i) GC[i * k + i] += inflate;
      for (int i = 0; i < k * k; ++i) GC[i] /= (1.0 + inflate);
      *bent = 1;
    }
  }
  if (o.OneVarB) {                                                                                                     // :1023
    double tmp = 0.0; for (int i = 0; i < k; ++i) tmp += TH_[i * k + i];
    tmp /= k;
    for (int i = 0; i < k * k; ++i) vb[i] = GC[i] * tmp;
  } else {
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) vb[i * k + j] = GC[i * k + j] * sqrt(vb[i * k + i] * vb[j * k + j]);   // :1023-1025 (in place, as there)
  }
  mrr_pinv(k, vb, iG);                                                                                                 // :1027
}

}  // namespace bwgr
