// kernels.hip.h -- relationship kernels on the resident int8 panel: the exact product G = X X' (n x n int64, k_xxt_*) and the fp64
// finishes that turn it into GRM / GAU (src/Rcpp20260726ai.cpp:1338-1383) and EigenGRM / EigenGAU / EigenARC
// (src/RcppEigen20230423.cpp:8-51) (k_kfin_*); the exact product X_f X_s' between two panels over the same markers (k_xyt_mfma_i8) and
// the finishes of the founder-by-sample kernels EigenArcZ / EigenGauZ (src/RcppEigen20230423.cpp:1877-1939) (k_kfin2_*).  DESIGN.md
// section 4.6 has the layout problem and the reasons for the choices below.
//
// Out of scope here: fp32 panels (they need a float product with a numerics contract of its own), EigenEVD / K2X / mkr / mkr2X (the
// eigendecomposition stays with the caller), CNT / IMP / SPC / SPM, and sharding the product over GPUs.  (Clearing the genotypes of covariates before a
// kernel is formed -- MLM's projection -- is project.hip.h, and gives a dense fp64 matrix, not a panel.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bwgr {

constexpr int XXT_TILE = 128;    // rows of an output tile side: one workgroup of four waves, a 64 x 64 quadrant each
constexpr int XXT_KSTEP = 64;    // markers per v_mfma_i32_16x16x64_i8
enum { KFIN_GRM = 0, KFIN_GAU = 1, KFIN_EIGEN_GRM = 2, KFIN_EIGEN_GAU = 3, KFIN_EIGEN_ARC = 4 };

struct XxtArgs {
  const int8_t *XA, *XB;    // operand A's panel (the rows of G) and operand B's (its columns) over the same p markers; X X': the same panel twice
  int64_t p;
  int RA, RB;               // slab rows of either panel (two panels are made independently: they may differ)
  int nA, nB;               // real rows of either panel
  int T;                    // X X': row tiles; X_A X_B': column tiles
  int64_t chunk, piece;     // markers per int32 chunk; markers per workgroup (a multiple of XXT_KSTEP), pieces never cross a chunk
  int sub;                  // pieces per chunk
  int accumulate;           // 0: one workgroup per tile stores; 1: every workgroup adds its int32 sums into the zeroed int64 tile
  long long *G;
  int64_t ldg;
};

// The product's tile (ti, tj) of 128 x 128: four waves, a 64 x 64 quadrant each.  The panel stores a marker's rows contiguously, the MFMA sums
// along its operands' 16-byte runs, and here the sum runs over the markers: the bytes have to be transposed.  The marker order inside a step
// and the row order inside a wave's 64 rows are free as long as both operands use the same maps -- they do, whether the operands are rows of
// the same matrix (X X') or of two panels (X_A X_B'); only the slab height that turns a marker into an address may differ between the
// operands.  A lane loads one dword = rows 4 m16 .. 4 m16 + 3 of one marker; sixteen such dwords (markers 16 u + 4 grp + q) go through the
// 4 x 4 byte transposition of k_sweep3's update operand (two rounds of v_perm_b32) and come out as four operands of 16 bytes, operand a =
// row 4 m16 + a over the lane's sixteen markers.  MFMA tile a of a wave therefore holds rows r0 + 4 m + a (m = 0 .. 15) and the write-out puts
// them back, guarding the rows against n_A and the columns against n_B.  No LDS, no barrier: the two waves that share a row range meet in
// the L1.  The paddings of the panels are zero.
//
// ONE_R: operand B has operand A's slab height (X X'), so that one set of sixteen lane offsets serves both; otherwise each has its own.
// blockIdx.y: chunk * sub + piece.
template <bool ONE_R>
__device__ __forceinline__ void xxt_tile(const XxtArgs &a, int ti, int tj) {
  const int64_t c = blockIdx.y / a.sub, s = blockIdx.y - c * a.sub;
  const int64_t chunk_hi = min(a.p, (c + 1) * a.chunk);
  const int64_t lo = c * a.chunk + s * a.piece, hi = min(chunk_hi, lo + a.piece);
  if (lo >= hi) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), m16 = lane & 15, grp = lane >> 4;
  const int rA0 = XXT_TILE * ti + 64 * (wave >> 1), rB0 = XXT_TILE * tj + 64 * (wave & 1);
  const int RA = a.RA, RB = ONE_R ? a.RA : a.RB;
  // slab bases (a tile never crosses a slab of its panel: RA and RB are multiples of 128); marker j adds j * RA, j * RB
  const int8_t *ubA = a.XA + (size_t)(rA0 / RA) * a.p * RA + (rA0 % RA);
  const int8_t *ubB = a.XB + (size_t)(rB0 / RB) * a.p * RB + (rB0 % RB);

  s2_v4i acc[4][4];
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int y = 0; y < 4; ++y) acc[x][y] = s2_v4i{0, 0, 0, 0};

  // whole steps: the lane's sixteen markers of a step are j0 + 16 u + q + 4 grp.  The step's base is a wave-uniform pointer per operand and
  // the lane's part a 32-bit offset that does not change over the loop, so that a load costs no vector address arithmetic.
  uint32_t voffA[4][4], voffB[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      voffA[u][q] = (uint32_t)(16 * u + q + 4 * grp) * (uint32_t)RA + 4u * m16;
      voffB[u][q] = (uint32_t)(16 * u + q + 4 * grp) * (uint32_t)RB + 4u * m16;
    }
  auto load_full = [&](int64_t j0, uint32_t (&ca)[4][4], uint32_t (&cb)[4][4]) {
    const int8_t *pa = ubA + (size_t)j0 * RA, *pb = ubB + (size_t)j0 * RB;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        ca[u][q] = *reinterpret_cast<const uint32_t *>(pa + voffA[u][q]);
        cb[u][q] = *reinterpret_cast<const uint32_t *>(pb + voffB[u][q]);
      }
  };
  // the last, partial step: markers past `hi` are read at hi - 1 and zeroed
  auto load_tail = [&](int64_t j0, uint32_t (&ca)[4][4], uint32_t (&cb)[4][4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t j = j0 + 16 * u + q + 4 * grp;
        const bool ok = j < hi;
        const size_t jj = (size_t)(ok ? j : hi - 1);
        const uint32_t va = *reinterpret_cast<const uint32_t *>(ubA + jj * RA + 4u * m16), vb = *reinterpret_cast<const uint32_t *>(ubB + jj * RB + 4u * m16);
        ca[u][q] = ok ? va : 0u; cb[u][q] = ok ? vb : 0u;
      }
  };
  // rw[x] = the operand of MFMA tile x: bytes (u, q) = row 4 m16 + x of marker 16 u + 4 grp + q
  auto transpose = [](const uint32_t (&cc)[4][4], s2_v4i (&rw)[4]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const uint32_t t0 = __builtin_amdgcn_perm(cc[u][1], cc[u][0], 0x05010400u), t1 = __builtin_amdgcn_perm(cc[u][1], cc[u][0], 0x07030602u);
      const uint32_t t2 = __builtin_amdgcn_perm(cc[u][3], cc[u][2], 0x05010400u), t3 = __builtin_amdgcn_perm(cc[u][3], cc[u][2], 0x07030602u);
      rw[0][u] = (int)__builtin_amdgcn_perm(t2, t0, 0x05040100u); rw[1][u] = (int)__builtin_amdgcn_perm(t2, t0, 0x07060302u);
      rw[2][u] = (int)__builtin_amdgcn_perm(t3, t1, 0x05040100u); rw[3][u] = (int)__builtin_amdgcn_perm(t3, t1, 0x07060302u);
    }
  };
  auto mma = [&](const uint32_t (&ca)[4][4], const uint32_t (&cb)[4][4]) {
    s2_v4i ra[4], rb[4];
    transpose(ca, ra); transpose(cb, rb);
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
      for (int y = 0; y < 4; ++y) acc[x][y] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ra[x], rb[y], acc[x][y], 0, 0, 0);
  };

  // One register set per wave: a wave's loads are not in flight during its own MFMAs; the other waves of the SIMD cover them.  (Two sets
  // in turn -- a step requested during the MFMAs of the step before -- measured 2.8 times SLOWER at 10 000 x 100 000: twice the lines in
  // flight per compute unit no longer fit the L1, where the four waves of a workgroup share every line)
  const int64_t nfull = (hi - lo) / XXT_KSTEP;
  uint32_t ca[4][4], cb[4][4];
  for (int64_t k = 0; k < nfull; ++k) {
    load_full(lo + XXT_KSTEP * k, ca, cb);
    mma(ca, cb);
  }
  if (lo + nfull * XXT_KSTEP < hi) {
    load_tail(lo + nfull * XXT_KSTEP, ca, cb);
    mma(ca, cb);
  }

  // acc[x][y][reg] of lane (m16, grp) = G[rA0 + 4 (4 grp + reg) + x][rB0 + 4 m16 + y]
#pragma unroll
  for (int x = 0; x < 4; ++x)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = rA0 + 4 * (4 * grp + reg) + x;
      if (row >= a.nA) continue;
      long long *g = a.G + (size_t)row * a.ldg + rB0 + 4 * m16;
#pragma unroll
      for (int y = 0; y < 4; ++y) {
        if (rB0 + 4 * m16 + y >= a.nB) continue;
        if (a.accumulate) atomicAdd(reinterpret_cast<unsigned long long *>(g + y), (unsigned long long)(long long)acc[x][y][reg]);
        else g[y] = (long long)acc[x][y][reg];
      }
    }
}

// G = X X' (XB = XA, RB = RA, nB = nA): only the tile pairs ti <= tj, blockIdx.x row-major over the upper triangle; k_xxt_mirror fills the rest
__global__ __launch_bounds__(256) void k_xxt_mfma_i8(const XxtArgs a) {
  int t = blockIdx.x, ti = 0;
  while (t >= a.T - ti) { t -= a.T - ti; ++ti; }
  xxt_tile<true>(a, ti, ti + t);
}
// G = X_A X_B' between two panels: every tile of the T_A x T_B grid (no triangle, no mirror), blockIdx.x = ti * T + tj
__global__ __launch_bounds__(256) void k_xyt_mfma_i8(const XxtArgs a) {
  const int ti = blockIdx.x / a.T;
  xxt_tile<false>(a, ti, blockIdx.x - ti * a.T);
}

// nr x nc entries of an int64 matrix set to zero (before an accumulating product); entries beyond column nc of a row are not touched.
// upper: only the tiles on and above the diagonal (those that X X' computes).
__global__ void k_xxt_zero(long long *G, int64_t ldg, int nr, int nc, int upper) {
  const int64_t total = (int64_t)nr * nc;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / nc, j = idx - i * nc;
    if (!upper || j / XXT_TILE >= i / XXT_TILE) G[(size_t)i * ldg + j] = 0;
  }
}

// G[i][j] = G[j][i] for i > j, through a 32 x 33 LDS tile so that both sides are read and written along rows.  block (32, 8); grid (T32, T32),
// workgroups above the diagonal leave at once.
__global__ __launch_bounds__(256) void k_xxt_mirror(long long *G, int64_t ldg, int n) {
  __shared__ long long tile[32][33];
  const int br = blockIdx.y, bc = blockIdx.x;
  if (bc > br) return;
  for (int y = threadIdx.y; y < 32; y += 8) {
    const int i = bc * 32 + y, j = br * 32 + threadIdx.x;     // source element (i, j) of the upper triangle
    tile[y][threadIdx.x] = (i < n && j < n) ? G[(size_t)i * ldg + j] : 0;
  }
  __syncthreads();
  for (int y = threadIdx.y; y < 32; y += 8) {
    const int i = br * 32 + y, j = bc * 32 + threadIdx.x;     // destination (i, j), i > j
    if (i < n && j < n && i > j) G[(size_t)i * ldg + j] = tile[threadIdx.x][y];
  }
}

// ---- the finishes -------------------------------------------------------------------------------------------------------------------
// s_j = sum_i x_ij and q_j = sum_i x_ij^2, exact; one wave per marker
__global__ void k_kfin_colstats(const int8_t *X, int R, int n, int64_t p, int32_t *s, long long *q) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= p) return;
  long long s1 = 0, s2 = 0;
  for (int i = lane; i < n; i += 64) { const int v = (int)X[xoff(i, j, R, p)]; s1 += v; s2 += v * v; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
  if (lane == 0) { s[j] = (int32_t)s1; q[j] = s2; }
}

// The row reduction of the finishes, exact in int64: out_i += sum_j x_ij w_j over the workgroup's markers, w_j = s_j (SQ = false: rs = X s)
// or w_j = x_ij itself (SQ = true: q_i = sum_j x_ij^2, diag(X X') without the product; s is not read).  out has ld entries and is zeroed by
// the caller; padded rows add 0; integer adds commute, so the split over workgroups does not show.  A workgroup takes 128 rows (a dword of
// four rows per thread of a group of 32) and `cols` markers, its eight groups every eighth of them.
template <bool SQ>
__device__ __forceinline__ void kfin_rows(const int8_t *X, int R, int64_t p, const int32_t *s, int64_t cols, long long *out) {
  __shared__ long long red[8][128];
  const int tx = threadIdx.x & 31, g = threadIdx.x >> 5;
  const int r0 = 128 * blockIdx.x;
  const int64_t j0 = (int64_t)blockIdx.y * cols, j1 = min(p, j0 + cols);
  const int8_t *base = X + (size_t)(r0 / R) * p * R + (r0 % R) + 4 * tx;
  long long acc[4] = {0, 0, 0, 0};
  for (int64_t j = j0 + g; j < j1; j += 8) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(base + (size_t)j * R);
    const long long sj = SQ ? 0 : s[j];
#pragma unroll
    for (int b = 0; b < 4; ++b) { const int v = (int)(int8_t)(w >> (8 * b)); acc[b] += SQ ? (long long)(v * v) : (long long)v * sj; }
  }
#pragma unroll
  for (int b = 0; b < 4; ++b) red[g][4 * tx + b] = acc[b];
  __syncthreads();
  if (threadIdx.x < 128) {
    long long v = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) v += red[k][threadIdx.x];
    atomicAdd(reinterpret_cast<unsigned long long *>(out + r0 + threadIdx.x), (unsigned long long)v);
  }
}
__global__ __launch_bounds__(256) void k_kfin_xs(const int8_t *X, int R, int64_t p, const int32_t *s, int64_t cols, long long *rs) {
  kfin_rows<false>(X, R, p, s, cols, rs);
}
__global__ __launch_bounds__(256) void k_kfin2_rowsq(const int8_t *X, int R, int64_t p, int64_t cols, long long *q) {
  kfin_rows<true>(X, R, p, nullptr, cols, q);
}

__global__ void k_kfin_diag(const long long *G, int64_t ldg, int n, long long *diag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) diag[i] = G[(size_t)i * ldg + i];
}

// sum over all i != j of sqrt(G_ii + G_jj - 2 G_ij) (EigenGAU's normaliser): fixed grid, fixed tree -- the same bits on every call
__global__ __launch_bounds__(256) void k_kfin_sumd_stage1(const long long *G, int64_t ldg, const long long *diag, int n, double *part) {
  __shared__ double red[4];
  const int64_t total = (int64_t)n * n;
  double v = 0.0;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = idx / n, j = idx - i * n;
    if (i != j) v += sqrt((double)(diag[i] + diag[j] - 2 * G[(size_t)i * ldg + j]));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_kfin_sumd_stage2(const double *part, int nparts, double *out) {
  __shared__ double red[256];
  double v = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) v += part[i];
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) { if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
  if (threadIdx.x == 0) *out = red[0];
}

// The element-wise finish, in place: the int64 G_ij becomes the double K_ij.  An element needs G_ij, the two diagonal entries (copied out
// before), the two entries of X s and scalars; every expression is symmetric in (i, j) operand by operand, so K is exactly symmetric.
// cen: the centred product ZZ'_ij = G_ij - (r_i + r_j) + c, r = (X s) / n, c = sum_j mean_j^2.
struct KfinArgs {
  long long *G; int64_t ldg; int n; int kind, cen;
  const long long *diag, *rs;
  double ninv, c;     // 1 / n; sum_j (s_j / n)^2
  double scale;       // GRM: 1 / D is NOT used (the reference divides): D; GAU: md; EIGEN_GRM / EIGEN_ARC: 1 / mean(diag); EIGEN_GAU: t
};
__device__ __forceinline__ double kfin_zz(const KfinArgs &a, long long g, int i, int j) {
  double v = (double)g;
  if (a.cen) v = v - ((double)a.rs[i] * a.ninv + (double)a.rs[j] * a.ninv) + a.c;
  return v;
}
__global__ __launch_bounds__(256) void k_kfin_apply(const KfinArgs a) {
  const int64_t total = (int64_t)a.n * a.n;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / a.n), j = (int)(idx - (int64_t)i * a.n);
    long long *gp = a.G + (size_t)i * a.ldg + j;
    const long long g = *gp;
    double k;
    switch (a.kind) {
      case KFIN_GRM: k = kfin_zz(a, g, i, j) / a.scale; break;
      case KFIN_GAU: k = exp(-(double)(a.diag[i] + a.diag[j] - 2 * g) / a.scale); break;
      case KFIN_EIGEN_GRM: k = (kfin_zz(a, g, i, j) + (i == j ? 1.0 : 0.0)) * a.scale; break;
      case KFIN_EIGEN_GAU: k = exp(a.scale * (i == j ? 0.0 : sqrt((double)(a.diag[i] + a.diag[j] - 2 * g)))); break;
      default: {   // KFIN_EIGEN_ARC; the literals as the reference writes them
        const double aii = kfin_zz(a, a.diag[i], i, i) * a.scale, ajj = kfin_zz(a, a.diag[j], j, j) * a.scale, aij = kfin_zz(a, g, i, j) * a.scale;
        const double nrm = sqrt(aii * ajj * 1.001), th = acos(aij / nrm);
        k = nrm / 3.1416 * (sin(th) + (3.1416 - th) * cos(th));
      }
    }
    *reinterpret_cast<double *>(gp) = k;
  }
}

// ---- the founder-by-sample finishes (EigenArcZ / EigenGauZ) ------------------------------------------------------------------------------
enum { KFIN2_ARC = 0, KFIN2_GAU = 1 };
// One element of either kind.  The literals as the reference writes them (3.14159 here, not EigenARC's 3.1416).
// ARC: a = the product centred by the founders' column means, da and db the two centred squared norms; the value before Kscalar.
__host__ __device__ inline double kfin2_arc(double a, double da, double db) {
  const double nrm = sqrt(da * db * 1.001);
  double t = acos(a / nrm);
  t = nrm * (sin(t) + (3.14159 - t) * cos(t));
  return t / 3.14159;
}
// The element-wise finish of K_ff (same = 1: rows and columns are both the founders, zero distance on the diagonal) and of K_fs, in place:
// the int64 G_ij becomes the double K_ij.  A row brings its founder's terms, a column its own; in K_ff both come from the same arrays and
// every expression is symmetric in (i, j) operand by operand, so K_ff is exactly symmetric.
struct Kfin2Args {
  long long *G; int64_t ldg; int nr, nc; int kind, same;
  const long long *irow, *icol;   // GAU: G_ff[i][i]; the column's squared norm (K_ff: G_ff[j][j]; K_fs: q_s,j)
  const double *rrow, *rcol;      // ARC: r_f,i = (X_f s)_i / n_f; the column's (K_ff: r_f,j; K_fs: r_s,j = (X_s s)_j / n_f)
  const double *drow, *dcol;      // ARC: the centred squared norms d_f,i; d_f,j or d_s,j
  double c, scale;                // ARC: sum_j mean_j^2, Kscalar; GAU: -, t
};
__global__ __launch_bounds__(256) void k_kfin2_apply(const Kfin2Args a) {
  const int64_t total = (int64_t)a.nr * a.nc;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / a.nc), j = (int)(idx - (int64_t)i * a.nc);
    long long *gp = a.G + (size_t)i * a.ldg + j;
    const long long g = *gp;
    double k;
    if (a.kind == KFIN2_GAU) k = exp(((a.same && i == j) ? 0.0 : sqrt((double)(a.irow[i] + a.icol[j] - 2 * g))) * a.scale);
    else k = kfin2_arc((double)g - (a.rrow[i] + a.rcol[j]) + a.c, a.drow[i], a.dcol[j]) * a.scale;
    *reinterpret_cast<double *>(gp) = k;
  }
}

}  // namespace bwgr
