// bwgr_amd/csrc/panel.hip.h -- the kernels on a resident panel that every family shares: the device helpers (wave_sum, block_sum, xval), the
// upload conversion, the column statistics and the two-stage sums, the Gram family, the two-stage X * coef, the row gathers, the column
// permutation of mrr and the EM family, the centring check, and the synthetic genotypes and variates of the test hooks.  Part of bwgr_hip.hip,
// which includes it after sweep.hip.h and rng.hip.h (xoff, philox4x32_10, Rng) and before every host function; it defines no host function.
// ------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
// block-wide sum; result valid in every thread.  red must hold >= 17 doubles.
__device__ inline double block_sum(double v, double *red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) { double s = 0; for (int w = 0; w < nw; ++w) s += red[w]; red[16] = s; }
  __syncthreads();
  return red[16];
}

__device__ __forceinline__ float xval(const int8_t *X, int64_t i) { return (float)X[i]; }
__device__ __forceinline__ float xval(const float *X, int64_t i) { return X[i]; }

// ---- upload conversion: src (n x p, ldx) -> X (ld x p), zero padded rows ----
template <typename ST, typename XT>
__global__ void k_convert(const ST *src, int64_t ldx, XT *X, int64_t ld, int n, int64_t j0, int64_t ncols, int R, int64_t p) {
  const int64_t total = ncols * ld;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t jj = idx / ld, i = idx - jj * ld;
    XT v = (XT)0;
    if (i < n) v = (XT)src[jj * ldx + i];
    X[xoff(i, j0 + jj, R, p)] = v;
  }
}

__global__ void k_f2d(const float *src, double *dst, int64_t n, int64_t ld) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ld; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (i < n) ? (double)src[i] : 0.0;
}
__global__ void k_d2f(const double *src, float *dst, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = (float)src[i];
}

// ---- a10: xx[j] = |X_j|^2, vx[j] = fvar(X_j)   (src/Rcpp20260726ai.cpp:7-9, 593-597); one wave per column ----
template <typename XT>
__global__ void k_stats(const XT *X, int R, int n, int p, float *xx, float *vx) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= p) return;
  double s1 = 0, s2 = 0;
  for (int i = lane; i < n; i += 64) { const float v = xval(X, xoff(i, j, R, p)); s1 += (double)v; s2 += (double)v * (double)v; }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  s1 = __shfl(s1, 0, 64); s2 = __shfl(s2, 0, 64);
  const float mean = (float)(s1 / (double)n);
  double sv = 0;
  for (int i = lane; i < n; i += 64) { const float dev = xval(X, xoff(i, j, R, p)) - mean; const float sq = dev * dev; sv += (double)sq; }
  sv = wave_sum(sv);
  if (lane == 0) { xx[j] = (float)s2; vx[j] = (float)(sv / (double)(float)(n - 1)); }
}

// ---- implicit centring of an int8 panel (bwgr_panel_set_centred): s_j = sum_i x_ij exactly, and the centred column's squared norm
// sum_i (x_ij - s_j / n)^2 = sum x^2 - s_j^2 / n from exact integer sums, rounded to float once (the reference would form it from the centred
// float column, X.colwise().squaredNorm(), src/Rcpp20260726ai.cpp:593-594); one wave per column ----
__global__ void k_colsum_i8(const int8_t *X, int R, int n, int p, int32_t *csum, float *xxc) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= p) return;
  long long s1 = 0, s2 = 0;
  for (int i = lane; i < n; i += 64) { const int v = (int)X[xoff(i, j, R, p)]; s1 += v; s2 += v * v; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_down(s1, o, 64); s2 += __shfl_down(s2, o, 64); }
  if (lane == 0) { csum[j] = (int32_t)s1; xxc[j] = (float)((double)s2 - (double)s1 * (double)s1 / (double)n); }
}
// sum_j s_j coef_j / n  (one workgroup, fixed order): what the centred columns take off X * coef
__global__ __launch_bounds__(1024) void k_cen_dot(const int32_t *csum, const float *coef, int64_t p, double ninv, double *out) {
  __shared__ double red[1024];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int64_t j = t; j < p; j += 1024) s = fma((double)csum[j], (double)coef[j], s);
  red[t] = s;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if (t < o) red[t] += red[t + o]; __syncthreads(); }
  if (t == 0) *out = red[0] * ninv;
}

// deterministic two-stage sum of a float vector into a double
__global__ void k_sum_stage1(const float *v, int64_t n, double *part) {
  __shared__ double red[17];
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += (double)v[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void k_sum_stage2(const double *part, int nparts, float *out_f) {
  __shared__ double red[17];
  double s = 0;
  for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) *out_f = (float)s;
}

// ---- block-diagonal Gram G_B = X_B' X_B (setup; exact int32 for int8 genotypes) ----
// 256 threads as a 16 x 16 grid, thread (tj,tk) owns G[tj+16a][tk+16c], a,c < m/16.
template <int TJ>
__global__ __launch_bounds__(256) void k_gram_i8(const int8_t *X, int64_t ld, int R, int p, int m, int32_t *gram) {
  constexpr int RC = 128, RW = RC / 4 + 1;  // rows per chunk, dwords per column in LDS (padded)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t *tile = reinterpret_cast<int32_t *>(smem);
  const int blk = blockIdx.x, j0 = blk * m, mB = min(m, p - j0);
  const int tj = threadIdx.x >> 4, tk = threadIdx.x & 15;
  int32_t acc[TJ][TJ];
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) acc[a][c] = 0;
  for (int64_t r0 = 0; r0 < ld; r0 += RC) {
    __syncthreads();
    for (int c = threadIdx.x; c < m * (RC / 4); c += 256) {
      const int jj = c / (RC / 4), w = c - jj * (RC / 4);
      int32_t v = 0;
      if (jj < mB) v = *reinterpret_cast<const int32_t *>(X + xoff(r0 + 4 * w, j0 + jj, R, p));
      tile[jj * RW + w] = v;
    }
    __syncthreads();
    for (int w = 0; w < RC / 4; ++w) {
      int32_t av[TJ], bv[TJ];
#pragma unroll
      for (int a = 0; a < TJ; ++a) { av[a] = tile[(tj + 16 * a) * RW + w]; bv[a] = tile[(tk + 16 * a) * RW + w]; }
#pragma unroll
      for (int a = 0; a < TJ; ++a)
#pragma unroll
        for (int c = 0; c < TJ; ++c) acc[a][c] = __builtin_amdgcn_sdot4(av[a], bv[c], acc[a][c], false);
    }
  }
  int32_t *g = gram + (size_t)blk * m * m;
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) g[(size_t)(tj + 16 * a) * m + (tk + 16 * c)] = acc[a][c];
}

// m = 128: the same blocks on the matrix cores.  out[blk][i][j] = X_{(blk-dist)m+i} . X_{blk*m+j} (dist = 0: the diagonal block),
// exact in the int32 accumulators.  One workgroup of four waves per block; wave w owns the 64 x 64 quadrant (4 x 4 tiles of
// 16 x 16); v_mfma_i32_16x16x64_i8 takes, per lane (m16, grp), the 16 bytes of marker 16t + m16 at rows 64kk + 16grp .. +15 for
// both operands -- straight from the slab-major panel, whose markers are contiguous along the rows -- and returns
// out[16ti + 4grp + reg][16tj + m16].  Per 64 rows a wave issues 8 loads and 16 MFMAs (the sdot4 kernels above ran at
// 0.75 TB/s: one dword per thread per load and an LDS round trip).
__global__ __launch_bounds__(256) void k_gram_mfma_i8(const int8_t *X, int64_t ld, int R, int p, int32_t *out, int dist) {
  constexpr int m = 128;
  const int blk = blockIdx.x + dist, ia0 = (blk - dist) * m, jb0 = blk * m;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m16 = lane & 15, grp = lane >> 4;
  const int ti0 = 4 * (wave >> 1), tj0 = 4 * (wave & 1);
  s2_v4i acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[a][c] = s2_v4i{0, 0, 0, 0};
  // markers past the panel (last block) are read at a clamped column and zeroed
  int ca[4], cb[4]; bool oka[4], okb[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int ja = ia0 + 16 * (ti0 + t) + m16, jb = jb0 + 16 * (tj0 + t) + m16;
    oka[t] = ja < p; okb[t] = jb < p; ca[t] = min(ja, p - 1); cb[t] = min(jb, p - 1);
  }
  const s2_v4i zero = {0, 0, 0, 0};
  // software pipeline: the operands of step k+1 are requested before the sixteen MFMAs of step k
  auto load_step = [&](int64_t r0, s2_v4i (&av)[4], s2_v4i (&bv)[4]) {
    const int64_t sl = r0 / R;
    const size_t roff = (size_t)(r0 - sl * R) + 16 * grp;
    const int8_t *sb = X + (size_t)sl * p * R + roff;       // slab base + row offset; marker j adds j*R
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      av[t] = *reinterpret_cast<const s2_v4i *>(sb + (size_t)ca[t] * R);
      bv[t] = *reinterpret_cast<const s2_v4i *>(sb + (size_t)cb[t] * R);
    }
  };
  s2_v4i av[4], bv[4], an[4], bn[4];
  load_step(0, av, bv);
  for (int64_t r0 = 0; r0 < ld; r0 += 64) {
    const bool more = r0 + 64 < ld;
    load_step(more ? r0 + 64 : r0, an, bn);                 // (the last step reloads its own operands: harmless)
#pragma unroll
    for (int t = 0; t < 4; ++t) { av[t] = oka[t] ? av[t] : zero; bv[t] = okb[t] ? bv[t] : zero; }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[a][c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[a], bv[c], acc[a][c], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < 4; ++t) { av[t] = an[t]; bv[t] = bn[t]; }
  }
  int32_t *g = out + (size_t)blk * m * m;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg)
        g[(size_t)(16 * (ti0 + a) + 4 * grp + reg) * m + 16 * (tj0 + c) + m16] = acc[a][c][reg];
}

// off-diagonal blocks for the pipelined sweep: gramx[blk][k][j] = X_{(blk-dist)m+k} . X_{blk*m+j}, blk >= dist (dist = 1, 2)
template <int TJ>
__global__ __launch_bounds__(256) void k_gramx_i8(const int8_t *X, int64_t ld, int R, int p, int m, int32_t *gramx, int dist) {
  constexpr int RC = 128, RW = RC / 4 + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t *ta = reinterpret_cast<int32_t *>(smem), *tb = ta + (size_t)m * RW;
  const int blk = blockIdx.x + dist, ja0 = (blk - dist) * m, jb0 = blk * m, mBb = min(m, p - jb0);
  const int tj = threadIdx.x >> 4, tk = threadIdx.x & 15;
  int32_t acc[TJ][TJ];
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) acc[a][c] = 0;
  for (int64_t r0 = 0; r0 < ld; r0 += RC) {
    __syncthreads();
    for (int c = threadIdx.x; c < m * (RC / 4); c += 256) {
      const int jj = c / (RC / 4), w = c - jj * (RC / 4);
      ta[jj * RW + w] = *reinterpret_cast<const int32_t *>(X + xoff(r0 + 4 * w, ja0 + jj, R, p));
      tb[jj * RW + w] = (jj < mBb) ? *reinterpret_cast<const int32_t *>(X + xoff(r0 + 4 * w, jb0 + jj, R, p)) : 0;
    }
    __syncthreads();
    for (int w = 0; w < RC / 4; ++w) {
      int32_t av[TJ], bv[TJ];
#pragma unroll
      for (int a = 0; a < TJ; ++a) { av[a] = ta[(tj + 16 * a) * RW + w]; bv[a] = tb[(tk + 16 * a) * RW + w]; }
#pragma unroll
      for (int a = 0; a < TJ; ++a)
#pragma unroll
        for (int c = 0; c < TJ; ++c) acc[a][c] = __builtin_amdgcn_sdot4(av[a], bv[c], acc[a][c], false);
    }
  }
  int32_t *g = gramx + (size_t)blk * m * m;
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) g[(size_t)(tj + 16 * a) * m + (tk + 16 * c)] = acc[a][c];
}
template <int TJ>
__global__ __launch_bounds__(256) void k_gramx_f32(const float *X, int64_t ld, int R, int p, int m, double *gramx, int dist) {
  constexpr int RC = 64, RW = RC + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *ta = reinterpret_cast<float *>(smem), *tb = ta + (size_t)m * RW;
  const int blk = blockIdx.x + dist, ja0 = (blk - dist) * m, jb0 = blk * m, mBb = min(m, p - jb0);
  const int tj = threadIdx.x >> 4, tk = threadIdx.x & 15;
  double acc[TJ][TJ];
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) acc[a][c] = 0.0;
  for (int64_t r0 = 0; r0 < ld; r0 += RC) {
    __syncthreads();
    for (int c = threadIdx.x; c < m * RC; c += 256) {
      const int jj = c / RC, w = c - jj * RC;
      ta[jj * RW + w] = X[xoff(r0 + w, ja0 + jj, R, p)];
      tb[jj * RW + w] = (jj < mBb) ? X[xoff(r0 + w, jb0 + jj, R, p)] : 0.0f;
    }
    __syncthreads();
    for (int w = 0; w < RC; ++w) {
      double av[TJ], bv[TJ];
#pragma unroll
      for (int a = 0; a < TJ; ++a) { av[a] = (double)ta[(tj + 16 * a) * RW + w]; bv[a] = (double)tb[(tk + 16 * a) * RW + w]; }
#pragma unroll
      for (int a = 0; a < TJ; ++a)
#pragma unroll
        for (int c = 0; c < TJ; ++c) acc[a][c] = fma(av[a], bv[c], acc[a][c]);
    }
  }
  double *g = gramx + (size_t)blk * m * m;
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) g[(size_t)(tj + 16 * a) * m + (tk + 16 * c)] = acc[a][c];
}

template <int TJ>
__global__ __launch_bounds__(256) void k_gram_f32(const float *X, int64_t ld, int R, int p, int m, double *gram) {
  constexpr int RC = 64, RW = RC + 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float *tile = reinterpret_cast<float *>(smem);
  const int blk = blockIdx.x, j0 = blk * m, mB = min(m, p - j0);
  const int tj = threadIdx.x >> 4, tk = threadIdx.x & 15;
  double acc[TJ][TJ];
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) acc[a][c] = 0.0;
  for (int64_t r0 = 0; r0 < ld; r0 += RC) {
    __syncthreads();
    for (int c = threadIdx.x; c < m * RC; c += 256) {
      const int jj = c / RC, w = c - jj * RC;
      tile[jj * RW + w] = (jj < mB) ? X[xoff(r0 + w, j0 + jj, R, p)] : 0.0f;
    }
    __syncthreads();
    for (int w = 0; w < RC; ++w) {
      double av[TJ], bv[TJ];
#pragma unroll
      for (int a = 0; a < TJ; ++a) { av[a] = (double)tile[(tj + 16 * a) * RW + w]; bv[a] = (double)tile[(tk + 16 * a) * RW + w]; }
#pragma unroll
      for (int a = 0; a < TJ; ++a)
#pragma unroll
        for (int c = 0; c < TJ; ++c) acc[a][c] = fma(av[a], bv[c], acc[a][c]);
    }
  }
  double *g = gram + (size_t)blk * m * m;
#pragma unroll
  for (int a = 0; a < TJ; ++a)
#pragma unroll
    for (int c = 0; c < TJ; ++c) g[(size_t)(tj + 16 * a) * m + (tk + 16 * c)] = acc[a][c];
}

// strict upper triangle of the diagonal Gram blocks, row-packed: entry (k, j>k) at k(m-1) - k(k-1)/2 + (j-k-1)
template <typename GT>
__global__ void k_gram_pack(const GT *gram, GT *gramp, int m, int pstride, int64_t nblocks) {
  const int64_t blk = blockIdx.x;
  const GT *G = gram + (size_t)blk * m * m;
  GT *P = gramp + (size_t)blk * pstride;
  for (int e = threadIdx.x; e < m * m; e += blockDim.x) {
    const int k = e / m, j = e - k * m;
    if (j > k) P[k * (m - 1) - k * (k - 1) / 2 + (j - k - 1)] = G[e];
  }
  for (int e = m * (m - 1) / 2 + threadIdx.x; e < pstride; e += blockDim.x) P[e] = (GT)0;
}

// 16-bit copies of the packed and the distance-1 cross Gram blocks for the k_sweep2 sequencer (half the bytes through its
// CU per block); *bad is set when an entry does not fit, and the sequencer then stages the 32-bit arrays
// largest |x| of an int8 panel (k_sweep3's integer sums are sized by it)
__global__ void k_absmax_i8(const int8_t *X, size_t count, int *out) {
  int mx = 0;
  for (size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 16; i < count; i += (size_t)gridDim.x * blockDim.x * 16) {
    const uint4 v = *reinterpret_cast<const uint4 *>(X + i);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int c = 0; c < 4; ++c) { const int x = (int)(int8_t)(w[q] >> (8 * c)); mx = max(mx, x < 0 ? -x : x); }
  }
  atomicMax(out, mx);
}
__global__ void k_gram_narrow(const int32_t *src, uint16_t *dst, int64_t count, int *bad) {
  int any = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t v = src[i];
    any |= (v < 0 || v > 65535);
    dst[i] = (uint16_t)v;
  }
  if (any) *bad = 1;
}

// partial[c][i] = sum_{j in column chunk c} x_ij * coef_j   (fp64), 4 rows per thread
template <typename XT, typename CT>
__global__ __launch_bounds__(256) void k_gemv_part(const XT *X, int64_t ld, int R, int p, const CT *coef, int cols_per_chunk, double *part) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i0 >= ld) return;
  const int c = blockIdx.y;
  const int ja = c * cols_per_chunk, jb = min(p, ja + cols_per_chunk);
  double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  for (int j = ja; j < jb; ++j) {
    const double cj = (double)coef[j];
    if (cj == 0.0) continue;
    const XT *xp = X + xoff(i0, j, R, p);
    float x0, x1, x2, x3;
    if constexpr (sizeof(XT) == 1) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(xp);
      x0 = (float)(int8_t)(w & 0xFF); x1 = (float)(int8_t)((w >> 8) & 0xFF); x2 = (float)(int8_t)((w >> 16) & 0xFF); x3 = (float)(int8_t)(w >> 24);
    } else {
      const float4 v = *reinterpret_cast<const float4 *>(xp);
      x0 = v.x; x1 = v.y; x2 = v.z; x3 = v.w;
    }
    a0 = fma((double)x0, cj, a0); a1 = fma((double)x1, cj, a1); a2 = fma((double)x2, cj, a2); a3 = fma((double)x3, cj, a3);
  }
  double *o = part + (int64_t)c * ld + i0;
  o[0] = a0; o[1] = a1; o[2] = a2; o[3] = a3;
}
// int8 panels: 16 rows per thread (one 16-byte load per marker), four markers' loads in flight, no data-dependent branch --
// the 4-rows-per-thread loop above with its skip of zero coefficients waited for every load and ran at 1.1 TB/s
template <typename CT>
__global__ __launch_bounds__(256) void k_gemv_part_i8(const int8_t *X, int64_t ld, int R, int p, const CT *coef, int cols_per_chunk, double *part) {
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
  if (i0 >= ld) return;
  const int c = blockIdx.y;
  const int ja = c * cols_per_chunk, jb = min(p, ja + cols_per_chunk);
  const int8_t *base = X + xoff(i0, 0, R, p);          // marker j of this slab: base + j*R (R is a multiple of 128)
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
#define GEMV_ADD(w_, cj_, k0_) { \
    acc[(k0_) + 0] = fma((double)(int)(int8_t)((w_) & 0xFF), cj_, acc[(k0_) + 0]); acc[(k0_) + 1] = fma((double)(int)(int8_t)(((w_) >> 8) & 0xFF), cj_, acc[(k0_) + 1]); \
    acc[(k0_) + 2] = fma((double)(int)(int8_t)(((w_) >> 16) & 0xFF), cj_, acc[(k0_) + 2]); acc[(k0_) + 3] = fma((double)((int)(w_) >> 24), cj_, acc[(k0_) + 3]); }
#define GEMV_COL(v_, cj_) { GEMV_ADD((v_).x, cj_, 0) GEMV_ADD((v_).y, cj_, 4) GEMV_ADD((v_).z, cj_, 8) GEMV_ADD((v_).w, cj_, 12) }
  int j = ja;
  for (; j + 4 <= jb; j += 4) {
    const uint4 v0 = *reinterpret_cast<const uint4 *>(base + (size_t)j * R), v1 = *reinterpret_cast<const uint4 *>(base + (size_t)(j + 1) * R);
    const uint4 v2 = *reinterpret_cast<const uint4 *>(base + (size_t)(j + 2) * R), v3 = *reinterpret_cast<const uint4 *>(base + (size_t)(j + 3) * R);
    const double c0 = (double)coef[j], c1 = (double)coef[j + 1], c2 = (double)coef[j + 2], c3 = (double)coef[j + 3];
    GEMV_COL(v0, c0) GEMV_COL(v1, c1) GEMV_COL(v2, c2) GEMV_COL(v3, c3)
  }
  for (; j < jb; ++j) { const uint4 v0 = *reinterpret_cast<const uint4 *>(base + (size_t)j * R); const double c0 = (double)coef[j]; GEMV_COL(v0, c0) }
#undef GEMV_COL
#undef GEMV_ADD
  double *o = part + (int64_t)c * ld + i0;
#pragma unroll
  for (int k = 0; k < 16; ++k) o[k] = acc[k];
}
__global__ void k_hat_finish(const double *part, int64_t ld, int nchunks, int n, float MU, float *hat, const double *cen_off = nullptr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = cen_off ? -*cen_off : 0.0;   // (implicitly centred columns: X_c B = X B - sum_j mean_j B_j)
  for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * ld + i];
  const float f = (float)s;
  hat[i] = f + MU;
}

// ---- bagging (bag != 1): KMUP2 works on a row subsample (src/Rcpp20260726ai.cpp:49-57) ----
// rows Use[0..nb) of the base panel -> a panel of nb rows (both slab-major, each with its own slab height)
template <typename XT>
__global__ void k_gather_rows(const XT *Xb, int Rb, const int *use, int nb, XT *Xo, int Ro, int64_t ldo, int64_t p) {
  const int64_t total = p * ldo;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx / ldo, i = idx - j * ldo;
    XT v = (XT)0;
    if (i < nb) v = Xb[xoff(use[i], j, Rb, p)];
    Xo[xoff(i, j, Ro, p)] = v;
  }
}
// int8 panels: a workgroup stages whole columns in LDS with 16-byte loads, picks the subsample's bytes there and writes the
// bagged panel with 16-byte stores (the element-wise kernel above moved one byte per load and ran at 0.6 TB/s)
__global__ __launch_bounds__(256) void k_gather_rows_i8(const int8_t *Xb, int Rb, int64_t ldb, const int *use, int nb, int8_t *Xo, int Ro,
                                                         int64_t ldo, int64_t p, int mpw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char col[];   // mpw columns of ldb bytes
  const int64_t j0 = (int64_t)blockIdx.x * mpw;
  const int nm = (int)min((int64_t)mpw, p - j0);
  const int cin = (int)(ldb / 16), cout = (int)(ldo / 16);
  for (int c = threadIdx.x; c < nm * cin; c += 256) {
    const int jj = c / cin, ci = c - jj * cin;
    const int64_t i = 16 * (int64_t)ci;
    reinterpret_cast<uint4 *>(col + (size_t)jj * ldb)[ci] = *reinterpret_cast<const uint4 *>(Xb + xoff(i, j0 + jj, Rb, p));
  }
  __syncthreads();
  for (int co = threadIdx.x; co < cout; co += 256) {   // the 16 row indices of an output chunk serve every column of the group
    int ui[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int i = 16 * co + k; ui[k] = (i < nb) ? use[i] : -1; }
    for (int jj = 0; jj < nm; ++jj) {
      const unsigned char *cj = col + (size_t)jj * ldb;
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t v = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { const int u = ui[4 * q + k]; v |= ((u >= 0) ? (uint32_t)cj[u] : 0u) << (8 * k); }
        w[q] = v;
      }
      *reinterpret_cast<uint4 *>(Xo + xoff(16 * (int64_t)co, j0 + jj, Ro, p)) = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}
// the columns of a slab-major panel in another order (mrr's and the EM family's sweep order): one pass over X
__global__ void k_permute_cols(const uint4 *__restrict__ X, uint4 *__restrict__ Xp, const int32_t *__restrict__ order,
                               int64_t p, int K, int cps) {
  // slab-major layout: (slab s, marker j) is one segment of R elements = cps 16-byte chunks
  const int64_t total = (int64_t)K * p * cps;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < total; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t seg = c / cps;
    const int off = (int)(c - seg * cps);
    const int64_t sl = seg / p, jj = seg - sl * p;
    Xp[c] = X[(sl * p + order[jj]) * cps + off];
  }
}
// are a panel's columns centred?  (bwgr_panel_centred: from the panel's own statistics, mean_j^2 = (xx_j - (n - 1) vx_j) / n)
__global__ void k_uncentred(const float *xx, const float *vx, int64_t p, double n, int *flag) {
  int any = 0;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < p; j += (int64_t)gridDim.x * blockDim.x) {
    const double v = (double)vx[j], m2 = fmax(0.0, ((double)xx[j] - (n - 1.0) * v) / n);
    any |= (m2 > 1e-6 * v + 1e-30);
  }
  if (any) *flag = 1;
}

// ---- synthetic genotypes: 4 rows per thread ----
__global__ void k_synth(int8_t *X, int64_t ld, int n, int64_t p, int64_t col0, uint32_t k0, uint32_t k1, float *freq) {
  const int64_t quads = ld / 4;
  const int64_t total = p * quads;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t j = idx / quads, q = idx - j * quads;
    const uint32_t jg = (uint32_t)(col0 + j);
    const uint4 fj = philox4x32_10(jg, 0u, 33u, 0u, k0, k1);
    const float f = 0.05f + 0.45f * ((float)(fj.x >> 8) * (1.0f / 16777216.0f));
    const uint32_t thr = (uint32_t)(f * 16777216.0f);
    if (q == 0 && freq) freq[j] = f;
    const uint4 a = philox4x32_10((uint32_t)q, jg, 32u, 0u, k0, k1);
    const uint4 c = philox4x32_10((uint32_t)q, jg, 32u, 1u, k0, k1);
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
    uint32_t packed = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      uint32_t g = ((w[2 * r] >> 8) < thr) + ((w[2 * r + 1] >> 8) < thr);
      if (q * 4 + r >= n) g = 0;
      packed |= g << (8 * r);
    }
    *reinterpret_cast<uint32_t *>(X + j * ld + q * 4) = packed;
  }
}

__global__ void k_debug_variates(Rng g, int kind, double nu, uint32_t marker0, uint32_t iter, uint32_t purpose, int count, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t mk = marker0 + (uint32_t)i;
  double v;
  if (kind == 0) v = rng_normal(g, mk, iter, purpose, 0);
  else if (kind == 1) v = rng_uniform(g, mk, iter, purpose, 0);
  else v = rng_chisq(g, nu, mk, iter, purpose);
  out[i] = v;
}

}  // namespace
