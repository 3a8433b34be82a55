// bwgr_amd: the transpose product of the resident int8 panel, out = X'A or X_c'A (bwgr_panel_xta) -- marker effects
// from row coefficients: mrr_svd's beta = W_c'(U D^-1 b), SNP effects from kernel-model GEBVs.
//
//   k_xta_stage   A (n x k, column stride lda) -> As[group][ld][16]: the traits in groups of XTA_KT, a row's sixteen values side by side,
//                 zeros on the rows n .. ld-1 and on the traits past k
//   k_xta_asum    s_t = sum_i a_it for the implicit centring: 256 partial sums (partial q takes the rows i = q, q + 256, ... in ascending order),
//                 then the partials in ascending q
//   k_xta         out[j][t] = sum_i x_ij a_it, and with centre fma(-xbar_j, s_t, .), xbar_j = (exact integer column sum) / n
//
// k_xta's tile.  A workgroup of 256 threads owns XTA_WGC = 64 whole columns, all ld rows of them, and one trait group; thread (cg, rl) =
// (tid / 16, tid % 16) keeps the 4 x 16 sums of columns 4 cg .. 4 cg + 3 over the rows of its row lane in registers.  The rows go by in tiles
// of XTA_RT = 128 (a slab height is a multiple of 128, so a tile lies in one slab and a column's share of it is 128 contiguous bytes): row
// lane rl takes the tile's rows 8 rl .. 8 rl + 7, one 8-byte load per column, so the sixteen row lanes of a column read one whole 128-byte line.
// The tile of A is staged in LDS, a row's sixteen doubles in one 144-byte record, the records in the order the row lanes read them (record
// 16 u + rl holds row 8 rl + u): at step u the sixteen row lanes read sixteen consecutive records, which the 144-byte stride spreads over
// all sixteen 16-byte slots of the LDS's 256-byte row, and the four column groups of a wave read the same records (a broadcast).  One
// 128-byte row of A read from LDS feeds 4 x 16 = 64 FMAs of the lane.
//
// The order of a sum: row lane rl adds its rows in ascending order (tiles ascending, u ascending), then the sixteen row lanes are added by an
// exchange over lane distances 8, 4, 2, 1 (the same tree of additions for every output).  It depends on ld alone -- not on p, the grid, the column's place in its workgroup or the trait's
// place in its group -- and nothing is accumulated by atomics.  Pad rows of X and of As are zero, so no row mask is needed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bwgr {

static constexpr int XTA_KT = 16;        // traits per group: one pass over X per group
static constexpr int XTA_CW = 4;         // columns per thread
static constexpr int XTA_RL = 16;        // row lanes per column group
static constexpr int XTA_RT = 128;       // rows per tile
static constexpr int XTA_RPT = XTA_RT / XTA_RL;              // rows per thread and tile: one 8-byte load per column
static constexpr int XTA_WGC = 256 / XTA_RL * XTA_CW;        // columns per workgroup
static constexpr int XTA_WVC = 64 / XTA_RL * XTA_CW;         // columns per wave
static constexpr int XTA_AS = XTA_KT + 2;                    // doubles per staged row of A (144 bytes)
static constexpr int XTA_WG_MAX = 1024;                      // workgroups per trait group at most; a workgroup strides over the column blocks
static constexpr int XTA_LDS = XTA_RT * XTA_AS * 8;          // static LDS of k_xta
typedef double xta_d2 __attribute__((ext_vector_type(2)));
static_assert(XTA_RPT == 8, "a thread's share of a column and tile is one 8-byte load");

__global__ __launch_bounds__(256) void k_xta_stage(const double *__restrict__ A, int64_t lda, int64_t n, int64_t k, int64_t ld, int64_t ngroups,
                                                   double *__restrict__ As) {
  const int64_t total = ngroups * XTA_KT * ld;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int64_t tt = e / ld, i = e - tt * ld;           // tt: the trait, padded to whole groups
    const int64_t g = tt / XTA_KT, t = tt - g * XTA_KT;
    As[(size_t)(g * ld + i) * XTA_KT + t] = (i < n && tt < k) ? A[(size_t)tt * (size_t)lda + (size_t)i] : 0.0;
  }
}

// one workgroup per (padded) trait
__global__ __launch_bounds__(256) void k_xta_asum(const double *__restrict__ As, int64_t n, int64_t ld, double *__restrict__ sA) {
  __shared__ double part[256];
  const int64_t g = blockIdx.x / XTA_KT, t = blockIdx.x % XTA_KT;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += As[(size_t)(g * ld + i) * XTA_KT + t];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int q = 0; q < 256; ++q) a += part[q];
    sA[blockIdx.x] = a;
  }
}

struct XtaArgs {
  const int8_t *X; int R; int64_t p, ld, n;
  const double *As, *sA;      // [group][ld][16]; [group][16]
  int64_t k, nblk;            // traits; column blocks of XTA_WGC
  int centre;
  double *out; int64_t ldo;
};

// the next tile's share of a thread: eight rows of its four columns (zeros past the panel's last column) and its two pieces of the tile of A
__device__ __forceinline__ void xta_fetch(const XtaArgs &a, const double *Ag, int64_t j0, int64_t w, int off, int64_t i0, const int (&soff)[2],
                                          uint2 (&xn)[XTA_CW], xta_d2 (&an)[4]) {
#pragma unroll
  for (int c = 0; c < XTA_CW; ++c) {
    xn[c] = uint2{0u, 0u};
    if (j0 + c < a.p) xn[c] = *reinterpret_cast<const uint2 *>(a.X + (size_t)((w * a.p + j0 + c) * a.R + off));
  }
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const xta_d2 *s = reinterpret_cast<const xta_d2 *>(Ag + (size_t)i0 * XTA_KT + soff[m]);
    an[2 * m] = s[0]; an[2 * m + 1] = s[1];
  }
}

__global__ __launch_bounds__(256, 2) void k_xta(const XtaArgs a) {
  __shared__ __attribute__((aligned(16))) double at[XTA_RT * XTA_AS];
  const int tid = threadIdx.x, rl = tid & (XTA_RL - 1), cg = tid >> 4;
  const int64_t g = blockIdx.y;
  const double *Ag = a.As + (size_t)g * (size_t)a.ld * XTA_KT;
  // staging: piece q = tid + 256 m is the 32 bytes `part` of record q / 4; record 16 u + rl holds the tile's row 8 rl + u
  int soff[2], doff[2];
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = tid + 256 * m, rec = q >> 2, part = q & 3;             // four 32-byte pieces per record
    const int row = (rec & (XTA_RL - 1)) * XTA_RPT + (rec >> 4);
    soff[m] = row * XTA_KT + part * 4; doff[m] = rec * XTA_AS + part * 4;
  }
  for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
    const int64_t j0 = blk * XTA_WGC + cg * XTA_CW;
    double acc[XTA_CW][XTA_KT];
    int cs[XTA_CW];
#pragma unroll
    for (int c = 0; c < XTA_CW; ++c) {
      cs[c] = 0;
#pragma unroll
      for (int t = 0; t < XTA_KT; ++t) acc[c][t] = 0.0;
    }
    uint2 xn[XTA_CW];
    xta_d2 an[4];
    xta_fetch(a, Ag, j0, 0, rl * XTA_RPT, 0, soff, xn, an);
    int64_t w = 0; int off = 0;                            // the next tile's slab and its first row within the slab
    for (int64_t i0 = 0; i0 < a.ld; i0 += XTA_RT) {
      uint2 xr[XTA_CW];
#pragma unroll
      for (int c = 0; c < XTA_CW; ++c) xr[c] = xn[c];
      __syncthreads();   // the previous tile is consumed
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        xta_d2 *d = reinterpret_cast<xta_d2 *>(at + doff[m]);
        d[0] = an[2 * m]; d[1] = an[2 * m + 1];
      }
      off += XTA_RT;
      if (off == a.R) { off = 0; ++w; }
      if (i0 + XTA_RT < a.ld) xta_fetch(a, Ag, j0, w, off + rl * XTA_RPT, i0 + XTA_RT, soff, xn, an);
      __syncthreads();
#pragma unroll
      for (int c = 0; c < XTA_CW; ++c)
        cs[c] = __builtin_amdgcn_sdot4((int)xr[c].y, 0x01010101, __builtin_amdgcn_sdot4((int)xr[c].x, 0x01010101, cs[c], false), false);
#pragma unroll
      for (int u = 0; u < XTA_RPT; ++u) {
        const xta_d2 *ar = reinterpret_cast<const xta_d2 *>(at + (u * XTA_RL + rl) * XTA_AS);
        double av[XTA_KT];
#pragma unroll
        for (int t = 0; t < XTA_KT / 2; ++t) { const xta_d2 v = ar[t]; av[2 * t] = v.x; av[2 * t + 1] = v.y; }
#pragma unroll
        for (int c = 0; c < XTA_CW; ++c) {
          const unsigned word = u < 4 ? xr[c].x : xr[c].y;
          const double x = (double)(int)(int8_t)(word >> (8 * (u & 3)));
#pragma unroll
          for (int t = 0; t < XTA_KT; ++t) acc[c][t] = fma(x, av[t], acc[c][t]);
        }
      }
    }
    // The sixteen row lanes of a column group, by a halving exchange over lane distances 8, 4, 2, 1: at distance o a lane keeps the half of its
    // values that its bit o of rl selects, sends the other half to its partner and adds what the partner sends.  Row lane rl ends with the
    // four results 4 rl .. 4 rl + 3 of the 64 (column rl / 4 of the group, traits 4 (rl % 4) ..), each the same tree of additions.
    double *v = &acc[0][0];
#pragma unroll
    for (int h = XTA_CW * XTA_KT / 2, o = XTA_RL / 2; o >= 1; h >>= 1, o >>= 1) {
      const bool up = (rl & o) != 0;
#pragma unroll
      for (int i = 0; i < h; ++i) {
        const double keep = up ? v[h + i] : v[i], send = up ? v[i] : v[h + i];
        v[i] = keep + __shfl_xor(send, o, 64);
      }
    }
#pragma unroll
    for (int o = 1; o < XTA_RL; o <<= 1) {
#pragma unroll
      for (int c = 0; c < XTA_CW; ++c) cs[c] += __shfl_xor(cs[c], o, 64);
    }
    const int cc = rl >> 2;
    const int csum = cc == 0 ? cs[0] : cc == 1 ? cs[1] : cc == 2 ? cs[2] : cs[3];
    const int64_t j = j0 + cc;
    const double xbar = (double)csum / (double)a.n;
    if (j < a.p) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t tt = g * XTA_KT + (rl & 3) * 4 + m;
        if (tt < a.k) {
          double r = v[m];
          if (a.centre) r = fma(-xbar, a.sA[tt], r);
          a.out[(size_t)tt * (size_t)a.ldo + (size_t)j] = r;
        }
      }
    }
  }
}

}  // namespace bwgr
