// bwgr_amd: the residual of a design on a set of covariates, Zp = Z - X C with C = (X'X)^-1 X'Z over all n rows (MLM's projection,
// src/RcppEigen20230423.cpp:1287-1288) -- genotypes cleared of population-structure components, of year or location
// means.  Z is a resident int8 panel or an n x p fp64 matrix; X is n x f fp64, 1 <= f <= PROJ_FMAX.
//
//   k_proj_ztx   out[l][j] = sum_i z_ij x_il on a dense Z: k_xta's tile, thread layout and order of additions (xta.hip.h) with a column of
//                doubles where k_xta reads a column of bytes, so an integer-valued dense Z gives the bits its panel gives.  X goes through
//                k_xta_stage like k_xta's A.  (On a panel Z'X is k_xta itself, centre = 0.)
//   k_project    Zp[i][j] = the chain  acc = (double)z_ij;  for l = 0 .. f-1: acc = fma(-x_il, c_lj, acc)
// The f x f solve between the two is the host's (project_host.hip.h).
//
// k_project's tile.  A workgroup step is PROJ_T = 64 rows x 64 columns, like the train's (mrr_dense.hip.h).  Thread (ci, ri) = (tid / 16, tid % 16)
// owns the 4 x 4 elements of rows 4 ri .. 4 ri + 3 and columns 4 ci .. 4 ci + 3 in registers: the four rows of a panel column are one 32-bit
// load, and the four results of a column are 32 contiguous bytes of the output, so the sixteen row lanes of a column write 512 contiguous bytes.
// f goes by in pieces of at most PROJ_FP = 64: xs[l][row] holds the piece of the row tile of X and cs[l][column] the piece of the column block of
// C, fp doubles x 64 each -- 64 KB at fp = 64, so that two workgroups fit a compute unit, and less for a smaller f.  At step l a thread reads
// its four rows as two 16-byte LDS reads (the sixteen row lanes read 512 contiguous bytes: every bank once per pass) and its four columns as two
// more (one address per sixteen lanes: a broadcast), for sixteen FMAs.  A workgroup keeps its column block and walks the row tiles blockIdx.y,
// blockIdx.y + gridDim.y, ...; with one piece the block of C is staged once per workgroup.
//
// The order of a sum is the chain's: it depends on (i, j, f) alone -- not on the tiling, the slab height, the kind of Z or the other columns of the
// call.  Nothing is reduced across lanes or workgroups, and there are no atomics.  In place (out == Z) is safe: a thread reads an element before
// it writes it, and no other thread reads that element.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "xta.hip.h"

namespace bwgr {

static constexpr int PROJ_FMAX = 256;    // covariates at most
static constexpr int PROJ_T = 64;        // rows and columns of a workgroup step
static constexpr int PROJ_FP = 64;       // covariates per piece at most
static constexpr int PROJ_GY_MAX = 16;   // row-tile workgroups per column block at most
__host__ __device__ inline size_t proj_lds(int fp) { return sizeof(double) * 2 * (size_t)fp * PROJ_T; }

// ---- Z'X on a dense Z (n x p, column stride ldz); the rows from n on count as zero ----
struct ProjZtxArgs {
  const double *Z; int64_t ldz, n, p, ld;   // ld: n padded to XTA_RT
  const double *As;                         // X staged by k_xta_stage: [group][ld][16]
  int64_t f, nblk;
  double *out; int64_t ldo;                 // out[l * ldo + j]
};
__global__ __launch_bounds__(256) void k_proj_ztx(const ProjZtxArgs a) {
  __shared__ __attribute__((aligned(16))) double at[XTA_RT * XTA_AS];
  const int tid = threadIdx.x, rl = tid & (XTA_RL - 1), cg = tid >> 4;
  const int64_t g = blockIdx.y;
  const double *Ag = a.As + (size_t)g * (size_t)a.ld * XTA_KT;
  int soff[2], doff[2];   // k_xta's staging: piece q = tid + 256 m is the 32 bytes `part` of record q / 4; record 16 u + rl holds the tile's row 8 rl + u
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int q = tid + 256 * m, rec = q >> 2, part = q & 3;
    const int row = (rec & (XTA_RL - 1)) * XTA_RPT + (rec >> 4);
    soff[m] = row * XTA_KT + part * 4; doff[m] = rec * XTA_AS + part * 4;
  }
  for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
    const int64_t j0 = blk * XTA_WGC + cg * XTA_CW;
    double acc[XTA_CW][XTA_KT];
#pragma unroll
    for (int c = 0; c < XTA_CW; ++c)
#pragma unroll
      for (int t = 0; t < XTA_KT; ++t) acc[c][t] = 0.0;
    for (int64_t i0 = 0; i0 < a.ld; i0 += XTA_RT) {
      __syncthreads();   // the previous tile is consumed
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        const xta_d2 *s = reinterpret_cast<const xta_d2 *>(Ag + (size_t)i0 * XTA_KT + soff[m]);
        xta_d2 *d = reinterpret_cast<xta_d2 *>(at + doff[m]);
        d[0] = s[0]; d[1] = s[1];
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < XTA_RPT; ++u) {
        const xta_d2 *ar = reinterpret_cast<const xta_d2 *>(at + (u * XTA_RL + rl) * XTA_AS);
        double av[XTA_KT];
#pragma unroll
        for (int t = 0; t < XTA_KT / 2; ++t) { const xta_d2 v = ar[t]; av[2 * t] = v.x; av[2 * t + 1] = v.y; }
        const int64_t i = i0 + rl * XTA_RPT + u;
#pragma unroll
        for (int c = 0; c < XTA_CW; ++c) {
          const double x = (i < a.n && j0 + c < a.p) ? a.Z[(size_t)(j0 + c) * (size_t)a.ldz + (size_t)i] : 0.0;
#pragma unroll
          for (int t = 0; t < XTA_KT; ++t) acc[c][t] = fma(x, av[t], acc[c][t]);
        }
      }
    }
    // the sixteen row lanes of a column group: k_xta's halving exchange over lane distances 8, 4, 2, 1
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
    const int64_t j = j0 + (rl >> 2);
    if (j < a.p) {
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int64_t tt = g * XTA_KT + (rl & 3) * 4 + m;
        if (tt < a.f) a.out[(size_t)tt * (size_t)a.ldo + (size_t)j] = v[m];
      }
    }
  }
}

// ---- Zp = Z - X C ----
struct ProjArgs {
  const int8_t *Xp; int R;                  // Z as a panel: slab w holds its p columns of R rows each (R a multiple of 128) ...
  const double *Zd; int64_t ldz;            // ... or dense, column stride ldz (Xp == nullptr)
  int64_t n, p, rows;                       // rows: a multiple of PROJ_T, at least n; the rows n .. rows-1 are written as zeros where pad is set
  const double *X; int64_t ldx;             // n x f on the device
  const double *C;                          // f x p on the device, C[j * f + l]
  int f, fp, pad;                           // fp: covariates per piece, min(f, PROJ_FP)
  double *out; int64_t ldo;
};
__global__ __launch_bounds__(256, 2) void k_project(const ProjArgs a) {
  extern __shared__ __attribute__((aligned(16))) double proj_smem[];
  double *xs = proj_smem, *cs = proj_smem + (size_t)a.fp * PROJ_T;   // [l][row], [l][column]
  const int tid = threadIdx.x, ri = tid & 15, ci = tid >> 4;
  const int64_t jb = (int64_t)blockIdx.x * PROJ_T, j0 = jb + 4 * ci;
  const int npieces = (a.f + a.fp - 1) / a.fp;
  const int64_t ntiles = a.rows / PROJ_T;
  const bool vec = ((a.ldo & 1) == 0) && ((reinterpret_cast<uintptr_t>(a.out) & 15) == 0);
  bool c_staged = false;
  for (int64_t tile = blockIdx.y; tile < ntiles; tile += gridDim.y) {
    const int64_t i0 = tile * PROJ_T + 4 * ri;
    double acc[4][4];   // [column][row]
    if (a.Xp) {
      const int64_t w = (tile * PROJ_T) / a.R;
      const int off = (int)(tile * PROJ_T - w * a.R) + 4 * ri;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        uint32_t word = 0u;
        if (j0 + c < a.p) word = *reinterpret_cast<const uint32_t *>(a.Xp + (size_t)((w * a.p + j0 + c) * a.R + off));
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c][r] = (double)(int)(int8_t)(word >> (8 * r));
      }
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[c][r] = (j0 + c < a.p && i0 + r < a.n) ? a.Zd[(size_t)(j0 + c) * (size_t)a.ldz + (size_t)(i0 + r)] : 0.0;
    }
    for (int pc = 0; pc < npieces; ++pc) {
      const int l0 = pc * a.fp, fl = a.f - l0 < a.fp ? a.f - l0 : a.fp;
      __syncthreads();   // the previous piece is consumed
      for (int e = tid; e < fl * PROJ_T; e += 256) {
        const int l = e >> 6, r = e & 63;
        const int64_t i = tile * PROJ_T + r;
        xs[l * PROJ_T + r] = i < a.n ? a.X[(size_t)(l0 + l) * (size_t)a.ldx + (size_t)i] : 0.0;
      }
      if (!c_staged || npieces > 1) {
        for (int e = tid; e < fl * PROJ_T; e += 256) {
          const int c = e / fl, l = e - c * fl;   // a column's piece of C is contiguous
          cs[l * PROJ_T + c] = jb + c < a.p ? a.C[(size_t)(jb + c) * (size_t)a.f + (size_t)(l0 + l)] : 0.0;
        }
        c_staged = true;
      }
      __syncthreads();
      for (int l = 0; l < fl; ++l) {
        const xta_d2 x0 = *reinterpret_cast<const xta_d2 *>(xs + l * PROJ_T + 4 * ri), x1 = *reinterpret_cast<const xta_d2 *>(xs + l * PROJ_T + 4 * ri + 2);
        const xta_d2 c0 = *reinterpret_cast<const xta_d2 *>(cs + l * PROJ_T + 4 * ci), c1 = *reinterpret_cast<const xta_d2 *>(cs + l * PROJ_T + 4 * ci + 2);
        const double xv[4] = {-x0.x, -x0.y, -x1.x, -x1.y}, cv[4] = {c0.x, c0.y, c1.x, c1.y};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[c][r] = fma(xv[r], cv[c], acc[c][r]);
      }
    }
    const int64_t top = a.pad ? a.rows : a.n;   // the rows this call writes
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (j0 + c >= a.p) continue;
      double *o = a.out + (size_t)(j0 + c) * (size_t)a.ldo + (size_t)i0;
      double v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = i0 + r < a.n ? acc[c][r] : 0.0;
      if (vec && i0 + 4 <= top) {
        reinterpret_cast<xta_d2 *>(o)[0] = xta_d2{v[0], v[1]};
        reinterpret_cast<xta_d2 *>(o)[1] = xta_d2{v[2], v[3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) if (i0 + r < top) o[r] = v[r];
      }
    }
  }
}

}  // namespace bwgr
