// bwgr_amd: the per-trait ridge engine -- solver1x / UVBETA (src/RcppEigen20230423.cpp:1410-1443, :1506-1515), solver1xF / FUVBETA
// (:1613-1646, :1709-1718), xsolver1xF / XFUVBETA (:1721-1753), zsolver1xF / ZFUVBETA (:1771-1816).
//
// One randomized Gauss-Seidel ridge fit per column of Y, all on one X.  The marker order of sweep s depends on s alone (:1428), so every trait
// walks the same gathered panel; the traits never couple.  They are taken in groups of UVB_W = 64; per sweep and group the launch train is
// mrr's (mrr.hip.h): k_mrr_gram, then per 64-marker block k_uvb_pass and k_uvb_solve, then the tails.  What differs from mrr:
//
//   k_uvb_setup   once per call and group: S_t(j) = sum_obs x_rj, Q_t(j) = sum_obs x_rj^2, tilde_t(j) = sum_r x_rj y_rt (raw x, :1415) ->
//                 XX_jt = (n_t Q - S^2) / n_t, the numerator in int64: a marker monomorphic among the trait's rows gets exactly 0
//   k_uvb_pass    per block: e_rt -= z_rt (sum_j x_rj dB_jt - c_t) for block b - 1, partial dots X_b' E for block b; 64 traits per tile
//   k_uvb_solve   per block: UVB_ST = 16 traits per workgroup, one lane per trait; the lane runs the block's 64-step recurrence of its own
//                 trait against its own pattern's Gram matrix.  No k x k system, no product across traits, no cross-lane traffic
//   k_uvb_rows, k_uvb_cols   the tails' fixed-order partial sums: sum e, e'y, e'e; b'b, tilde'b (or sum XX)
//
// Centring is per trait and implicit: with x_c,j = x_j - S_t(j) / n_t on the trait's rows and E zero on unobserved rows,
//   x_c,j'e_t = x_j'e_t - (S_t(j) / n_t) sum(e_t)       and       Gc_t(l, j) = G_g(l, j) - S_t(l) S_t(j) / n_t,  g = the trait's pattern.
// The solve keeps u_l = x_l'e - sum_{i<j} G_g(l, i) dB_i in LDS and the scalar c = sum_{i<j} S_t(i) dB_i / n_t in a register, so that the
// centred dot of marker l is u_l + S_t(l) (c - sum(e) / n_t); c at the block's end is the pass's c_t = sum_j xbar_jt dB_jt.
//
// Per-(marker, trait) arrays of a group are [p][UVB_W] (a marker's 64 traits side by side: the lanes of a solve read them coalesced);
// E and y are [trait][ld].  A frozen trait (stopped earlier) or a padding lane of the last group has active = 0: its dB is never read,
// nothing of it is written, and the tails skip it.
#pragma once
#include "mrr.hip.h"
#include "uvb_tail.h"

namespace bwgr {

static constexpr int UVB_W = 64;          // traits per group (row masks are one uint64 per row)
static constexpr int UVB_ST = 16;         // traits per solve workgroup
static constexpr int UVB_PASS_WG = 64;    // workgroups of k_uvb_pass at most (= partial dot sets a solve reduces)
static constexpr int UVB_NP = 32;         // partials of the tail reductions
static constexpr int UVB_GSTR = MRR_MB * MRR_MB + 4;   // words between two staged Gram matrices: 16-byte aligned, four banks apart
// (UvbTrait, what the kernels read of a trait: uvb_tail.h)

// where trait t of a group sits in the pass's LDS tiles: thread slice tq = t & 3 holds its 16 traits t = tq + 4 i side by side
__device__ __forceinline__ int uvb_perm(int t) { return (t & 3) * 16 + (t >> 2); }

// ---- once per call and group: S, XX, tilde of every marker, natural order; workgroup = one 64-marker block, all rows ----
// Sums of integers (|.| < 2^53) in doubles are exact in any order.
__global__ __launch_bounds__(256) void k_uvb_setup(const int8_t *__restrict__ X, int R, int64_t p, int64_t ld, const unsigned long long *__restrict__ zb,
                                                   const double *__restrict__ y, const UvbTrait *__restrict__ tr, int kg,
                                                   double *__restrict__ S, double *__restrict__ XX, double *__restrict__ tilde) {
  __shared__ __attribute__((aligned(16))) int8_t xt[MRR_MB * 68];
  __shared__ __attribute__((aligned(16))) double yt[64 * UVB_W];
  __shared__ __attribute__((aligned(16))) float zt[64 * UVB_W];
  const int tid = threadIdx.x, rr = tid & 63, tq = tid >> 6, jm = tid & 63;
  const int blk = blockIdx.x;
  double xy[16], ss[16], qq[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) { xy[i] = 0.0; ss[i] = 0.0; qq[i] = 0.0; }
  for (int64_t r0 = 0; r0 < ld; r0 += 64) {
    __syncthreads();
    {
      const int lm = tid >> 2, q = tid & 3;
      const int64_t j = (int64_t)blk * MRR_MB + lm;
      mrr_v4i v = {0, 0, 0, 0};
      if (j < p) v = *reinterpret_cast<const mrr_v4i *>(X + mrr_xoff(r0 + 16 * q, j, R, p));
      int *dst = reinterpret_cast<int *>(xt + lm * 68 + 16 * q);
      dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
    }
    const unsigned long long z = zb[r0 + rr];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int t = tq + 4 * i;
      yt[rr * UVB_W + tq * 16 + i] = t < kg ? y[(size_t)t * ld + r0 + rr] : 0.0;
      zt[rr * UVB_W + tq * 16 + i] = (float)((z >> t) & 1ull);
    }
    __syncthreads();
    const int *xw = reinterpret_cast<const int *>(xt + jm * 68);
    for (int w4 = 0; w4 < 16; ++w4) {
      const int word = xw[w4];
#pragma unroll
      for (int by = 0; by < 4; ++by) {
        const double x = (double)(int)(int8_t)(word >> (8 * by)), x2 = x * x;
        const int row = 4 * w4 + by;
        const double *yp = yt + row * UVB_W + tq * 16;
        const float *zp = zt + row * UVB_W + tq * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const double zv = (double)zp[i];
          xy[i] = fma(x, yp[i], xy[i]); ss[i] = fma(x, zv, ss[i]); qq[i] = fma(x2, zv, qq[i]);
        }
      }
    }
  }
  const int64_t j = (int64_t)blk * MRR_MB + jm;
  if (j >= p) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int t = tq + 4 * i;
    if (t >= kg) continue;
    const long long nt = (long long)tr[t].nt, s = (long long)ss[i], q = (long long)qq[i];
    const size_t o = (size_t)j * UVB_W + t;
    S[o] = ss[i];
    XX[o] = nt > 0 ? (double)(nt * q - s * s) / (double)nt : 0.0;
    tilde[o] = xy[i];
  }
}

// ---- per block: the residual update of block `prev` and the partial dots of block `next` in one pass over the rows ----
// k_mrr_pass for 64 traits: thread (row or marker = tid & 63, slice tq = tid >> 6) carries the 16 traits t = tq + 4 i.  The tiles in LDS are
// [.][uvb_perm(t)], so a thread's 16 values are 128 contiguous bytes that its whole wave reads as a broadcast.
struct UvbPassArgs {
  const int8_t *Xs; int R; int64_t p, ld;
  const unsigned long long *zb; double *e;
  const double *dB;       // [64][UVB_W] + c[UVB_W]
  double *part;           // [G][65][UVB_W]
  int prev, next;
  unsigned long long act; // traits of the group that run this sweep
};
static constexpr size_t UVB_PASS_LDS = sizeof(double) * (2 * 64 * UVB_W + UVB_W) + MRR_MB * 68;
__global__ __launch_bounds__(256) void k_uvb_pass(const UvbPassArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double *et = reinterpret_cast<double *>(smem);     // [row][perm t]
  double *dBl = et + 64 * UVB_W;                     // [marker][perm t]
  double *cl = dBl + 64 * UVB_W;                     // [perm t]
  int8_t *xt = reinterpret_cast<int8_t *>(cl + UVB_W);   // [marker][row], 68-byte rows
  const int tid = threadIdx.x, rr = tid & 63, tq = tid >> 6;
  const int64_t ntiles = A.ld / 64;
  unsigned mine = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) mine |= (unsigned)((A.act >> (tq + 4 * i)) & 1ull) << i;
  if (A.prev >= 0)
    for (int i = tid; i < 64 * UVB_W + UVB_W; i += 256) {
      const int jm = i >> 6, t = i & 63;
      dBl[jm * UVB_W + uvb_perm(t)] = A.dB[i];   // (row 64 of dB is c: it lands in cl)
    }
  double dacc[16], eacc = 0.0;
#pragma unroll
  for (int i = 0; i < 16; ++i) dacc[i] = 0.0;
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
      const unsigned long long z = A.zb[r];
      double s[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) s[i] = 0.0;
      for (int jm = 0; jm < MRR_MB; ++jm) {
        const double x = (double)xt[jm * 68 + rr];
        const double *d = dBl + jm * UVB_W + tq * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) if ((mine >> i) & 1u) s[i] = fma(x, d[i], s[i]);
      }
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        if (!((mine >> i) & 1u)) continue;
        const int t = tq + 4 * i;
        double ev = A.e[(size_t)t * A.ld + r];
        if ((z >> t) & 1ull) { ev -= s[i] - cl[tq * 16 + i]; A.e[(size_t)t * A.ld + r] = ev; }
        et[rr * UVB_W + tq * 16 + i] = ev;
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if ((mine >> i) & 1u) et[rr * UVB_W + tq * 16 + i] = A.e[(size_t)(tq + 4 * i) * A.ld + r];
    }
    if (A.next < 0) continue;
    load_tile(A.next, r0);
    __syncthreads();
    const int *xw = reinterpret_cast<const int *>(xt + rr * 68);   // (rr: this thread's marker in the dots)
    for (int w4 = 0; w4 < 16; ++w4) {
      const int word = xw[w4];
#pragma unroll
      for (int by = 0; by < 4; ++by) {
        const double x = (double)(int)(int8_t)(word >> (8 * by));
        const double *ep = et + (4 * w4 + by) * UVB_W + tq * 16;
#pragma unroll
        for (int i = 0; i < 16; ++i) if ((mine >> i) & 1u) dacc[i] = fma(x, ep[i], dacc[i]);
      }
    }
    if (tid < UVB_W && ((A.act >> tid) & 1ull)) {
      const int o = uvb_perm(tid);
      for (int row = 0; row < 64; ++row) eacc += et[row * UVB_W + o];
    }
  }
  if (A.next < 0) return;
  double *pw = A.part + (size_t)blockIdx.x * (MRR_MB + 1) * UVB_W;
#pragma unroll
  for (int i = 0; i < 16; ++i) if ((mine >> i) & 1u) pw[rr * UVB_W + tq + 4 * i] = dacc[i];
  if (tid < UVB_W && ((A.act >> tid) & 1ull)) pw[MRR_MB * UVB_W + tid] = eacc;
}

// ---- per block: the serial recurrence of the block's markers (:1429-1432), one lane per trait ----
// Phase 1 (256 threads): the Gram matrices of the workgroup's first `ngl` patterns into LDS (slotpat names them; a slot no running trait uses is skipped), u[j][t] = sum_w part[w][j][t].
// Phase 2 (lanes 0 .. 15 of wave 0, lane = trait 16 blockIdx.x + lane, no barriers), marker j in order:
//   q = u_j + S_j (c - sum(e) / n_t);   b1 = (q + XX_j b0) / (XX_j + lambda) where XX_j > thr, else b_j = 0;   d = b1 - b0
//   u_l -= G_g(l, j) d for l > j (row j of the symmetric matrix; the next row is requested a step ahead);   c += S_j d / n_t
// thr = 1e-5 is solver1xF's test (:1633-1635).  The other solvers run with thr = 0: their centred column is exactly zero where XX is, so
// their b1 is exactly 0 there, which the rounding of u_j + S_j c would not give.
struct UvbSolveArgs {
  const double *part; int G;
  const int32_t *order; int blk; int64_t p;
  const int32_t *gram; int npat;
  const double *S, *XX;
  double *b, *dB, *db2;
  const UvbTrait *tr;
  const int *slotpat;     // [solve workgroup][ngl]: the pattern staged in each LDS slot, or -1
  int ngl;
  double thr;
};
__host__ __device__ inline size_t uvb_solve_lds(int ngl) {
  return (size_t)ngl * UVB_GSTR * 4 + sizeof(double) * (MRR_MB * UVB_ST + UVB_ST) + 4 * MRR_MB;
}
__global__ __launch_bounds__(256) void k_uvb_solve(const UvbSolveArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t *gl = reinterpret_cast<int32_t *>(smem);
  double *u = reinterpret_cast<double *>(smem + (size_t)A.ngl * UVB_GSTR * 4);   // [64][UVB_ST]
  double *sel = u + MRR_MB * UVB_ST;
  int *Jl = reinterpret_cast<int *>(sel + UVB_ST);
  const int tid = threadIdx.x, t0 = blockIdx.x * UVB_ST;
  const int64_t j0 = (int64_t)A.blk * MRR_MB;
  const int mB = (int)(A.p - j0 < MRR_MB ? A.p - j0 : MRR_MB);
  const int32_t *gblk = A.gram + (size_t)A.blk * A.npat * (MRR_MB * MRR_MB);
  if (tid < MRR_MB) Jl[tid] = tid < mB ? A.order[j0 + tid] : 0;
  for (int s = 0; s < A.ngl; ++s) {
    const int g = A.slotpat[blockIdx.x * A.ngl + s];
    if (g < 0) continue;
    bool used = false;   // by a trait of this workgroup that still runs
    for (int tl = 0; tl < UVB_ST; ++tl) used = used || (A.tr[t0 + tl].active && A.tr[t0 + tl].slot == s);
    if (!used) continue;
    const int4 *src = reinterpret_cast<const int4 *>(gblk + (size_t)g * (MRR_MB * MRR_MB));
    int4 *dst = reinterpret_cast<int4 *>(gl + (size_t)s * UVB_GSTR);
    for (int i = tid; i < MRR_MB * MRR_MB / 4; i += 256) dst[i] = src[i];
  }
  for (int o = tid; o < (MRR_MB + 1) * UVB_ST; o += 256) {
    const int jm = o / UVB_ST, tl = o - jm * UVB_ST;
    if (!A.tr[t0 + tl].active) continue;
    double s = 0.0;
    for (int w = 0; w < A.G; ++w) s += A.part[((size_t)w * (MRR_MB + 1) + jm) * UVB_W + t0 + tl];
    u[o] = s;   // (row 64 is sel: sum e)
  }
  __syncthreads();
  if (tid >= UVB_ST) return;
  const int t = t0 + tid;
  const UvbTrait T = A.tr[t];
  if (!T.active) return;
  const double inv_nt = 1.0 / T.nt, c0 = -sel[tid] * inv_nt;
  const int32_t *grow = gblk + (size_t)T.pat * (MRR_MB * MRR_MB);
  const int32_t *lrow = gl + (size_t)(T.slot >= 0 ? T.slot : 0) * UVB_GSTR;
  const bool in_lds = T.slot >= 0;
  int4 gc[16], gn[16];
  auto load_row = [&](int j, int4 *dst) {   // the quads of row j that hold an l > j
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (4 * i + 3 > j) dst[i] = in_lds ? *reinterpret_cast<const int4 *>(lrow + j * MRR_MB + 4 * i) : *reinterpret_cast<const int4 *>(grow + j * MRR_MB + 4 * i);
  };
#pragma unroll
  for (int i = 0; i < 16; ++i) { gc[i] = make_int4(0, 0, 0, 0); gn[i] = make_int4(0, 0, 0, 0); }
  double c = 0.0, acc2 = 0.0;
  size_t o = (size_t)Jl[0] * UVB_W + t;
  double xx_n = A.XX[o], s_n = A.S[o], b_n = A.b[o];
  load_row(0, gc);
  for (int j = 0; j < mB; ++j) {
    const double xx = xx_n, sj = s_n, b0 = b_n;
    const size_t oj = o;
    if (j + 1 < mB) {
      o = (size_t)Jl[j + 1] * UVB_W + t;
      xx_n = A.XX[o]; s_n = A.S[o]; b_n = A.b[o];
      load_row(j + 1, gn);
    }
    double b1 = 0.0, d = 0.0;
    if (xx > A.thr) {
      const double q = u[j * UVB_ST + tid] + sj * (c0 + c);
      b1 = (q + xx * b0) / (xx + T.lam);
      d = b1 - b0;
    }
    A.b[oj] = b1;
    A.dB[j * UVB_W + t] = d;
    acc2 = fma(d, d, acc2);
    c = fma(sj * inv_nt, d, c);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (4 * i + 3 <= j) continue;
      const int gq[4] = {gc[i].x, gc[i].y, gc[i].z, gc[i].w};
#pragma unroll
      for (int cc = 0; cc < 4; ++cc) {
        const int l = 4 * i + cc;
        if (l > j) u[l * UVB_ST + tid] = fma(-(double)gq[cc], d, u[l * UVB_ST + tid]);
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) gc[i] = gn[i];
  }
  for (int j = mB; j < MRR_MB; ++j) A.dB[j * UVB_W + t] = 0.0;   // a short last block: the pass multiplies these by columns of zeros
  A.dB[MRR_MB * UVB_W + t] = c;
  A.db2[t] += acc2;
}

// ---- tails, deterministic (fixed partial order); a frozen or padding trait is skipped ----
// part[(bx * 3 + q) * UVB_W + t]: q = 0 sum_r e_rt, 1 sum_r e_rt y_rt, 2 sum_r e_rt^2     grid (UVB_NP, UVB_W)
__global__ __launch_bounds__(256) void k_uvb_rows(const double *__restrict__ e, const double *__restrict__ y, int64_t ld, unsigned long long act,
                                                  double *__restrict__ part) {
  __shared__ double red[12];
  const int t = blockIdx.y;
  if (!((act >> t) & 1ull)) return;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < ld; r += (int64_t)gridDim.x * 256) {
    const double ev = e[(size_t)t * ld + r];
    s0 += ev; s1 = fma(ev, y[(size_t)t * ld + r], s1); s2 = fma(ev, ev, s2);
  }
  s0 = mrr_wave_sum(s0); s1 = mrr_wave_sum(s1); s2 = mrr_wave_sum(s2);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { red[w] = s0; red[4 + w] = s1; red[8 + w] = s2; }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    part[((size_t)blockIdx.x * 3 + q) * UVB_W + t] = red[4 * q] + red[4 * q + 1] + red[4 * q + 2] + red[4 * q + 3];
  }
}
// part[(bx * 2 + q) * UVB_W + t]: mode 0: q = 0 sum_j b_jt^2, 1 sum_j tilde_jt b_jt; mode 1: q = 0 sum_j XX_jt (TrXSX)     grid (UVB_NP)
__global__ __launch_bounds__(256) void k_uvb_cols(const double *__restrict__ b, const double *__restrict__ tilde, const double *__restrict__ XX,
                                                  int64_t p, int mode, unsigned long long act, double *__restrict__ part) {
  __shared__ double red[2 * 4 * UVB_W];
  const int t = threadIdx.x & 63, jq = threadIdx.x >> 6;
  double a0 = 0.0, a1 = 0.0;
  if ((act >> t) & 1ull)
    for (int64_t j = (int64_t)blockIdx.x * 4 + jq; j < p; j += (int64_t)gridDim.x * 4) {
      const size_t o = (size_t)j * UVB_W + t;
      if (mode == 1) { a0 += XX[o]; continue; }
      const double bv = b[o];
      a0 = fma(bv, bv, a0); a1 = fma(tilde[o], bv, a1);
    }
  red[jq * UVB_W + t] = a0; red[(4 + jq) * UVB_W + t] = a1;
  __syncthreads();
  if (threadIdx.x < 2 * UVB_W) {
    const int q = threadIdx.x >> 6;
    part[((size_t)blockIdx.x * 2 + q) * UVB_W + t] = red[(4 * q) * UVB_W + t] + red[(4 * q + 1) * UVB_W + t] + red[(4 * q + 2) * UVB_W + t] + red[(4 * q + 3) * UVB_W + t];
  }
}
// e_t -= mu0_t on the trait's rows (:1433) for the traits that ran this sweep     grid (row blocks, UVB_W)
__global__ void k_uvb_mu_shift(double *__restrict__ e, const unsigned long long *__restrict__ zb, int64_t ld, int n, unsigned long long ran,
                               const double *__restrict__ mu0) {
  const int t = blockIdx.y;
  if (!((ran >> t) & 1ull)) return;
  const double m = mu0[t];
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    if ((zb[r] >> t) & 1ull) e[(size_t)t * ld + r] -= m;
}
// xb[t][r] = sum_j x_rj b_jt over the natural panel, every row, markers in order     grid (row blocks, 16-trait slices)
__global__ __launch_bounds__(256) void k_uvb_xb(const int8_t *__restrict__ X, int R, int64_t p, int n, const double *__restrict__ b, int kg,
                                                double *__restrict__ xb) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int t0 = blockIdx.y * 16;
  if (r >= n) return;
  double acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.0;
  for (int64_t j = 0; j < p; ++j) {
    const double x = (double)X[mrr_xoff(r, j, R, p)];
    const double *bp = b + (size_t)j * UVB_W + t0;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = fma(x, bp[i], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) if (t0 + i < kg) xb[(size_t)(t0 + i) * n + r] = acc[i];
}
// the group's [p][UVB_W] effects as columns of the p x k output
__global__ void k_uvb_b_out(const double *__restrict__ b, int64_t p, int kg, double *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p * kg; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t t = i / p, j = i - t * p;
    out[i] = b[(size_t)j * UVB_W + t];
  }
}

}  // namespace bwgr
