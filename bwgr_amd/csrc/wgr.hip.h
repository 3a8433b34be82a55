// bwgr_amd/csrc/wgr.hip.h -- wgr's kernels: the R-side (double) steps around the KMUP sweep, the polygenic term, bagging's residual gather
// and the posterior means.  Part of bwgr_hip.hip, which includes it after sweep.hip.h, rng.hip.h (ChainScalars, Rng and the variates) and
// panel.hip.h (wave_sum, block_sum, xval); it defines no host function.
namespace {
// ---- wgr(): R-side (double) steps around the KMUP sweep, R/wgr.R:41-168 --------------------------------------------
struct WgrScalars {
  double mu, Ve, Va, Sb, Se, MSx, vy, bb, B0, VE, VA, sumD, cxx;
  double Vp, VP, Sk;   // polygenic term (eigK)
};
// per-column double statistics as R computes them: xx = crossprod, var = sum((x-mean)^2)/(n-1); one wave per column
template <typename XT>
__global__ void k_stats64(const XT *X, int R, int n, int p, double *xx, double *vx) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (j >= p) return;
  double s1 = 0, s2 = 0;
  for (int i = lane; i < n; i += 64) { const double v = (double)xval(X, xoff(i, j, R, p)); s1 += v; s2 = fma(v, v, s2); }
  s1 = wave_sum(s1); s2 = wave_sum(s2);
  s1 = __shfl(s1, 0, 64); s2 = __shfl(s2, 0, 64);
  const double mean = s1 / (double)n;
  double sv = 0;
  for (int i = lane; i < n; i += 64) { const double dev = (double)xval(X, xoff(i, j, R, p)) - mean; sv = fma(dev, dev, sv); }
  sv = wave_sum(sv);
  if (lane == 0) { xx[j] = s2; vx[j] = sv / (double)(n - 1); }
}
__global__ void k_dsum_stage1(const double *v, int64_t n, double *part, int square) {
  __shared__ double red[17];
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) s += square ? v[i] * v[i] : v[i];
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// setup: mu = mean(y), e = y - mu, vy = var(y), MSx, priors (R/wgr.R:49-59); part = 256 partial sums of column variances,
// part2 = 256 partial sums of xx
__global__ void k_wgr_init(const double *y, double *eR, int n, int64_t ld, const double *part, const double *part2, int p,
                           double df, double R2, WgrScalars *ws) {
  __shared__ double red[17];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += y[i];
  s = block_sum(s, red);
  const double mu = s / (double)n;
  double sv = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { const double dev = y[i] - mu; sv += dev * dev; }
  sv = block_sum(sv, red);
  double ms = 0, sx = 0;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) { ms += part[i]; sx += part2[i]; }
  ms = block_sum(ms, red);
  sx = block_sum(sx, red);
  for (int64_t i = threadIdx.x; i < ld; i += blockDim.x) eR[i] = (i < n) ? (y[i] - mu) : 0.0;
  if (threadIdx.x == 0) {
    WgrScalars w; memset(&w, 0, sizeof(w));
    w.mu = mu; w.vy = sv / (double)(n - 1); w.MSx = ms; w.Ve = 1.0; w.Va = ms;
    w.Sb = (R2) * df * w.vy / ms; w.Se = (1 - R2) * df * w.vy; w.cxx = sx / (double)p;
    w.Sk = R2 * w.vy * (df + 2); w.Vp = 1.0;                                       // R/wgr.R:60, :30
    *ws = w;
  }
}
__global__ void k_wgr_marker_init(double *bR, double *dR, double *VbR, double *LR, double *B, double *D, double *VB, int p, const WgrScalars *ws) {
  const double Va = ws->Va, Ve = ws->Ve;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    bR[j] = 0; dR[j] = 1; VbR[j] = Va; LR[j] = Va / Ve; B[j] = 0; D[j] = 0; VB[j] = 0;   // L = Vb/Ve (sic), R/wgr.R:55
  }
}
// narrowing at the .Call boundary (src/RcppExports.cpp:20-27): double R vectors -> float KMUP arguments
__global__ void k_wgr_pre(const double *bR, const double *dR, const double *LR, const double *xx64, const double *eR, float *bf, float *df_,
                          float *Lf, float *xxf, double *e64, int p, int n, int64_t ld, float pi, const WgrScalars *ws, ChainScalars *sc) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = gid; j < p; j += gsz) { bf[j] = (float)bR[j]; df_[j] = (float)dR[j]; Lf[j] = (float)LR[j]; xxf[j] = (float)xx64[j]; }
  for (int64_t i = gid; i < ld; i += gsz) e64[i] = (i < n) ? (double)(float)eR[i] : 0.0;
  if (gid == 0) {
    ChainScalars c; memset(&c, 0, sizeof(c));
    const float Ve = (float)ws->Ve;
    c.ve = Ve; c.pi = pi; c.C = -0.5f / sqrtf(Ve); c.odds = pi / (1.0f - pi); c.dfp1 = 1.0f;
    c.inc_rate = 1.0f - pi;
    c.nredo = sc->nredo;   // (the call's count so far: zeroed before the first iteration)
    *sc = c;
  }
}
// widening of KMUP's outputs + marker-variance step (R/wgr.R:86-111)
__global__ void k_wgr_post(const float *bf, const float *df_, double *bR, double *dR, double *VbR, int p, int use_d, int iv, int de,
                           double dfv, uint32_t iter, Rng rng, const WgrScalars *ws) {
  const double Sb = ws->Sb, Ve = ws->Ve, MSx = ws->MSx;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    const double b = (double)bf[j];
    bR[j] = b;
    if (use_d) dR[j] = (double)df_[j];
    if (iv) VbR[j] = de ? sqrt(b * b * Ve / MSx) : (Sb + b * b) / rng_chisq(rng, dfv + 1.0, (uint32_t)j, iter, RNG_CHI);
  }
}
// Va (common variance) and Ve draws (R/wgr.R:113,121); e64 holds KMUP's residual (float values)
__global__ __launch_bounds__(1024) void k_wgr_scal(const double *e64, int n, double n_dof, int p, const double *bbpart, int iv, double dfv, uint32_t iter, Rng rng, WgrScalars *ws) {
  __shared__ double red[17];
  double ee = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) { const double v = (double)(float)e64[i]; ee += v * v; }
  ee = block_sum(ee, red);
  double bb = 0;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) bb += bbpart[i];
  bb = block_sum(bb, red);
  if (threadIdx.x == 0) {
    if (!iv) ws->Va = (bb + ws->Sb) / rng_chisq(rng, dfv + (double)p, RNG_GLOBAL_MARKER, iter, RNG_G_VB);
    ws->Ve = (ee + ws->Se) / rng_chisq(rng, n_dof + dfv, RNG_GLOBAL_MARKER, iter, RNG_G_VE);   // n*bag + df, R/wgr.R:121
    ws->bb = bb;
  }
}
// L = Ve/Vb (R/wgr.R:122) and posterior sums of the marker vectors (R/wgr.R:130-134)
__global__ void k_wgr_L(const double *bR, const double *dR, double *VbR, double *LR, double *B, double *D, double *VB, int p, int iv, int accumulate, const WgrScalars *ws) {
  const double Ve = ws->Ve, Va = ws->Va;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    if (!iv) VbR[j] = Va;
    LR[j] = Ve / VbR[j];
    if (accumulate) { B[j] += bR[j]; D[j] += dR[j]; if (iv) VB[j] += VbR[j]; }
  }
}
// e = y - mu - X b from the fp64 partial products (R/wgr.R:124)
__global__ void k_wgr_efinish(const double *part, int64_t ld, int nchunks, int n, const double *y, double *eR, const WgrScalars *ws) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * ld + i];
  eR[i] = y[i] - ws->mu - s;
}
// intercept (R/wgr.R:125-127) and scalar posterior sums
__global__ __launch_bounds__(1024) void k_wgr_mu(double *eR, int n, int iv, int accumulate, uint32_t iter, Rng rng, WgrScalars *ws) {
  __shared__ double red[17];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += eR[i];
  s = block_sum(s, red);
  const double mu0 = s / (double)n + (ws->Ve / (double)n) * rng_normal(rng, RNG_GLOBAL_MARKER, iter, RNG_G_MU, 0);   // sd = Ve/n (sic)
  for (int i = threadIdx.x; i < n; i += blockDim.x) eR[i] -= mu0;
  __syncthreads();
  if (threadIdx.x == 0) {
    ws->mu += mu0;
    if (accumulate) { ws->B0 += ws->mu; ws->VE += ws->Ve; if (!iv) ws->VA += ws->Va; }
  }
}
// ---- polygenic term: narrowing for KMUP(U,h,dh,xxK,e,Lk,Ve,0) (R/wgr.R:70-76), widening of its outputs ----
__global__ void k_wgr_pre_k(const double *hR, const double *Vd, const double *eR, float *hf, float *dhf, float *xxKf, float *Lkf, double *e64,
                            int pk, int n, int64_t ld, const WgrScalars *ws, ChainScalars *sc) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
  const double Ve = ws->Ve, Vp = ws->Vp;
  for (int64_t k = gid; k < pk; k += gsz) { hf[k] = (float)hR[k]; dhf[k] = 0.0f; xxKf[k] = 1.0f; Lkf[k] = (float)(Ve / (Vd[k] * Vp)); }
  for (int64_t i = gid; i < ld; i += gsz) e64[i] = (i < n) ? (double)(float)eR[i] : 0.0;
  if (gid == 0) {
    ChainScalars c; memset(&c, 0, sizeof(c));
    const float Vef = (float)Ve;
    c.ve = Vef; c.pi = 0.0f; c.C = -0.5f / sqrtf(Vef); c.odds = 0.0f; c.dfp1 = 1.0f;
    *sc = c;
  }
}
__global__ void k_wgr_post_k(const float *hf, double *hR, const double *e64, double *eR, int pk, int n) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, gsz = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = gid; k < pk; k += gsz) hR[k] = (double)hf[k];
  for (int64_t i = gid; i < n; i += gsz) eR[i] = (double)(float)e64[i];   // KMUP returns e as float (src/Rcpp20260726ai.cpp:37)
}
// Vp = (sum(h^2/V) + Sk)/rchisq(1, df+pk)  (R/wgr.R:117)
__global__ __launch_bounds__(1024) void k_wgr_vp(const double *hR, const double *Vd, int pk, double dfv, uint32_t iter, Rng rng, WgrScalars *ws) {
  __shared__ double red[17];
  double s = 0;
  for (int k = threadIdx.x; k < pk; k += blockDim.x) s += hR[k] * hR[k] / Vd[k];
  s = block_sum(s, red);
  if (threadIdx.x == 0) ws->Vp = (s + ws->Sk) / rng_chisq(rng, dfv + (double)pk, RNG_GLOBAL_MARKER, iter, RNG_G_VK);
}
// out[i] (+)= sum_k U[i,k] * coef[k] * scale   (U %*% h in double, R/wgr.R:124,148)
__global__ void k_uh(const double *Ud, const double *coef, int n, int pk, double scale, double *out, int accumulate_into_neg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int k = 0; k < pk; ++k) s = fma(Ud[(size_t)k * n + i], coef[k] * scale, s);
  if (accumulate_into_neg) out[i] -= s; else out[i] = s;
}
__global__ void k_wgr_accum_k(const double *hR, double *H, int pk, WgrScalars *ws) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < pk; k += gridDim.x * blockDim.x) H[k] += hR[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) ws->VP += ws->Vp;
}
__global__ void k_add_vec(double *a, const double *b, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) a[i] += b[i];
}
__global__ void k_gather_e(const double *eR, const int *use, int nb, int64_t ldo, double *e64) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ldo; i += (int64_t)gridDim.x * blockDim.x)
    e64[i] = (i < nb) ? (double)(float)eR[use[i]] : 0.0;
}
__global__ void k_scale_d(double *v, int64_t n, double s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] *= s;
}
__global__ void k_set_bg(ChainScalars *sc, float bg) { sc->bg = bg; }
// posterior means (R/wgr.R:141-145)
__global__ void k_wgr_final(double *B, double *D, double *VB, int p, double mc, const double *dpart, int iv, WgrScalars *ws) {
  __shared__ double red[17];
  double sd = 0;
  for (int i = threadIdx.x; i < 256; i += blockDim.x) sd += dpart[i];
  sd = block_sum(sd, red);
  const double meanD = sd / mc / (double)p;
  for (int j = threadIdx.x; j < p; j += blockDim.x) { D[j] = D[j] / mc; B[j] = B[j] / mc / meanD; if (iv) VB[j] = VB[j] / mc; }
  if (threadIdx.x == 0) ws->sumD = sd;
}
__global__ void k_hat64_finish(const double *part, int64_t ld, int nchunks, int n, double B0, double *hat) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s = 0;
  for (int c = 0; c < nchunks; ++c) s += part[(int64_t)c * ld + i];
  hat[i] = B0 + s;
}
}  // namespace
