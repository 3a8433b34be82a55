// bwgr_amd/csrc/chain.hip.h -- the kernels of the fused chains around the sweep: set-up, the per-iteration tails of one chain and of the
// two-panel models, finalisation, the snapshot and recovery of a fixed-point sweep that leaves its range, and the exchange rounds and sums
// of the sharded sampler and the group.  Part of bwgr_hip.hip, which includes it after sweep.hip.h, rng.hip.h (ChainScalars, Rng and the
// variates) and panel.hip.h (block_sum); it defines no host function.
namespace {
// ---- chain setup (src/Rcpp20260726ai.cpp:599-610 and the identical blocks of the other samplers) ----
struct InitArgs {
  const float *y; double *e; int n, p; int64_t ld; int model; float pi, df, R2; float MSx; ChainScalars *sc;
};
__global__ void k_chain_init(const InitArgs a) {
  __shared__ double red[17];
  double s = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) s += (double)a.y[i];
  s = block_sum(s, red);
  const float mu = (float)(s / (double)a.n);               // y.mean()
  double sv = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) { const float dev = a.y[i] - mu; const float sq = dev * dev; sv += (double)sq; }
  sv = block_sum(sv, red);
  const float vy = (float)(sv / (double)(float)(a.n - 1));   // fvar(y)
  for (int i = threadIdx.x; i < a.ld; i += blockDim.x) { const float t = (i < a.n) ? (a.y[i] - mu) : 0.0f; a.e[i] = (double)t; }
  if (threadIdx.x == 0) {
    float pi = a.pi;
    if (a.model == BWGR_BAYESCPI || a.model == BWGR_BAYESDPI) pi = 0.5f;
    float Sb;
    if (a.model == BWGR_BAYESC || a.model == BWGR_BAYESCPI) Sb = a.df * (a.R2) * vy / a.MSx / (1 - pi);
    else Sb = (a.R2) * a.df * vy / a.MSx;
    ChainScalars sc;
    memset(&sc, 0, sizeof(sc));
    sc.ve = vy; sc.vb = Sb; sc.lam = vy / Sb; sc.pi = pi;
    sc.Sb = Sb; sc.Se = (1 - a.R2) * a.df * vy; sc.C = -0.5f / sqrtf(vy); sc.odds = pi / (1.0f - pi);
    sc.mu = mu; sc.dfp1 = a.df + 1; sc.vy = vy; sc.MSx = a.MSx;
    sc.inc_rate = 1.0f - pi;
    *a.sc = sc;
  }
}
__global__ void k_marker_init(float *b, float *d, float *vb, float *lam, float *B, float *D, float *VB, int p,
                              const ChainScalars *sc) {
  const float Sb = sc->Sb, ve = sc->ve;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    b[j] = 0; d[j] = 0; B[j] = 0; D[j] = 0; VB[j] = 0;
    vb[j] = Sb;
    lam[j] = ve * (1.0f / Sb);   // ve * vb.cwiseInverse()
  }
}

// ---- per-iteration tail: intercept, residual / marker variances, pi (one workgroup) ----
struct TailArgs {
  double *e; int n, p; int model; float df, R2, Phi; int accumulate; uint32_t iter; Rng rng; ChainScalars *sc;
};
__global__ __launch_bounds__(1024) void k_tail(const TailArgs a) {
  __shared__ double red[17];
  ChainScalars &sc = *a.sc;
  const float ve0 = sc.ve;
  double s = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) s += a.e[i];
  s = block_sum(s, red);
  const float me = (float)(s / (double)a.n);                                        // e.mean()
  const double z = rng_normal(a.rng, RNG_GLOBAL_MARKER, a.iter, RNG_G_MU, 0);
  const float eM = (float)((double)me + (double)sqrtf(ve0 / a.n) * z);              // :620
  double ss = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) { const double v = a.e[i] - (double)eM; a.e[i] = v; ss = fma(v, v, ss); }
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) {
    const float ssf = (float)ss;                                                    // e.squaredNorm()
    const float b2f = (float)sc.sum_b2;                                             // b.squaredNorm()
    float ve = ve0, vb = sc.vb, pi = sc.pi, Sb = sc.Sb;
    const float mu = sc.mu + eM;
    const double chi_e = rng_chisq(a.rng, (double)(a.n + a.df), RNG_GLOBAL_MARKER, a.iter, RNG_G_VE);
    switch (a.model) {
      case BWGR_BAYESA: case BWGR_BAYESB: case BWGR_BAYESDPI: case BWGR_BAYESL:
        ve = (float)((double)(ssf + sc.Se) / chi_e);
        break;
      case BWGR_BAYESRR: {
        ve = (float)((double)(ssf + sc.Se) / chi_e);
        const double chi_b = rng_chisq(a.rng, (double)(a.p + a.df), RNG_GLOBAL_MARKER, a.iter, RNG_G_VB);
        vb = (float)((double)(b2f + Sb) / chi_b);
        sc.lam = ve / vb;
      } break;
      case BWGR_BAYESC: case BWGR_BAYESCPI: {
        const double chi_b = rng_chisq(a.rng, (double)(a.df + a.p), RNG_GLOBAL_MARKER, a.iter, RNG_G_VB);
        vb = (float)((double)(b2f + Sb) / chi_b);
        ve = (float)((double)(ssf + sc.Se) / chi_e);
        sc.lam = ve / vb;
      } break;
    }
    if (a.model == BWGR_BAYESCPI) {
      pi = (float)(sc.sum_d / (double)a.p);
      Sb = a.df * (a.R2) * sc.vy / sc.MSx / (1 - pi);
    }
    if (a.model == BWGR_BAYESDPI) pi = (float)(sc.sum_d / (double)a.p);
    sc.ve = ve; sc.vb = vb; sc.pi = pi; sc.Sb = Sb; sc.mu = mu;
    sc.C = -0.5f / sqrtf(ve);
    sc.inc_rate = (float)(sc.sum_d / (double)a.p);
    sc.sum_d = 0.0; sc.sum_b2 = 0.0;
    if (a.accumulate) { sc.MU += mu; sc.VE += ve; sc.VBs += vb; sc.Pi += pi; }
  }
}
// per-marker part of the tail: lambda_j for the next sweep and the posterior sums
__global__ void k_marker_tail(const float *b, const float *d, const float *vb, float *lam, float *B, float *D, float *VB,
                              int p, int model, float Phi, int accumulate, const ChainScalars *sc) {
  const float ve = sc->ve;
  const bool per = (model == BWGR_BAYESA || model == BWGR_BAYESB || model == BWGR_BAYESDPI || model == BWGR_BAYESL);
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    if (per) {
      const float v = vb[j];
      lam[j] = (model == BWGR_BAYESL) ? sqrtf(Phi * ve / v) : ve * (1.0f / v);
      if (accumulate) VB[j] += v;
    }
    if (accumulate) { B[j] += b[j]; D[j] += d[j]; }
  }
}

// ---- tail of the two-effect samplers (src/Rcpp20260726ai.cpp:1042-1047, :1138-1143, :1204-1210): one intercept and one
// residual variance from the shared residual; RR2 also draws the two common marker variances (second chi-square with
// the marker word RNG_GLOBAL_MARKER - 1).  Scalars are written to both chains' blocks; MU / VE accumulate in the first.
struct Tail2Args {
  double *e; int n, p1, p2; int rr; float df; int accumulate; uint32_t iter; Rng rng; ChainScalars *sc1, *sc2;
};
__global__ __launch_bounds__(1024) void k_tail2(const Tail2Args a) {
  __shared__ double red[17];
  ChainScalars &s1 = *a.sc1, &s2 = *a.sc2;
  const float ve0 = s1.ve;
  double s = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) s += a.e[i];
  s = block_sum(s, red);
  const float me = (float)(s / (double)a.n);
  const double z = rng_normal(a.rng, RNG_GLOBAL_MARKER, a.iter, RNG_G_MU, 0);
  const float eM = (float)((double)me + (double)sqrtf(ve0 / a.n) * z);
  double ss = 0;
  for (int i = threadIdx.x; i < a.n; i += blockDim.x) { const double v = a.e[i] - (double)eM; a.e[i] = v; ss = fma(v, v, ss); }
  ss = block_sum(ss, red);
  if (threadIdx.x == 0) {
    const float ssf = (float)ss;
    const float mu = s1.mu + eM;
    const double chi_e = rng_chisq(a.rng, (double)(a.n + a.df), RNG_GLOBAL_MARKER, a.iter, RNG_G_VE);
    const float ve = (float)((double)(ssf + s1.Se) / chi_e);
    if (a.rr) {
      const double c1 = rng_chisq(a.rng, (double)(a.df + a.p1), RNG_GLOBAL_MARKER, a.iter, RNG_G_VB);
      const double c2 = rng_chisq(a.rng, (double)(a.df + a.p2), RNG_GLOBAL_MARKER - 1u, a.iter, RNG_G_VB);
      s1.vb = (float)((double)(s1.Sb + (float)s1.sum_b2) / c1);
      s2.vb = (float)((double)(s2.Sb + (float)s2.sum_b2) / c2);
      s1.lam = ve / s1.vb; s2.lam = ve / s2.vb;
    }
    const float Cn = -0.5f / sqrtf(ve);
    s1.ve = ve; s2.ve = ve; s1.mu = mu; s2.mu = mu; s1.C = Cn; s2.C = Cn;
    s1.inc_rate = (float)(s1.sum_d / (double)a.p1); s2.inc_rate = (float)(s2.sum_d / (double)a.p2);
    s1.sum_d = 0.0; s1.sum_b2 = 0.0; s2.sum_d = 0.0; s2.sum_b2 = 0.0;
    if (a.accumulate) { s1.MU += mu; s1.VE += ve; s1.VBs += s1.vb; s2.VBs += s2.vb; }
  }
}
__global__ void k_set_rr2_start(ChainScalars *sc) { sc->lam = sc->MSx; }   // BayesRR2 starts with Lmb = MSx (:1190)
__global__ void k_hat2(const float *h1, const float *h2, float MU, float *hat, int n) {   // fit = X1*B1 + X2*B2; fit += MU
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { const float f = h1[i] + h2[i]; hat[i] = f + MU; }
}

// ---- finalisation ----
__global__ void k_final_markers(float *B, float *D, float *VB, float *pval, int p, float MCMC, int per) {
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < p; j += gridDim.x * blockDim.x) {
    B[j] /= MCMC; D[j] /= MCMC;
    if (per) VB[j] /= MCMC;
    if (pval) pval[j] = -1.0f * logf(1.0f - D[j]);
  }
}

// ---- a fixed-point sweep (k_sweep3 / k_sweep2w's fixed-point streamers) that leaves its range is redone on the fp64 residual:
// the state it starts from is kept (12 bytes per marker and the residual: 12 MB against a 10 GB read at C4), and when the range flag
// comes back the state is restored, the flag cleared and sc->redo set, which lets the fp64 launches queued behind (redo_only) run ----
struct SnapArgs { double *e, *se; float *b, *d, *vb, *sb, *sd, *svb; int64_t ld; int j0, j1; ChainScalars *sc; };
__global__ void k_range_snapshot(const SnapArgs s) {
  const int64_t nt = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < s.ld; i += nt) s.se[i] = s.e[i];
  for (int64_t j = s.j0 + t0; j < s.j1; j += nt) { s.sb[j] = s.b[j]; s.sd[j] = s.d[j]; if (s.vb) s.svb[j] = s.vb[j]; }
  if (t0 == 0) { s.sc->snap_sum_d = s.sc->sum_d; s.sc->snap_sum_b2 = s.sc->sum_b2; }
}
__global__ void k_range_recover(const SnapArgs s) {
  if (s.sc->error != 2u) return;
  const int64_t nt = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < s.ld; i += nt) s.e[i] = s.se[i];
  for (int64_t j = s.j0 + t0; j < s.j1; j += nt) { s.b[j] = s.sb[j]; s.d[j] = s.sd[j]; if (s.vb) s.vb[j] = s.svb[j]; }
}
__global__ void k_range_flag(ChainScalars *sc) {   // (after k_range_recover: every thread of it has read the status)
  if (sc->error == 2u) { sc->error = 0u; sc->redo = 1u; sc->nredo += 1u; sc->sum_d = sc->snap_sum_d; sc->sum_b2 = sc->snap_sum_b2; }
}
__global__ void k_redo_clear(ChainScalars *sc) { sc->redo = 0u; }
// ---- one exchange round of the marker-sharded sampler (bwgr_chain_round_sweep / bwgr_chain_round_apply) ----
__global__ void k_round_delta(const double *__restrict__ e, const double *__restrict__ e0, double *__restrict__ delta, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) delta[i] = e[i] - e0[i];
}
__global__ void k_round_apply(double *__restrict__ e, const double *__restrict__ e0, const double *__restrict__ delta, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) e[i] = e0[i] + delta[i];
}
}  // namespace

// ---- the iteration's sums over all shards, from the host and from the device ----
// (k_set_sums stands outside the unnamed namespace, as it always has: its symbol is one of the code object's kernel names)
__global__ void k_set_sums(ChainScalars *sc, double sd, double sb2) { sc->sum_d = sd; sc->sum_b2 = sb2; }
namespace {
__global__ void k_get_sums_dev(const ChainScalars *sc, double *out2) { out2[0] = sc->sum_d; out2[1] = sc->sum_b2; }
__global__ void k_set_sums_dev(ChainScalars *sc, const double *in2) { sc->sum_d = in2[0]; sc->sum_b2 = in2[1]; }
struct SumPtrs { const double *src[64]; };
__global__ void k_group_sum(const SumPtrs s, int G, double *out, int64_t count) {   // out = sum over the shards, in shard order (the same bits on every run)
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    double t = 0.0;
    for (int g = 0; g < G; ++g) t += s.src[g][i];
    out[i] = t;
  }
}
}  // namespace
