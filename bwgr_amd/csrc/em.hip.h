// bwgr_amd/csrc/em.hip.h -- the EM / Gauss-Seidel family's kernels around the sweep: staging a sweep's per-marker inputs in sweep order and
// back, the start values on the device, and the members' tail.  Part of bwgr_hip.hip, which includes it after sweep.hip.h (ChainScalars); it
// defines no host function.  (The columns are put into sweep order by k_permute_cols, panel.hip.h.)
namespace {
struct EmState {
  float mu, ve, vb, Lmb, cnv, Sb, Se, Rho, cxx, df, vy, MSx;
  float va, Sa, Pi, Pi0, PriorPi, sumvx, R2, alpha, Lmb1, Lmb2, Sy, trAC22;
};

// per-marker inputs of one sweep, in sweep order: b, xx, lambda
__global__ void k_em_stage(const int32_t *__restrict__ order, int64_t p, int model, int weighted, const float *__restrict__ b,
                           const float *__restrict__ xx, const float *__restrict__ lam, const float *__restrict__ D,
                           const EmState *__restrict__ st, float *__restrict__ bq, float *__restrict__ xxq, float *__restrict__ lamq) {
  const float Lmb = st->Lmb, Lmb2 = st->Lmb2;
  for (int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; jj < p; jj += (int64_t)gridDim.x * blockDim.x) {
    const int j = order[jj];
    bq[jj] = b[j]; xxq[jj] = xx[j];
    float l;
    if (model == BWGR_EM_BA || model == BWGR_EM_DE || model == BWGR_EM_BB) l = lam[j];
    else if (model == BWGR_EM_BL || model == BWGR_EM_EN) l = Lmb2;                   // denominators Lmb2 + xx, :382, :434
    else if (model == BWGR_EM_LASSO) l = 0.0f;                                       // denominator xx, :1480
    else if (weighted) l = Lmb / D[j];                                               // :496
    else l = Lmb;
    lamq[jj] = l;
  }
}
__global__ void k_em_unstage(const int32_t *__restrict__ order, int64_t p, const float *__restrict__ bq, float *__restrict__ b,
                             const float *__restrict__ dq, float *__restrict__ d) {
  for (int64_t jj = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; jj < p; jj += (int64_t)gridDim.x * blockDim.x) {
    const int j = order[jj];
    b[j] = bq[jj];
    if (d) d[j] = dq[jj];
  }
}
__global__ void k_em_fix_xx(float *xx, int64_t p) {                                   // if(xx[k]==0) xx[k]=0.1f, :261
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < p; j += (int64_t)gridDim.x * blockDim.x) if (xx[j] == 0.0f) xx[j] = 0.1f;
}
__global__ void k_em_init(const float *__restrict__ y, double *__restrict__ e, int n, int64_t ld, EmState *st) {
  // mu = y.mean(); e = y.array()-mu  (float), :98-99; padding rows of e stay 0
  __shared__ double sh[1024];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 1024) s += (double)y[i];
  sh[threadIdx.x] = s; __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
  const float mu = (float)(sh[0] / (double)n);
  for (int64_t i = threadIdx.x; i < ld; i += 1024) e[i] = i < n ? (double)(y[i] - mu) : 0.0;
  if (threadIdx.x == 0) st->mu = mu;
}

struct EmTailArgs {
  int model, n, conv; int64_t p;
  double *e; const float *y; const float *b; const float *bc; const float *d; float *lam; float *vbv; const float *xx;
  EmState *st; ChainScalars *sc;
};

__device__ double em_block_sum(double v, double *sh) {
  __syncthreads();
  sh[threadIdx.x] = v; __syncthreads();
  for (int o = 512; o > 0; o >>= 1) { if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o]; __syncthreads(); }
  return sh[0];
}

// what follows a sweep, one workgroup: the model's variance components and lambda, then eM = e.mean(); mu += eM; e -= eM;
// last, the scalars the next sweep's kernels read (C, Pi0, Lmb1) are refreshed in the ChainScalars block
__global__ __launch_bounds__(1024) void k_em_tail(const EmTailArgs a) {
  __shared__ double sh[1024];
  EmState st = *a.st;
  const int n = a.n; const int64_t p = a.p; const int tid = threadIdx.x; const int model = a.model;
  const float df = st.df;
  float b2n = 0, e2n = 0, dmean = 0;
  if (model == BWGR_EM_RR || model == BWGR_EM_BC || model == BWGR_EM_BCPI || model == BWGR_EM_EN) {
    double s = 0; for (int64_t j = tid; j < p; j += 1024) s = fma((double)a.b[j], (double)a.b[j], s);
    b2n = (float)em_block_sum(s, sh);                                                // b.squaredNorm()
  }
  if (model == BWGR_EM_BC || model == BWGR_EM_BCPI) {
    double s = 0; for (int64_t j = tid; j < p; j += 1024) s += (double)a.d[j];
    dmean = (float)(em_block_sum(s, sh) / (double)p);                                // d.mean()
  }
  if (model == BWGR_EM_BA || model == BWGR_EM_BB || model == BWGR_EM_RR || model == BWGR_EM_BC || model == BWGR_EM_BCPI) {
    double s = 0; for (int i = tid; i < n; i += 1024) s = fma(a.e[i], a.e[i], s);
    e2n = (float)em_block_sum(s, sh);                                                // e.squaredNorm() (before centring)
  }
  if (model == BWGR_EM_BA || model == BWGR_EM_BB) {
    st.ve = (e2n + st.Se) / ((float)n + df);                                         // :113, :170
    for (int64_t j = tid; j < p; j += 1024) {
      const float bj = a.b[j];
      const float vbj = (st.Sb + bj * bj) / (df + 1);                                // :110, :167
      a.vbv[j] = vbj;
      a.lam[j] = st.ve * (1.0f / vbj);                                               // Lmb = ve * vb.cwiseInverse(), :114, :171
    }
  } else if (model == BWGR_EM_RR) {
    st.vb = (b2n + st.Sb) / ((float)p + df);                                         // :338
    st.ve = (e2n + st.Se) / ((float)n + df);                                         // :339
    st.Lmb = sqrtf(st.Rho * st.ve / st.vb);                                          // :340
  } else if (model == BWGR_EM_BC) {
    st.ve = (e2n + st.Se) / ((float)n + df);                                         // :229
    st.va = (b2n + st.Sa) / ((float)p + df) / (dmean - st.Pi);                       // :230
    st.Lmb = st.ve / st.va;                                                          // :231
  } else if (model == BWGR_EM_BCPI) {
    st.Pi = ((1.0f - dmean) * (float)p + st.PriorPi * df) / ((float)p + df);         // :1533
    st.Pi0 = (1.0f - st.Pi) / st.Pi;                                                 // :1534
    st.MSx = st.sumvx * st.Pi * (1.0f - st.Pi);                                      // :1535
    st.Sa = st.R2 * (df + 2) * st.vy / st.MSx;                                       // :1536
    st.ve = (e2n + st.Se) / ((float)n + df);                                         // :1538
    st.va = (b2n + st.Sa) / ((float)p + df) / (dmean - st.Pi);                       // :1539
    st.Lmb = st.ve / st.va;                                                          // :1540
  }
  {
    double s = 0; for (int i = tid; i < n; i += 1024) s += a.e[i];
    const float eM = (float)(em_block_sum(s, sh) / (double)n);                       // :115-117
    st.mu += eM;
    for (int i = tid; i < n; i += 1024) a.e[i] = a.e[i] - (double)eM;
    __syncthreads();
  }
  if (model == BWGR_EM_DE || model == BWGR_EM_EN) {
    double s = 0; for (int i = tid; i < n; i += 1024) s = fma(a.e[i], (double)a.y[i], s);
    st.ve = (float)em_block_sum(s, sh) / (float)(n - 1);                             // Ve = e.dot(y)/(n-1), :289, :445
  }
  if (model == BWGR_EM_DE) {
    for (int64_t j = tid; j < p; j += 1024) {
      const float bj = a.b[j];
      const float vbj = bj * bj + st.ve / (a.xx[j] + a.lam[j] + 0.0001f);            // :290
      a.vbv[j] = vbj;
      a.lam[j] = sqrtf(st.cxx * st.ve / vbj);                                        // :292
    }
  } else if (model == BWGR_EM_EN) {
    st.va = (b2n + st.trAC22 * st.ve) / (float)p;                                    // :446
    st.Lmb = st.ve / st.va;                                                          // :447
    st.Lmb1 = 0.5f * st.Lmb * st.alpha * st.Sy;                                      // :448
    st.Lmb2 = st.Lmb * (1 - st.alpha);                                               // :449
  } else if (model == BWGR_EM_ML) {
    double s1 = 0, s2 = 0;
    for (int i = tid; i < n; i += 1024) {
      const float ym = a.y[i] - st.mu;
      s1 = fma((double)ym, a.e[i], s1);                                              // :505
      s2 = fma((double)ym, (double)ym - a.e[i], s2);                                 // :506
    }
    const float d1 = (float)em_block_sum(s1, sh), d2 = (float)em_block_sum(s2, sh);
    st.ve = d1 / (float)n;
    st.vb = d2 / (float)((float)n * st.MSx);
    st.Lmb = st.ve / st.vb;                                                          // :507
  }
  if (a.conv) {
    double s = 0; for (int64_t j = tid; j < p; j += 1024) s += (double)fabsf(a.bc[j] - a.b[j]);
    st.cnv = (float)em_block_sum(s, sh);                                             // :295, :451, :509
  }
  if (tid == 0) {
    *a.st = st;
    a.sc->C = -0.5f / sqrtf(st.ve);                                                  // C of the next sweep, :157, :216, :1522
    a.sc->odds = st.Pi0;
    a.sc->lam = st.Lmb1;
  }
}

__global__ void k_em_fit_ml(const float *__restrict__ y, const double *__restrict__ e, float *__restrict__ hat, int n) {   // fit = y - e, :512
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) hat[i] = (float)((double)y[i] - e[i]);
}
}  // namespace
