// bwgr_amd/csrc/mlm_host.hip.h -- the host entries of MLM (src/RcppEigen20230423.cpp:1260-1407): the projection
// Zp = Z - X (X'X)^-1 X'Z of a resident int8 panel or a dense design on a set of covariates (bwgr_project; the kernels are project.hip.h), the
// fixed-effects multi-trait fit on the dense block train staged by it (bwgr_mlm), and their plan (bwgr_debug_mlm_plan).  Part of bwgr_hip.hip,
// after mrr_svd_host.hip.h, whose xta_plan the panel's Z'X takes; it defines no kernel.  The k x k work after a sweep is mlm_tail.h, what happens
// to Y and X before a kernel runs is pegsx_setup.h's read_fixed.
// ------------------------------------------------------------------------------------------------
// The plan, decided here and nowhere else (bwgr_debug_mlm_plan exposes it to the CPU tests): the train's plan on Zp, and the projection's.
struct ProjPlan { int64_t rows, tiles, gx, gy, trips, pieces, fp, groups; size_t lds, ws_bytes; };
static ProjPlan proj_plan(int64_t n, int64_t p, int64_t f) {
  ProjPlan pl;
  pl.rows = (n + 127) / 128 * 128;                  // the train's ld
  pl.tiles = pl.rows / PROJ_T;
  pl.gx = (p + PROJ_T - 1) / PROJ_T;
  pl.gy = std::min<int64_t>(pl.tiles, PROJ_GY_MAX);
  pl.trips = (pl.tiles + pl.gy - 1) / pl.gy;
  pl.fp = std::min<int64_t>(f, PROJ_FP);
  pl.pieces = (f + pl.fp - 1) / pl.fp;
  pl.groups = (f + XTA_KT - 1) / XTA_KT;
  pl.lds = proj_lds((int)pl.fp);
  pl.ws_bytes = sizeof(double) * ((size_t)n * (size_t)f + (size_t)pl.groups * (size_t)pl.rows * XTA_KT + 2 * (size_t)p * (size_t)f);   // X, its staged copy (a panel pads it to its slab height), Z'X, C
  return pl;
}
extern "C" int bwgr_debug_mlm_plan(int64_t n, int64_t p, int64_t f, int k, int npat, int64_t out[BWGR_MLM_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "mlm plan: null pointer");
  if (n < 2 || p < 1 || p > 0x7FFFFF00ll || f < 1 || f > PROJ_FMAX || k < 1 || k > BWGR_MRR_MAXK || npat < 1 || npat > k)
    return fail(BWGR_EINVAL, "mlm plan: n = %lld (at least 2), p = %lld (1 .. 2147483392), f = %lld (1 <= f <= %d), k = %d (1 <= k <= %d), npat = %d (1 <= npat <= k)",
                (long long)n, (long long)p, (long long)f, PROJ_FMAX, k, BWGR_MRR_MAXK, npat);
  CHK(bwgr_debug_mrr_dense_plan(n, p, k, npat, out));
  const ProjPlan pl = proj_plan(n, p, f);
  const int64_t v[BWGR_MLM_PLAN_NOUT - BWGR_MRR_DENSE_PLAN_NOUT] = {pl.gx, pl.gy, pl.trips, pl.pieces, pl.fp, (int64_t)pl.lds, pl.groups, (int64_t)pl.ws_bytes,
                                                                  out[BWGR_MRR_DENSE_PLAN_NOUT - 1] + (int64_t)pl.ws_bytes};
  std::copy(v, v + (BWGR_MLM_PLAN_NOUT - BWGR_MRR_DENSE_PLAN_NOUT), out + BWGR_MRR_DENSE_PLAN_NOUT);
  return BWGR_OK;
}

// Test and probe hook: with mode = 1 the projection's steps wait for the stream and keep their wall-clock milliseconds -- out[0] X'X and its
// eigen-decomposition (host), out[1] X onto the device, its staging and Z'X, out[2] Z'X back, C = (X'X)^-1 X'Z on the host and C onto the device,
// out[3] k_project -- of the last bwgr_project or bwgr_mlm of the process; mode = 0 (the default) times nothing.  out may be null.
static int g_proj_timing = 0;
static double g_proj_ms[BWGR_PROJECT_TIMING_NOUT] = {0.0, 0.0, 0.0, 0.0};
extern "C" int bwgr_debug_project_timing(int mode, double out[BWGR_PROJECT_TIMING_NOUT]) {
  if (mode != 0 && mode != 1) return fail(BWGR_EINVAL, "project timing: mode = %d (0 or 1)", mode);
  g_proj_timing = mode;
  if (out) std::copy(g_proj_ms, g_proj_ms + BWGR_PROJECT_TIMING_NOUT, out);
  return BWGR_OK;
}
static double proj_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ------------------------------------------------------------------------------------------------
// Z as the projection reads it: a panel, or a dense matrix on the device
struct ProjSrc { const bwgr_panel *P; const double *Zd; int64_t ldz; };

// What `who` (project or mlm) refuses of Z and X before anything touches the device
static int proj_check(const char *who, const bwgr_panel *P, const double *Z, int zloc, int64_t n, int64_t p, int64_t ldz, const double *X, int64_t f, int64_t ldx) {
  if (!X || (!P && !Z)) return fail(BWGR_EINVAL, "%s: null pointer (X, or Z without a panel)", who);
  if (f < 1 || f > PROJ_FMAX) return fail(BWGR_EINVAL, "%s: f = %lld covariates; this entry takes 1 <= f <= %d", who, (long long)f, PROJ_FMAX);
  if (n < 2) return fail(BWGR_EINVAL, "%s: n = %lld rows (at least 2)", who, (long long)n);
  if (ldx < n) return fail(BWGR_EINVAL, "%s: ldx = %lld is below n = %lld", who, (long long)ldx, (long long)n);
  if (P) {
    if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: the panel holds fp32 genotypes; %s takes int8 panels or a dense Z", who, who);
    if (P->data->n != n) return fail(BWGR_EINVAL, "%s: Z has %lld rows, X and Y %lld", who, (long long)P->data->n, (long long)n);
    if (P->data->p != p) return fail(BWGR_EINVAL, "%s: p = %lld, the panel has %lld columns", who, (long long)p, (long long)P->data->p);
    if (P->data->plan.R % XTA_RT != 0) return fail(BWGR_EINVAL, "%s: the panel's slabs have %d rows, not a multiple of %d", who, P->data->plan.R, XTA_RT);
  } else {
    if (zloc != BWGR_HOST && zloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "%s: bad memloc %d of Z", who, zloc);
    if (p < 1 || p > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "%s: p = %lld columns of Z (at least 1, at most 2147483392)", who, (long long)p);
    if (ldz < n) return fail(BWGR_EINVAL, "%s: Z has a column stride of %lld rows, X and Y have n = %lld", who, (long long)ldz, (long long)n);
    if (zloc == BWGR_HOST)
      for (int64_t j = 0; j < p; ++j)
        for (int64_t i = 0; i < n; ++i)
          if (!std::isfinite(Z[(size_t)j * (size_t)ldz + (size_t)i])) return fail(BWGR_EINVAL, "%s: Z[%lld, %lld] is not finite", who, (long long)i, (long long)j);
  }
  return BWGR_OK;
}

// (X'X)^-1 over all n rows of the compact n x f X, rows added in ascending order; refused where the float rank rule drops a direction
static int proj_design(const char *who, const std::vector<double> &Xc, int64_t n, int64_t f, std::vector<double> &iXX) {
  const size_t nf = (size_t)f, nn = (size_t)n;
  const double t0 = proj_now_ms();
  std::vector<double> A(nf * nf), ratios(nf);
  for (size_t a = 0; a < nf; ++a)
    for (size_t c = a; c < nf; ++c) {
      const double *xa = Xc.data() + a * nn, *xc = Xc.data() + c * nn;
      double s = 0.0;
      for (size_t r = 0; r < nn; ++r) s += xa[r] * xc[r];
      A[a * nf + c] = A[c * nf + a] = s;
    }
  iXX.assign(nf * nf, 0.0);
  if (pegsx_pinv((int)f, A.data(), iXX.data(), ratios.data()) < (int)f)
    return fail(BWGR_EINVAL, "%s: X'X over all rows is rank-deficient at float precision: its smallest eigenvalue is %.3g of its largest, the rule asks for more than f 2^-23 = %.3g (f = %lld)",
                who, *std::min_element(ratios.begin(), ratios.end()), (double)f * 0x1p-23, (long long)f);
  g_proj_ms[0] = proj_now_ms() - t0;
  return BWGR_OK;
}

// The device side of C = (X'X)^-1 X'Z: X (compact, host) onto the device, Z'X, the product with iXX on the host, C back.  Xd (n x f), As, ZtX and
// Cd (f x p) are the caller's arrays; returns when Cd is complete (so Xc, iXX and the host copy may go away).
struct ProjBufs { double *Xd = nullptr, *As = nullptr, *ZtX = nullptr, *Cd = nullptr; int64_t lda = 0; };
static void proj_alloc(DevBufs &bufs, ProjBufs &B, const ProjSrc &src, int64_t n, int64_t p, int64_t f) {
  const ProjPlan pl = proj_plan(n, p, f);
  B.lda = src.P ? xta_plan(n, p, f, src.P->data->plan.R).ld : pl.rows;
  B.Xd = bufs.get<double>((size_t)n * (size_t)f); B.As = bufs.get<double>((size_t)pl.groups * (size_t)B.lda * XTA_KT);
  B.ZtX = bufs.get<double>((size_t)p * (size_t)f); B.Cd = bufs.get<double>((size_t)p * (size_t)f);
}
static int proj_coeffs(hipStream_t st, const ProjBufs &B, const ProjSrc &src, int64_t n, int64_t p, int64_t f, const std::vector<double> &Xc, const std::vector<double> &iXX) {
  const ProjPlan pl = proj_plan(n, p, f);
  const bool timing = g_proj_timing != 0;
  if (timing) HIPCHK(hipStreamSynchronize(st));
  const double t0 = proj_now_ms();
  HIPCHK(h2d(st, B.Xd, Xc.data(), (size_t)n * (size_t)f));
  const int64_t staged = pl.groups * XTA_KT * B.lda;
  hipLaunchKernelGGL(k_xta_stage, dim3((unsigned)std::min<int64_t>((staged + 255) / 256, 4096)), dim3(256), 0, st, (const double *)B.Xd, n, n, f, B.lda, pl.groups, B.As);
  if (src.P) {
    const XtaPlan xp = xta_plan(n, p, f, src.P->data->plan.R);
    XtaArgs a;
    a.X = (const int8_t *)src.P->data->X; a.R = src.P->data->plan.R; a.p = p; a.ld = xp.ld; a.n = n; a.As = B.As; a.sA = nullptr; a.k = f; a.nblk = xp.nblk; a.centre = 0;
    a.out = B.ZtX; a.ldo = p;
    hipLaunchKernelGGL(k_xta, dim3((unsigned)xp.grid, (unsigned)xp.groups), dim3(256), 0, st, a);
  } else {
    ProjZtxArgs a;
    a.Z = src.Zd; a.ldz = src.ldz; a.n = n; a.p = p; a.ld = B.lda; a.As = B.As; a.f = f; a.nblk = (p + XTA_WGC - 1) / XTA_WGC; a.out = B.ZtX; a.ldo = p;
    hipLaunchKernelGGL(k_proj_ztx, dim3((unsigned)std::min<int64_t>(a.nblk, XTA_WG_MAX), (unsigned)pl.groups), dim3(256), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  if (timing) HIPCHK(hipStreamSynchronize(st));
  const double t1 = proj_now_ms();
  const size_t nf = (size_t)f, np = (size_t)p;
  std::vector<double> ZtX(np * nf), C(np * nf);
  HIPCHK(d2h(st, ZtX.data(), B.ZtX, sizeof(double) * np * nf));
  for (size_t j = 0; j < np; ++j)
    for (size_t l = 0; l < nf; ++l) {
      double s = 0.0;
      for (size_t m = 0; m < nf; ++m) s += iXX[l * nf + m] * ZtX[m * np + j];
      C[j * nf + l] = s;
    }
  HIPCHK(h2d(st, B.Cd, C.data(), np * nf));
  HIPCHK(hipStreamSynchronize(st));
  if (timing) { g_proj_ms[1] = t1 - t0; g_proj_ms[2] = proj_now_ms() - t1; }
  return BWGR_OK;
}
// out = Z - X C on the rows 0 .. n-1 (pad: and zeros on the rows n .. rows-1 of the train's copy); out may be src.Zd
static int proj_launch(hipStream_t st, const ProjBufs &B, const ProjSrc &src, int64_t n, int64_t p, int64_t f, int pad, double *out, int64_t ldo) {
  const ProjPlan pl = proj_plan(n, p, f);
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_project), hipFuncAttributeMaxDynamicSharedMemorySize, (int)proj_lds(PROJ_FP)));
  ProjArgs a;
  a.Xp = src.P ? (const int8_t *)src.P->data->X : nullptr; a.R = src.P ? src.P->data->plan.R : 0; a.Zd = src.Zd; a.ldz = src.ldz;
  a.n = n; a.p = p; a.rows = pl.rows; a.X = B.Xd; a.ldx = n; a.C = B.Cd; a.f = (int)f; a.fp = (int)pl.fp; a.pad = pad; a.out = out; a.ldo = ldo;
  const bool timing = g_proj_timing != 0;
  if (timing) HIPCHK(hipStreamSynchronize(st));
  const double t0 = proj_now_ms();
  hipLaunchKernelGGL(k_project, dim3((unsigned)pl.gx, (unsigned)pl.gy), dim3(256), pl.lds, st, a);
  HIPCHK(hipGetLastError());
  if (timing) { HIPCHK(hipStreamSynchronize(st)); g_proj_ms[3] = proj_now_ms() - t0; }
  return BWGR_OK;
}

extern "C" int bwgr_project(int device, bwgr_panel *P, const double *Z, int zloc, int64_t n, int64_t p, int64_t ldz, const double *X, int64_t f, int64_t ldx,
                            double *out, int oloc, int64_t ldo) {
  if (!out) return fail(BWGR_EINVAL, "project: null pointer (out)");
  if (oloc != BWGR_HOST && oloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "project: bad memloc %d of out", oloc);
  CHK(proj_check("project", P, Z, zloc, n, p, ldz, X, f, ldx));
  if (ldo < n) return fail(BWGR_EINVAL, "project: ldo = %lld is below n = %lld", (long long)ldo, (long long)n);
  std::vector<double> Xc, iXX;
  int64_t br = -1, bc = -1;
  if (!compact_z(X, n, f, ldx, Xc, &br, &bc)) return fail(BWGR_EINVAL, "project: X[%lld, %lld] is not finite", (long long)br, (long long)bc);
  CHK(proj_design("project", Xc, n, f, iXX));
  if (P) HIPCHK(hipSetDevice(P->data->device)); else CHK(require_device(device));
  hipStream_t st = P ? P->stream : nullptr;
  const bool ztmp = !P && zloc == BWGR_HOST, otmp = oloc == BWGR_HOST && !ztmp;   // a host Z is projected in place in its device copy
  {
    size_t free_b = 0, total_b = 0;
    const size_t need = proj_plan(n, p, f).ws_bytes + ((ztmp || otmp) ? sizeof(double) * (size_t)n * (size_t)p : 0);
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) return fail(BWGR_EINVAL, "project: n = %lld, p = %lld, f = %lld need a device workspace of %zu bytes; %zu are free", (long long)n, (long long)p, (long long)f, need, free_b);
  }
  DevBufs bufs(st);
  double *tmp = (ztmp || otmp) ? bufs.get<double>((size_t)n * (size_t)p) : nullptr;
  ProjSrc src = {P, Z, ldz};
  ProjBufs B;
  proj_alloc(bufs, B, src, n, p, f);
  if (bufs.failed()) return no_memory("project");
  if (ztmp) {
    HIPCHK(hipMemcpy2DAsync(tmp, sizeof(double) * n, Z, sizeof(double) * ldz, sizeof(double) * n, (size_t)p, hipMemcpyHostToDevice, st));
    src.Zd = tmp; src.ldz = n;
  }
  CHK(proj_coeffs(st, B, src, n, p, f, Xc, iXX));
  double *dst = oloc == BWGR_DEVICE ? out : tmp;
  CHK(proj_launch(st, B, src, n, p, f, 0, dst, oloc == BWGR_DEVICE ? ldo : n));
  if (oloc == BWGR_HOST)
    HIPCHK(hipMemcpy2DAsync(out, sizeof(double) * ldo, tmp, sizeof(double) * n, sizeof(double) * n, (size_t)p, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// MLM: a fit with one effect on the dense train, staged by the projection and never centred.
//   once:       read_fixed (masks, MU, y) -> X'X, Z'X, C -> k_project into the train's copy -> k_mrrd_setup (ZZ, tilde) -> TrZSZ (k_mrr_tilde mode 2)
//   per sweep:  order -> k_mrrd_gram -> k_mrr_linv -> [k_mrrd_pass(b-1 | b), k_mrrd_solve(b)] for every block -> k_mrrd_pass(last | -) -> k_mrr_ey ->
//               k_mrr_tilde (mode 0) -> (host, mlm_tail.h: ve, vb, bending, pinv, cnv)
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_mlm(int device, bwgr_panel *P, const double *Z, int zloc, int64_t n, int64_t p, int64_t ldz, const double *X, int64_t f, int64_t ldx,
                        const double *Y, int k, int maxit, double logtol, double df0, int verb, double *b_out, double *u_out, double *hat_out, double *h2_out,
                        double *GC_out, double *vb_out, double *ve_out, double *cnv_out, int *its) {
  if (!Y || !u_out || !its) return fail(BWGR_EINVAL, "mlm: null pointer (Y, u or its)");
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "mlm: k = %d traits; this engine takes 1 <= k <= %d", k, BWGR_MRR_MAXK);
  if (maxit < 0) return fail(BWGR_EINVAL, "mlm: maxit = %d", maxit);
  if (std::isnan(logtol) || !std::isfinite(df0) || df0 < 0.0) return fail(BWGR_EINVAL, "mlm: logtol = %g, df0 = %g (logtol a number, df0 finite and >= 0)", logtol, df0);
  CHK(proj_check("mlm", P, Z, zloc, n, p, ldz, X, f, ldx));
  const int64_t ld = (n + 127) / 128 * 128;
  // ---- host set-up (:1269-1286): the masks, MU and the projected traits ----
  FixedSet F = read_fixed(Y, X, n, k, f, ldx, ld);
  if (F.bad_row >= 0) return fail(BWGR_EINVAL, "mlm: X[%lld, %lld] is not finite", (long long)F.bad_row, (long long)F.bad_col);
  for (int t = 0; t < k && (F.S.bad < 0 || t <= F.S.bad); ++t)
    if (F.S.nt[(size_t)t] <= (double)f)
      return fail(BWGR_EINVAL, "mlm: trait %d has n_t = %g records and f = %lld covariates (needs n_t > f)", t, F.S.nt[(size_t)t], (long long)f);
  for (int t = 0; t < k; ++t) {
    const size_t g = (size_t)F.pat.id[(size_t)t];
    if (F.rank[g] < (int)f)
      return fail(BWGR_EINVAL, "mlm: trait %d: M'M on its rows is rank-deficient at float precision: its smallest eigenvalue is %.3g of its largest, the rule asks for more than f 2^-23 = %.3g (f = %lld)",
                  t, *std::min_element(F.ratios.begin() + (ptrdiff_t)(g * (size_t)f), F.ratios.begin() + (ptrdiff_t)((g + 1) * (size_t)f)), (double)f * 0x1p-23, (long long)f);
  }
  std::vector<double> iXX;
  CHK(proj_design("mlm", F.X, n, f, iXX));                                                         // :1287
  if (P) HIPCHK(hipSetDevice(P->data->device)); else CHK(require_device(device));
  hipStream_t st = P ? P->stream : nullptr;
  const int npat = (int)F.pat.rep.size();
  {
    int64_t pl[BWGR_MLM_PLAN_NOUT];
    CHK(bwgr_debug_mlm_plan(n, p, f, k, npat, pl));
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if ((size_t)pl[BWGR_MLM_PLAN_NOUT - 1] > free_b)
      return fail(BWGR_EINVAL, "mlm: n = %lld, p = %lld, f = %lld, k = %d need a device workspace of %lld bytes (%lld of them the fp64 copy of the projected Z); %zu are free",
                  (long long)n, (long long)p, (long long)f, k, (long long)pl[BWGR_MLM_PLAN_NOUT - 1], (long long)(sizeof(double) * (size_t)ld * (size_t)p), free_b);
  }
  const bwgr_pegs_effect_ex one = {nullptr, Z, p, ldz, nullptr, nullptr, nullptr, 0};
  MtList E;
  E.eff = &one; E.neff = 1; E.n = n; E.ld = ld; E.st = st; E.train = true;
  E.Zc.resize(1); E.csr.resize(1); E.disjoint.assign(1, 0);
  MlmState T;                                       // (its iG is copied from asynchronously: before the fit, whose holder waits for the stream)
  T.iG.assign((size_t)k * k, 0.0);
  MtFit M(E, k);
  M.masks(F.S, F.pat);
  M.alloc(hat_out != nullptr, false);
  ProjSrc src = {P, Z, ldz};
  ProjBufs B;
  proj_alloc(M.bufs, B, src, n, p, f);
  if (M.bufs.failed()) return no_memory("mlm");
  CHK(M.upload(F.S, nullptr));                                                                     // e = y, :1300
  CHK(M.stage_train_by(0, [&](double *Zp, int64_t ldp) -> int {                                    // :1288
    if (!P && zloc == BWGR_HOST) {                  // a host Z goes into the copy and is projected in place
      HIPCHK(hipMemcpy2DAsync(Zp, sizeof(double) * ldp, Z, sizeof(double) * ldz, sizeof(double) * n, (size_t)p, hipMemcpyHostToDevice, st));
      src.Zd = Zp; src.ldz = ldp;
    }
    CHK(proj_coeffs(st, B, src, n, p, f, F.X, iXX));
    return proj_launch(st, B, src, n, p, f, 1, Zp, ldp);
  }));
  CHK(M.stage_effect(0));                                                                          // u = 0, :1298
  CHK(M.setup_effect(0, 0));                                                                       // ZZ, tilde, :1292, :1310
  const MtEffect &Fx = M.eff[0];
  std::vector<double> Tr((size_t)k), ey(2 * (size_t)k), TH((size_t)k * k), h2((size_t)k), GC((size_t)k * k);
  CHK(M.reduce(Fx.b(), Fx.tilde(), Fx.XX(), p, 2, k, nullptr, Tr.data()));                         // TrZSZ = colSums(ZZ), :1293
  mlm_start(T, k, (int)f, df0, F.S.nt.data(), F.ssy.data(), Tr.data());                            // :1303-1320 (iG keeps its storage)
  // ---- iterations (:1332-1382) ----
  while (T.numit < maxit) {
    for (int t = 0; t < k; ++t) M.mc.iVe[t] = 1.0 / T.ve[(size_t)t];
    CHK(M.sweep_effect(0, T.numit, T.iG.data()));                                                  // :1338-1351 (the order is cumulative, as there)
    CHK(M.residual_sums(ey.data()));
    double db2 = 0.0;
    CHK(M.effect_sums(0, TH.data(), &db2));                                                        // TildeHat, :1359 (ends in a wait: iG may change now)
    mlm_after_sweep(T, ey.data(), TH.data(), db2);
    if (verb) {                                                                                    // :1376-1380
      if (std::isnan(T.cnv)) { printf("Numerical issue! Job aborted (it=%d)\n", T.numit); break; }
      if (T.numit % 100 == 0) printf("Iter: %d || log10 Conv: %g\n", T.numit, T.cnv);
      if (T.cnv < logtol) { printf("Model coverged in %d iterations\n", T.numit); break; }
      if (T.numit == maxit) printf("Model did not converge\n");
    } else if (std::isnan(T.cnv)) break;
  }
  // ---- outputs (:1385-1402) ----
  CHK(M.read_b(0, u_out));                                                                         // p x k column-major
  if (hat_out) {                                                                                   // hat = Zp u + X MU on every row, :1386-1387
    CHK(M.stage_vec(M.off));                                                                       // (zeros)
    CHK(M.train_hat(0, M.hatd));
    HIPCHK(d2h(st, hat_out, M.hatd, sizeof(double) * n * k));
    for (int t = 0; t < k; ++t)
      for (int64_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (int64_t l = 0; l < f; ++l) s += F.X[(size_t)l * (size_t)n + (size_t)i] * F.b[(size_t)t * (size_t)f + (size_t)l];
        hat_out[(size_t)t * (size_t)n + (size_t)i] += s;
      }
  }
  mlm_finish(T, h2.data(), GC.data());
  if (b_out) std::copy(F.b.begin(), F.b.end(), b_out);                                             // f x k column-major
  for (int t = 0; t < k; ++t) {
    if (h2_out) h2_out[t] = h2[(size_t)t];
    if (ve_out) ve_out[t] = T.ve[(size_t)t];
  }
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {   // column-major, as R's matrices
      if (GC_out) GC_out[j * k + i] = GC[(size_t)i * k + j];
      if (vb_out) vb_out[j * k + i] = T.vb[(size_t)i * k + j];
    }
  if (cnv_out) *cnv_out = T.cnv;
  *its = T.numit;
  return BWGR_OK;
}
