// bwgr_amd/csrc/mrr_svd_host.hip.h -- the host entries of mrr_svd (src/RcppEigen20230423.cpp:1083-1260): the transpose
// product X'A on a resident int8 panel with its plan (bwgr_panel_xta, bwgr_debug_xta_plan; the kernels are xta.hip.h) and the reference's
// Gauss-Seidel on a given design (bwgr_mrr_svd_fit).  Part of bwgr_hip.hip, after mrr_host.hip.h, whose mrr_dense_fit the fit stands on; it
// defines no kernel.  The decomposition that makes the design, and the back-map through bwgr_panel_xta, are the host layers' (bwgr_amd/svd.py).
// ------------------------------------------------------------------------------------------------
// The plan of bwgr_panel_xta, decided here and nowhere else (bwgr_debug_xta_plan exposes it to the CPU tests).  ld: the rows of the slabs that
// hold a row of the panel (a panel made with more slab workgroups than its rows need has all-zero slabs behind them, which are not read).
struct XtaPlan { int64_t ld, groups, nblk, grid, trips, tiles; size_t ws_bytes; };
static XtaPlan xta_plan(int64_t n, int64_t p, int64_t k, int R) {
  XtaPlan pl;
  pl.ld = (n + R - 1) / R * R;
  pl.groups = (k + XTA_KT - 1) / XTA_KT;
  pl.nblk = (p + XTA_WGC - 1) / XTA_WGC;
  pl.grid = std::min<int64_t>(pl.nblk, XTA_WG_MAX);
  pl.trips = (pl.nblk + pl.grid - 1) / pl.grid;
  pl.tiles = pl.ld / XTA_RT;
  pl.ws_bytes = sizeof(double) * ((size_t)pl.groups * (size_t)pl.ld * XTA_KT + (size_t)pl.groups * XTA_KT);   // As, sA
  return pl;
}
extern "C" int bwgr_debug_xta_plan(int64_t n, int64_t p, int64_t k, int64_t R, int64_t out[BWGR_XTA_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "xta plan: null pointer");
  if (n < 1 || p < 1 || k < 1 || k > (int64_t)65535 * XTA_KT || R < XTA_RT || R > 4096 || R % XTA_RT != 0)
    return fail(BWGR_EINVAL, "xta plan: n = %lld, p = %lld, k = %lld (each at least 1, k at most %d), R = %lld (a multiple of %d, at most 4096)", (long long)n, (long long)p, (long long)k,
                65535 * XTA_KT, (long long)R, XTA_RT);
  const XtaPlan pl = xta_plan(n, p, k, (int)R);
  const int64_t v[BWGR_XTA_PLAN_NOUT] = {pl.groups, XTA_WGC, XTA_WVC, pl.grid, pl.trips, XTA_LDS, XTA_RT, pl.tiles, (int64_t)pl.ws_bytes};
  std::copy(v, v + BWGR_XTA_PLAN_NOUT, out);
  return BWGR_OK;
}

extern "C" int bwgr_panel_xta(bwgr_panel *P, const double *A, int64_t lda, int64_t k, int centre, int memloc, double *out, int64_t ldo) {
  if (!P || !A || !out) return fail(BWGR_EINVAL, "panel_xta: null pointer");
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "panel_xta: bad memloc %d", memloc);
  if (k < 1 || k > (int64_t)65535 * XTA_KT) return fail(BWGR_EINVAL, "panel_xta: k = %lld columns of A (at least 1, at most %d per call)", (long long)k, 65535 * XTA_KT);
  if (P->data->is_f32) return fail(BWGR_EINVAL, "panel_xta: the panel holds fp32 genotypes; panel_xta takes int8 panels only");
  const int64_t n = P->data->n, p = P->data->p;
  const int R = P->data->plan.R;
  if (lda < n) return fail(BWGR_EINVAL, "panel_xta: lda = %lld is below n = %lld", (long long)lda, (long long)n);
  if (ldo < p) return fail(BWGR_EINVAL, "panel_xta: ldo = %lld is below p = %lld", (long long)ldo, (long long)p);
  if (R % XTA_RT != 0) return fail(BWGR_EINVAL, "panel_xta: the panel's slabs have %d rows, not a multiple of %d", R, XTA_RT);
  if (memloc == BWGR_HOST)
    for (int64_t t = 0; t < k; ++t)
      for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(A[(size_t)t * (size_t)lda + (size_t)i])) return fail(BWGR_EINVAL, "panel_xta: A[%lld, %lld] is not finite", (long long)i, (long long)t);
  HIPCHK(hipSetDevice(P->data->device));
  const XtaPlan pl = xta_plan(n, p, k, R);
  hipStream_t st = P->stream;
  DevBufs bufs(st);
  double *As = bufs.get<double>((size_t)pl.groups * (size_t)pl.ld * XTA_KT), *sA = bufs.get<double>((size_t)pl.groups * XTA_KT);
  double *Ad = nullptr, *outd = nullptr;
  if (memloc == BWGR_HOST) { Ad = bufs.get<double>((size_t)n * (size_t)k); outd = bufs.get<double>((size_t)p * (size_t)k); }
  if (bufs.failed()) return no_memory("panel_xta");
  if (memloc == BWGR_HOST) {
    if (lda == n) HIPCHK(h2d(st, Ad, A, (size_t)n * (size_t)k));
    else HIPCHK(hipMemcpy2DAsync(Ad, sizeof(double) * n, A, sizeof(double) * lda, sizeof(double) * n, (size_t)k, hipMemcpyHostToDevice, st));
  }
  const int64_t staged = pl.groups * XTA_KT * pl.ld;
  hipLaunchKernelGGL(k_xta_stage, dim3((unsigned)std::min<int64_t>((staged + 255) / 256, 4096)), dim3(256), 0, st, memloc == BWGR_HOST ? (const double *)Ad : A,
                     memloc == BWGR_HOST ? n : lda, n, k, pl.ld, pl.groups, As);
  hipLaunchKernelGGL(k_xta_asum, dim3((unsigned)(pl.groups * XTA_KT)), dim3(256), 0, st, (const double *)As, n, pl.ld, sA);
  XtaArgs a;
  a.X = (const int8_t *)P->data->X; a.R = R; a.p = p; a.ld = pl.ld; a.n = n; a.As = As; a.sA = sA; a.k = k; a.nblk = pl.nblk; a.centre = centre != 0;
  a.out = memloc == BWGR_HOST ? outd : out; a.ldo = memloc == BWGR_HOST ? p : ldo;
  hipLaunchKernelGGL(k_xta, dim3((unsigned)pl.grid, (unsigned)pl.groups), dim3(256), 0, st, a);
  HIPCHK(hipGetLastError());
  if (memloc == BWGR_HOST) {
    if (ldo == p) HIPCHK(hipMemcpyAsync(out, outd, sizeof(double) * p * k, hipMemcpyDeviceToHost, st));
    else HIPCHK(hipMemcpy2DAsync(out, sizeof(double) * ldo, outd, sizeof(double) * p, sizeof(double) * p, (size_t)k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// mrr_svd's Gauss-Seidel (:1103-1243) on a given n x r design: a fit with one effect on the dense train (mrr_dense_fit), swept in the columns'
// natural order (:1176), with the reference's own variance update (mrr_svd_tail.h).
//   per sweep:  k_mrrd_gram -> k_mrr_linv -> [k_mrrd_pass(b-1 | b), k_mrrd_solve(b)] for every block -> k_mrrd_pass(last | -) -> k_mrr_ey ->
//               (host: ve, h2) -> k_mrr_tilde (mode 1: TildeHat and TrDinvXSX) -> (host, mrr_svd_tail.h: vb, bending, pinv, cnv)
// ------------------------------------------------------------------------------------------------
struct MrrSvdOut { double *mu, *b, *hat, *h2, *GC, *vb, *ve, *cnvB, *cnvH2, *cnvV; int *its; };
static int mrr_svd_iterate(MtFit &M, const TraitSet &S, int maxit, double tol, bool verbose, std::vector<double> &iG, const MrrSvdOut &res) {
  const int k = M.k;
  const int64_t n = M.n, r = M.eff[0].m;
  const MtEffect &F = M.eff[0];
  MrrConst &mc = M.mc;
  std::vector<double> MSx(k), ve(k), h2(k), iN(k), vb((size_t)k * k), GC((size_t)k * k), Tr(k), ey(2 * k), db2h(k), th((size_t)k * k + k), vb0, h20;
  CHK(M.reduce(F.b(), F.tilde(), F.XSX(), r, 2, k, nullptr, MSx.data()));                          // MSx = colSums(XSX), :1133
  mrr_svd_start(k, S.nt.data(), S.vy.data(), MSx.data(), ve.data(), vb.data(), iG.data(), h2.data(), iN.data());
  const double logtol = log10(tol);
  int numit = 0;
  while (numit < maxit) {
    vb0 = vb; h20 = h2;                                                                            // :1169-1172
    for (int t = 0; t < k; ++t) mc.iVe[t] = 1.0 / ve[t];
    CHK(M.sweep_effect(0, numit, iG.data()));                                                      // :1175-1187, the columns in their natural order
    CHK(M.residual_sums(ey.data()));
    CHK(M.read_db2(0, db2h.data()));
    for (int t = 0; t < k; ++t) {
      ve[t] = ey[t] * iN[t];                                                                       // :1190-1191
      h2[t] = 1.0 - ve[t] / S.vy[(size_t)t];                                                       // :1193
    }
    // TildeHat and TrDinvXSX (:1196-1199) with this iteration's ve and the sweep's iG
    for (int t = 0; t < k; ++t) { mc.iVe[t] = 1.0 / ve[t]; M.d[(size_t)t] = iG[(size_t)t * k + t]; }
    CHK(M.stage_vec(M.d));
    CHK(M.reduce(F.b(), F.tilde(), F.XSX(), r, 1, k * k + k, M.vecd, th.data()));
    for (int t = 0; t < k; ++t) Tr[t] = th[(size_t)k * k + t];
    int bent = 0; double minev = 0.0;
    mrr_svd_tail_vb(k, th.data(), Tr.data(), vb.data(), iG.data(), &bent, &minev);                 // :1201-1216
    if (bent && verbose) printf("Inflate (it=%d)\n", numit);
    double c1, c2, c3;
    mrr_svd_cnv(k, db2h.data(), h20.data(), h2.data(), vb0.data(), vb.data(), &c1, &c2, &c3);      // :1219-1221
    if (res.cnvB) res.cnvB[numit] = c1;
    if (res.cnvH2) res.cnvH2[numit] = c2;
    if (res.cnvV) res.cnvV[numit] = c3;
    ++numit;                                                                                       // :1224
    if (verbose && numit % 100 == 0) printf("Iter: %d || Conv: %g\n", numit, c1);
    if (c1 < logtol) { if (verbose) printf("Model coverged in %d iterations\n", numit); break; }
    if (std::isnan(c1)) break;                                                                     // :1227 (after the count, as there)
  }
  CHK(M.read_b(0, res.b));                                                                         // r x k column-major
  if (res.hat) {                                                                                   // hat = X b + mu for every row (:1233-1234); mu is never updated
    for (int t = 0; t < k; ++t) M.off[(size_t)t] = S.mu[(size_t)t];
    CHK(M.stage_vec(M.off));
    CHK(M.train_hat(0, M.hatd));
    HIPCHK(d2h(M.st, res.hat, M.hatd, sizeof(double) * n * k));
  }
  mrr_svd_gc(k, vb.data(), GC.data());                                                             // :1238-1241
  for (int t = 0; t < k; ++t) {
    if (res.mu) res.mu[t] = S.mu[(size_t)t];
    if (res.h2) res.h2[t] = h2[t];
    if (res.ve) res.ve[t] = ve[t];
  }
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {   // column-major, as R's matrices
      if (res.GC) res.GC[j * k + i] = GC[i * k + j];
      if (res.vb) res.vb[j * k + i] = vb[i * k + j];
    }
  *res.its = numit;
  return BWGR_OK;
}

extern "C" int bwgr_mrr_svd_fit(int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, int maxit, double tol, int verbose,
                                double *mu_out, double *b_out, double *hat_out, double *h2_out, double *GC_out, double *vb_out, double *ve_out, double *cnvB,
                                double *cnvH2, double *cnvV, int *its) {
  if (!X || !Y || !b_out || !its) return fail(BWGR_EINVAL, "mrr_svd_fit: null pointer");
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "mrr_svd_fit: bad memloc %d", memloc);
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "mrr_svd_fit: k = %d traits; this engine takes 1 <= k <= %d", k, BWGR_MRR_MAXK);
  if (maxit < 0) return fail(BWGR_EINVAL, "mrr_svd_fit: maxit = %d", maxit);
  const MrrSvdOut out = {mu_out, b_out, hat_out, h2_out, GC_out, vb_out, ve_out, cnvB, cnvH2, cnvV, its};
  return mrr_dense_fit("mrr_svd_fit", device, X, memloc, n, r, ldx, Y, k, hat_out != nullptr, true,
                       [&](MtFit &M, const TraitSet &S, std::vector<double> &iG) { return mrr_svd_iterate(M, S, maxit, tol, verbose != 0, iG, out); });
}
