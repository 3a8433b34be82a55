// bwgr_amd/csrc/mrr_host.hip.h -- the host entries of mrr on a resident int8 panel and on a dense fp64 design (bwgr_mrr, bwgr_mrr_dense).
// Part of bwgr_hip.hip, which includes it after everything it uses (fail, HIPCHK, DevBufs, no_memory, d2h / h2d / zero, Guard, guard_busy,
// and mtfit_host.hip.h) and before the other fp64 families' entries, uvb_host.hip.h and kernels_host.hip.h; it defines no kernel.  What
// these entries do to Y and Z before a kernel runs is traits.h.
// ------------------------------------------------------------------------------------------------
// mrr / mrr_float (MRR3 / MRR3F, src/RcppEigen20230423.cpp:318-1080): the engine of mrr.hip.h as a per-block launch train
//   per sweep:  order (host std::shuffle, cumulative) -> k_permute_cols -> k_mrr_gram -> k_mrr_linv ->
//               [k_mrr_pass(b-1 | b), k_mrr_solve(b)] for every block -> k_mrr_pass(last | -) -> k_mrr_ey -> (host: ve) ->
//               k_mrr_tilde -> (host: vb, GC, bending, pinv) -> k_mrr_mu_shift (updateMu)
// The sweep itself (order .. closing pass) is mrr_sweep of mtfit_host.hip.h, and the fit's device arrays and repeated steps are MtFit's, there:
// bwgr_mrr is a fit with one panel effect, centred.  What is left here is mrr's own algebra.
// ------------------------------------------------------------------------------------------------
// k and the options of bwgr_mrr and bwgr_mrr_dense (`who`), from one table: defaults, refusals and the checks on what is read
static int mrr_read_opts(const char *who, int k, const double *opts, int nopts, MrrOpts &o) {
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "%s: k = %d traits; this engine takes 1 <= k <= %d", who, k, BWGR_MRR_MAXK);
  if (nopts < 0 || nopts > BWGR_MRR_NOPTS || (nopts > 0 && !opts)) return fail(BWGR_EINVAL, "%s: nopts = %d (at most %d)", who, nopts, BWGR_MRR_NOPTS);
  double O[BWGR_MRR_NOPTS] = BWGR_MRR_DEFAULTS;
  const double D0[BWGR_MRR_NOPTS] = BWGR_MRR_DEFAULTS;
  for (int i = 0; i < nopts; ++i) O[i] = opts[i];
  {
    static const struct { int id; const char *name; } refused[] = {
      {BWGR_MRR_NLFACTOR, "NLfactor / NonLinearFactor"}, {BWGR_MRR_INNERGS, "InnerGS"}, {BWGR_MRR_NOINV, "NoInv"}, {BWGR_MRR_PENCOR, "PenCor"},
      {BWGR_MRR_MINCOR, "MinCor"}, {BWGR_MRR_UNCORH2BELOW, "uncorH2below"}, {BWGR_MRR_ROUNDGCUPFROM, "roundGCupFrom"}, {BWGR_MRR_ROUNDGCUPTO, "roundGCupTo"},
      {BWGR_MRR_ROUNDGCDOWNFROM, "roundGCdownFrom"}, {BWGR_MRR_ROUNDGCDOWNTO, "roundGCdownTo"}, {BWGR_MRR_BUCKETGCFROM, "bucketGCfrom"},
      {BWGR_MRR_BUCKETGCTO, "bucketGCto"}, {BWGR_MRR_DEFLATEBY, "DeflateBy"}};
    for (const auto &r : refused)
      if (O[r.id] != D0[r.id]) return fail(BWGR_EINVAL, "%s: option %s = %g is not supported (only its default, %g)", who, r.name, O[r.id], D0[r.id]);
  }
  o.maxit = (int)O[BWGR_MRR_MAXIT]; o.tol = O[BWGR_MRR_TOL]; o.TH = O[BWGR_MRR_TH] != 0; o.HCS = O[BWGR_MRR_HCS] != 0; o.XFA = O[BWGR_MRR_XFA] != 0;
  o.ACS = O[BWGR_MRR_ACS] != 0; o.NumXFA = (int)O[BWGR_MRR_NUMXFA]; o.R2 = O[BWGR_MRR_R2]; o.gc0 = O[BWGR_MRR_GC0]; o.df0 = O[BWGR_MRR_DF0];
  o.updateMu = O[BWGR_MRR_UPDATEMU] != 0; o.wph2 = O[BWGR_MRR_WEIGHT_PRIOR_H2]; o.wpgc = O[BWGR_MRR_WEIGHT_PRIOR_GC];
  o.OneVarB = O[BWGR_MRR_ONEVARB] != 0; o.OneVarE = O[BWGR_MRR_ONEVARE] != 0; o.verbose = O[BWGR_MRR_VERBOSE] != 0;
  if (o.maxit < 0) return fail(BWGR_EINVAL, "%s: maxit = %d", who, o.maxit);
  if ((o.XFA || o.ACS) && (o.NumXFA < 1 || o.NumXFA > k))
    return fail(BWGR_EINVAL, "%s: NumXFA = %d with XFA / ACS needs 1 <= NumXFA <= k = %d (the reference indexes eigenvalue k - NumXFA)", who, o.NumXFA, k);
  return BWGR_OK;
}

struct MrrOut { double *mu, *b, *hat, *h2, *GC, *vb, *ve, *MSx, *cnvB, *cnvH2, *cnvV; int *its; };
static int mrr_iterate(MtFit &M, const TraitSet &S, const MrrOpts &o, std::vector<double> &iG, const MrrOut &res);

extern "C" int bwgr_mrr(bwgr_panel *P, const double *Y, int k, const double *opts, int nopts, double *mu_out, double *b_out, double *hat_out,
                        double *h2_out, double *GC_out, double *vb_out, double *ve_out, double *MSx_out, double *cnvB, double *cnvH2, double *cnvV,
                        int *its) {
  if (!P || !Y || !b_out || !its) return fail(BWGR_EINVAL, "mrr: null pointer");
  MrrOpts o;
  CHK(mrr_read_opts("mrr", k, opts, nopts, o));
  if (P->data->is_f32) return fail(BWGR_EINVAL, "mrr: the panel holds fp32 genotypes; mrr takes int8 panels only");
  const int64_t n = P->data->n;
  const bwgr_pegs_effect_ex one = {P, nullptr, 0, 0, nullptr, nullptr, nullptr, 0};
  MtList E;
  CHK(mt_check_effects("mrr", "b", &one, 1, n, P->data->device, &b_out, E));                        // (nothing left to refuse: the panel's device, ld and stream)
  // (the int32 pattern Grams sum over at most n rows: n * max|x|^2 < 2^31 holds for every int8 panel, panel_build_gram)
  // ---- host set-up (:742-816): nt, mu and the centred y (:746-761); vy with iN = 1/(n-1) (:781-782) ----
  const TraitSet S = read_traits(Y, n, k, E.ld, k, RowRule::AtLeastTwo);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "mrr: trait %d has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  // missingness patterns: traits with the same observed rows share one masked Gram
  const Patterns pat = find_patterns(S, 0, k);
  std::vector<double> iG((size_t)k * k, 0.0);     // (copied from asynchronously: before the fit, whose holder waits for the stream)
  MtFit M(E, k);
  M.masks(S, pat);
  M.alloc(hat_out != nullptr, false);
  if (M.bufs.failed()) return no_memory("mrr");
  CHK(M.upload(S, S.sumy.data()));                                                                 // e = y, :825
  CHK(M.stage_effect(0));                                                                          // b = 0, :823
  CHK(M.setup_effect(0, 1));
  const MrrOut out = {mu_out, b_out, hat_out, h2_out, GC_out, vb_out, ve_out, MSx_out, cnvB, cnvH2, cnvV, its};
  return mrr_iterate(M, S, o, iG, out);
}

// mrr's own algebra after the set-up of its one effect (a panel, centred implicitly, or a dense design on the train, centred in its copy): MSx,
// the start values, the iterations and the outputs.  iG (k x k, zeros) is the caller's: it is copied from asynchronously and outlives M.
static int mrr_iterate(MtFit &M, const TraitSet &S, const MrrOpts &o, std::vector<double> &iG, const MrrOut &res) {
  const int k = M.k;
  const int64_t n = M.n, p = M.eff[0].m;
  double *const mu_out = res.mu, *const b_out = res.b, *const hat_out = res.hat, *const h2_out = res.h2, *const GC_out = res.GC, *const vb_out = res.vb,
         *const ve_out = res.ve, *const MSx_out = res.MSx, *const cnvB = res.cnvB, *const cnvH2 = res.cnvH2, *const cnvV = res.cnvV;
  int *const its = res.its;
  const std::vector<double> &nt = S.nt, &vy = S.vy;
  std::vector<double> mu = S.mu;
  const MtEffect &F = M.eff[0];
  MrrConst &mc = M.mc;
  std::vector<double> &d = M.d, &off = M.off;
  // a reduction over p of the k^2 (+k) products, partials in a fixed order
  auto reduce_pk = [&](int mode, int nout, const double *dvec, std::vector<double> &out) -> int {
    out.resize(nout);
    return M.reduce(F.b(), F.tilde(), F.XSX(), p, mode, nout, dvec, out.data());
  };
  std::vector<double> MSx;
  CHK(reduce_pk(2, k, nullptr, MSx));                                                              // MSx = colSums(XSX), :777
  // ---- start values (:784-816) ----
  std::vector<double> ve(k), vbInit(k), veInit(k), h2(k), TrXSX(k), Se(k), iNp(k), iN(k);
  std::vector<double> vb((size_t)k * k, 0.0), Sb((size_t)k * k), GC((size_t)k * k, 0.0), TH_((size_t)k * k), Tr(k);
  for (int t = 0; t < k; ++t) {
    TrXSX[t] = nt[t] * MSx[t];                                                                     // :778
    ve[t] = vy[t] * (1 - o.R2); veInit[t] = ve[t];                                                 // :784, :788
    vbInit[t] = vy[t] * o.R2 / MSx[t];                                                             // :787
    vb[t * k + t] = vbInit[t]; iG[t * k + t] = 1.0 / vbInit[t];                                    // :789-790 (iG before the covariances)
    h2[t] = 1 - ve[t] / vy[t];                                                                     // :791
    Se[t] = ve[t] * o.df0; iNp[t] = 1.0 / (nt[t] + o.df0 - 1); iN[t] = 1.0 / (nt[t] - 1);          // :817-818, :781
  }
  for (int i = 0; i < k; ++i) for (int j = 0; j < i; ++j) vb[i * k + j] = vb[j * k + i] = o.gc0 * sqrt(vb[i * k + i] * vb[j * k + j]);   // :796-804
  for (int i = 0; i < k * k; ++i) Sb[i] = vb[i] * o.df0;                                           // :816
  for (int i = 0; i < k * k; ++i) GC[i] = vb[i];
  // ---- iterations ----
  const double logtol = log10(o.tol);
  std::vector<double> ey, db2h(k), vb0, h20;
  int numit = 0;
  while (numit < o.maxit) {
    vb0 = vb; h20 = h2;
    for (int t = 0; t < k; ++t) mc.iVe[t] = 1.0 / ve[t];
    CHK(M.sweep_effect(0, numit, iG.data()));                                                      // :869 (cumulative, as there)
    // residual variance (:916-924)
    ey.resize(2 * k);
    CHK(M.residual_sums(ey.data()));
    CHK(M.read_db2(0, db2h.data()));
    for (int t = 0; t < k; ++t) {
      ve[t] = (ey[t] + Se[t]) * iNp[t];                                                            // :916-917
      h2[t] = 1 - ve[t] / vy[t];                                                                   // :918 (before the prior)
      if (o.wph2 > 0) ve[t] = ve[t] * (1 - o.wph2) + o.wph2 * veInit[t];                           // :920
    }
    if (o.OneVarE) { double m = 0; for (int t = 0; t < k; ++t) m += ve[t]; m /= k; for (int t = 0; t < k; ++t) ve[t] = m; }   // :922
    // TildeHat (:928-936): the TH form reads this iteration's ve and the sweep's iG
    for (int t = 0; t < k; ++t) { mc.iVe[t] = 1.0 / ve[t]; d[t] = iG[t * k + t]; }
    std::vector<double> th;
    if (o.TH) {
      CHK(M.stage_vec(d));
      CHK(reduce_pk(1, k * k + k, M.vecd, th));
      for (int t = 0; t < k; ++t) Tr[t] = th[k * k + t];
    } else {
      CHK(reduce_pk(0, k * k, nullptr, th));
      for (int t = 0; t < k; ++t) Tr[t] = TrXSX[t];
    }
    // th[s * k + t] = sum_j b_js tilde_jt = TildeHat(s, t)
    for (int i = 0; i < k * k; ++i) TH_[i] = th[i];
    int bent = 0;
    mrr_tail_vb(k, o, TH_.data(), Tr.data(), Sb.data(), vbInit.data(), vb.data(), GC.data(), iG.data(), &bent);
    if (bent && o.verbose) printf("Inflate (it=%d)\n", numit);
    if (o.updateMu) {                                                                              // :1030-1036
      for (int t = 0; t < k; ++t) { d[t] = ey[k + t] * iN[t]; mu[t] += d[t]; }
      CHK(M.mu_shift());
    }
    double mx = -INFINITY;
    for (int t = 0; t < k; ++t) mx = std::max(mx, db2h[t]);
    const double cnv = log10(mx);                                                                  // :1040-1041
    if (cnvB) cnvB[numit] = cnv;
    if (std::isnan(cnv)) { if (o.verbose) printf("Numerical issue! Job aborted (it=%d)\n", numit); break; }
    double s2 = 0, s3 = 0;
    for (int t = 0; t < k; ++t) s2 += (h20[t] - h2[t]) * (h20[t] - h2[t]);
    for (int i = 0; i < k * k; ++i) s3 += (vb0[i] - vb[i]) * (vb0[i] - vb[i]);
    if (cnvH2) cnvH2[numit] = log10(s2);                                                           // :1042
    if (cnvV) cnvV[numit] = log10(s3);                                                             // :1043
    ++numit;
    if (o.verbose && numit % 100 == 0) printf("Iter: %d || Conv: %g\n", numit, cnv);
    if (cnv < logtol) { if (o.verbose) printf("Model coverged in %d iterations\n", numit); break; }
    if (numit == o.maxit && o.verbose) printf("Model did not converge\n");
  }
  // ---- fitted values for every row, the missing ones included (:1054-1055) ----
  CHK(M.read_b(0, b_out));                                                                         // p x k column-major
  if (F.train) {
    for (int t = 0; t < k; ++t) off[t] = mu[t];                                                    // (the copy is centred: no offset but mu)
  } else {
    std::vector<double> xb((size_t)p);
    HIPCHK(d2h(M.st, xb.data(), F.leg.xbar, sizeof(double) * p));
    for (int t = 0; t < k; ++t) { double s = 0; for (int64_t j = 0; j < p; ++j) s += xb[(size_t)j] * b_out[(size_t)t * p + j]; off[t] = mu[t] - s; }
  }
  if (hat_out) {
    CHK(M.stage_vec(off));
    if (F.train) CHK(M.train_hat(0, M.hatd)); else CHK(M.panel_hat(0, M.hatd));
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(M.st, hat_out, M.hatd, sizeof(double) * n * k));
  }
  for (int t = 0; t < k; ++t) {
    if (mu_out) mu_out[t] = mu[t];
    if (h2_out) h2_out[t] = h2[t];
    if (ve_out) ve_out[t] = ve[t];
    if (MSx_out) MSx_out[t] = MSx[t];
  }
  for (int i = 0; i < k; ++i)
    for (int j = 0; j < k; ++j) {   // column-major, as R's matrices (both are symmetric)
      if (GC_out) GC_out[j * k + i] = GC[i * k + j];
      if (vb_out) vb_out[j * k + i] = vb[i * k + j];
    }
  *its = numit;
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// mrr on a dense fp64 design: mrr(Y, dense(X)), mkr(Y, K) = MRR3(Y, K2X(K)) (R/mix.R:1275) -- the train of mrr_dense.hip.h
//   once:       X -> the engine's padded copy, k_mrrd_centre (explicit centring, :763-765), k_mrrd_setup
//   per sweep:  order -> k_mrrd_gram -> k_mrr_linv -> [k_mrrd_pass(b-1 | b), k_mrrd_solve(b)] for every block -> k_mrrd_pass(last | -), then
//               bwgr_mrr's tail (mrr_iterate)
// A fit with one effect on the dense train (MtFit, mrrd_sweep); options, defaults, refusals and outputs are bwgr_mrr's (mrr_read_opts).  What such a fit
// does around its iterate is mrr_dense_fit, which bwgr_mrr_svd_fit (mrr_svd_host.hip.h) shares.
// ------------------------------------------------------------------------------------------------
// What a fit with one effect on the dense train does around its own algebra, for bwgr_mrr_dense and bwgr_mrr_svd_fit (`who`): the refusals of
// the shape, the host copy of a host X, the traits and their patterns, the workspace against the device's free memory, the fit's arrays and the
// set-up of its effect; then iterate(M, S, iG).  natural: the sweeps walk the columns in their natural order.
template <typename F>
static int mrr_dense_fit(const char *who, int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, bool want_hat,
                         bool natural, F iterate) {
  if (r < 1 || r > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "%s: r = %lld columns of X (at least 1, at most 2147483392)", who, (long long)r);
  if (n < 2) return fail(BWGR_EINVAL, "%s: n = %lld rows (at least 2)", who, (long long)n);
  if (ldx < n) return fail(BWGR_EINVAL, "%s: ldx = %lld is below n = %lld", who, (long long)ldx, (long long)n);
  const int64_t ld = (n + 127) / 128 * 128;
  std::vector<double> Xh;                         // host X with the engine's column stride (copied from asynchronously: before the fit)
  if (memloc == BWGR_HOST) {
    Xh.assign((size_t)ld * (size_t)r, 0.0);
    for (int64_t j = 0; j < r; ++j)
      for (int64_t i = 0; i < n; ++i) {
        const double v = X[(size_t)j * (size_t)ldx + (size_t)i];
        if (!std::isfinite(v)) return fail(BWGR_EINVAL, "%s: X[%lld, %lld] is not finite", who, (long long)i, (long long)j);
        Xh[(size_t)j * (size_t)ld + (size_t)i] = v;
      }
  }
  CHK(require_device(device));
  const bwgr_pegs_effect_ex one = {nullptr, X, r, ldx, nullptr, nullptr, nullptr, 0};
  MtList E;
  E.eff = &one; E.neff = 1; E.n = n; E.ld = ld; E.st = nullptr; E.train = true;
  E.Zc.resize(1); E.csr.resize(1); E.disjoint.assign(1, 0);
  const TraitSet S = read_traits(Y, n, k, E.ld, k, RowRule::AtLeastTwo);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "%s: trait %d of Y has %g observed rows (needs 2)", who, (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns pat = find_patterns(S, 0, k);
  {
    const MrrDensePlan pl = mrr_dense_plan(n, r, k, (int)pat.rep.size());
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (pl.ws_bytes > free_b)
      return fail(BWGR_EINVAL, "%s: n = %lld, r = %lld, k = %d need a device workspace of %zu bytes; %zu are free", who, (long long)n, (long long)r, k, pl.ws_bytes, free_b);
  }
  std::vector<double> iG((size_t)k * k, 0.0);     // (copied from asynchronously: before the fit, whose holder waits for the stream)
  MtFit M(E, k);
  M.natural_order = natural;
  M.masks(S, pat);
  M.alloc(want_hat, false);
  if (M.bufs.failed()) return no_memory(who);
  CHK(M.upload(S, nullptr));                                                                       // e = y, :825 (nothing reads the traits' sums: xbar = 0)
  CHK(M.stage_train(0, memloc == BWGR_HOST ? Xh.data() : X, memloc == BWGR_HOST ? ld : ldx, memloc == BWGR_DEVICE));
  CHK(M.stage_effect(0));                                                                          // b = 0, :823
  CHK(M.setup_effect(0, 0));
  return iterate(M, S, iG);
}

extern "C" int bwgr_mrr_dense(int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, const double *opts, int nopts,
                              double *mu_out, double *b_out, double *hat_out, double *h2_out, double *GC_out, double *vb_out, double *ve_out, double *MSx_out,
                              double *cnvB, double *cnvH2, double *cnvV, int *its) {
  if (!X || !Y || !b_out || !its) return fail(BWGR_EINVAL, "mrr_dense: null pointer");
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "mrr_dense: bad memloc %d", memloc);
  MrrOpts o;
  CHK(mrr_read_opts("mrr_dense", k, opts, nopts, o));
  const MrrOut out = {mu_out, b_out, hat_out, h2_out, GC_out, vb_out, ve_out, MSx_out, cnvB, cnvH2, cnvV, its};
  return mrr_dense_fit("mrr_dense", device, X, memloc, n, r, ldx, Y, k, hat_out != nullptr, false,
                       [&](MtFit &M, const TraitSet &S, std::vector<double> &iG) { return mrr_iterate(M, S, o, iG, out); });
}
