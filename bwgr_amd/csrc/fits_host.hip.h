// bwgr_amd/csrc/fits_host.hip.h -- the host entries of the fp64 fits and products on a resident int8 panel: mrr (and mrr on a dense fp64
// design, bwgr_mrr_dense), the UVBETA family with
// solver2x, the dense fits, X B, and the relationship kernels.  Part of bwgr_hip.hip, which includes it after everything it uses (fail, HIPCHK,
// DevBufs, no_memory, d2h / h2d / zero, Guard, guard_busy, and mtfit_host.hip.h); it defines no kernel.  What these entries do to Y and Z before
// a kernel runs is traits.h.
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
// A fit with one effect on the dense train (MtFit, mrrd_sweep); options, defaults, refusals and outputs are bwgr_mrr's (mrr_read_opts).
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_mrr_dense(int device, const double *X, int memloc, int64_t n, int64_t r, int64_t ldx, const double *Y, int k, const double *opts, int nopts,
                              double *mu_out, double *b_out, double *hat_out, double *h2_out, double *GC_out, double *vb_out, double *ve_out, double *MSx_out,
                              double *cnvB, double *cnvH2, double *cnvV, int *its) {
  if (!X || !Y || !b_out || !its) return fail(BWGR_EINVAL, "mrr_dense: null pointer");
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "mrr_dense: bad memloc %d", memloc);
  MrrOpts o;
  CHK(mrr_read_opts("mrr_dense", k, opts, nopts, o));
  if (r < 1 || r > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "mrr_dense: r = %lld columns of X (at least 1, at most 2147483392)", (long long)r);
  if (n < 2) return fail(BWGR_EINVAL, "mrr_dense: n = %lld rows (at least 2)", (long long)n);
  if (ldx < n) return fail(BWGR_EINVAL, "mrr_dense: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
  const int64_t ld = (n + 127) / 128 * 128;
  std::vector<double> Xh;                         // host X with the engine's column stride (copied from asynchronously: before the fit)
  if (memloc == BWGR_HOST) {
    Xh.assign((size_t)ld * (size_t)r, 0.0);
    for (int64_t j = 0; j < r; ++j)
      for (int64_t i = 0; i < n; ++i) {
        const double v = X[(size_t)j * (size_t)ldx + (size_t)i];
        if (!std::isfinite(v)) return fail(BWGR_EINVAL, "mrr_dense: X[%lld, %lld] is not finite", (long long)i, (long long)j);
        Xh[(size_t)j * (size_t)ld + (size_t)i] = v;
      }
  }
  CHK(require_device(device));
  const bwgr_pegs_effect_ex one = {nullptr, X, r, ldx, nullptr, nullptr, nullptr, 0};
  MtList E;
  E.eff = &one; E.neff = 1; E.n = n; E.ld = ld; E.st = nullptr; E.train = true;
  E.Zc.resize(1); E.csr.resize(1); E.disjoint.assign(1, 0);
  const TraitSet S = read_traits(Y, n, k, E.ld, k, RowRule::AtLeastTwo);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "mrr_dense: trait %d of Y has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns pat = find_patterns(S, 0, k);
  {
    const MrrDensePlan pl = mrr_dense_plan(n, r, k, (int)pat.rep.size());
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (pl.ws_bytes > free_b)
      return fail(BWGR_EINVAL, "mrr_dense: n = %lld, r = %lld, k = %d need a device workspace of %zu bytes; %zu are free", (long long)n, (long long)r, k, pl.ws_bytes, free_b);
  }
  std::vector<double> iG((size_t)k * k, 0.0);     // (copied from asynchronously: before the fit, whose holder waits for the stream)
  MtFit M(E, k);
  M.masks(S, pat);
  M.alloc(hat_out != nullptr, false);
  if (M.bufs.failed()) return no_memory("mrr_dense");
  CHK(M.upload(S, nullptr));                                                                       // e = y, :825 (nothing reads the traits' sums: xbar = 0)
  CHK(M.stage_train(0, memloc == BWGR_HOST ? Xh.data() : X, memloc == BWGR_HOST ? ld : ldx, memloc == BWGR_DEVICE));
  CHK(M.stage_effect(0));                                                                          // b = 0, :823
  CHK(M.setup_effect(0, 0));
  const MrrOut out = {mu_out, b_out, hat_out, h2_out, GC_out, vb_out, ve_out, MSx_out, cnvB, cnvH2, cnvV, its};
  return mrr_iterate(M, S, o, iG, out);
}

// ------------------------------------------------------------------------------------------------
// per-trait ridge fits: solver1x / UVBETA, solver1xF / FUVBETA, xsolver1xF / XFUVBETA, zsolver1xF / ZFUVBETA
// (src/RcppEigen20230423.cpp:1410-1443, :1506-1515, :1613-1646, :1709-1753, :1771-1816): the engine of uvb.hip.h
//   once:       k_uvb_setup, k_uvb_cols(TrXSX) per group of 64 traits
//   per sweep:  order (host std::shuffle, cumulative) -> k_permute_cols, then for every group with a trait still running:
//               k_mrr_gram -> [k_uvb_pass(b-1 | b), k_uvb_solve(b)] for every block -> k_uvb_pass(last | -) -> k_uvb_rows, k_uvb_cols;
//               one copy of every group's sums -> (host: mu, ve, vb, lambda, cnv, who stops) -> k_uvb_mu_shift
// ------------------------------------------------------------------------------------------------
// The plan, decided here and nowhere else (bwgr_debug_uvb_plan exposes it to the CPU tests): the groups, the solve's LDS (as many of a
// solve workgroup's Gram matrices as fit beside u), the pass's grid, and the element counts of the call's device arrays.
static constexpr int UVB_SHIFT_WG = 1024;     // workgroups of k_uvb_mu_shift per trait at most, 256 rows each per trip
static inline int64_t uvb_pass_grid(int64_t ld) { return std::min<int64_t>(ld / 64, UVB_PASS_WG); }
static inline int64_t uvb_shift_grid(int64_t n) { return std::min<int64_t>((n + TAIL_THREADS - 1) / TAIL_THREADS, UVB_SHIFT_WG); }
static inline int64_t uvb_xb_grid(int64_t n) { return (n + TAIL_THREADS - 1) / TAIL_THREADS; }
struct UvbPlan {
  int64_t groups, nblk, kpad; int ngl, G, nsolve; size_t lds_solve, lds_pass;
  size_t x_bytes, n_gram, n_zm, n_rows, n_cols, n_part, n_dB, n_tpart, n_res, n_slot, n_bout, n_xb;   // element counts
  size_t ws_bytes;
};
// npat_max: the most patterns any group has; npat_total: the patterns of all groups.  Negative: their bounds (every trait its own pattern),
// which is what is known before Y has been read.
static UvbPlan uvb_plan(int64_t n, int64_t ld, int64_t p, int64_t k, size_t x_bytes, int64_t npat_max, int64_t npat_total, bool want_xb) {
  UvbPlan pl;
  if (npat_max < 0) npat_max = std::min<int64_t>(k, UVB_W);
  if (npat_total < 0) npat_total = k;
  pl.groups = (k + UVB_W - 1) / UVB_W; pl.kpad = pl.groups * UVB_W; pl.nblk = (p + MRR_MB - 1) / MRR_MB;
  pl.nsolve = UVB_W / UVB_ST;
  pl.ngl = (int)std::min<size_t>((size_t)UVB_ST, (MRR_LDS_MAX - uvb_solve_lds(0)) / ((size_t)UVB_GSTR * 4));
  pl.lds_solve = uvb_solve_lds(pl.ngl); pl.lds_pass = UVB_PASS_LDS;
  pl.G = (int)uvb_pass_grid(ld);
  pl.x_bytes = x_bytes;
  pl.n_gram = (size_t)pl.nblk * (size_t)npat_max * MRR_MB * MRR_MB;      // int32: one group's block Gram matrices, rebuilt per sweep and group
  pl.n_zm = (size_t)npat_total * ld;                                      // bytes: the row masks k_mrr_gram ANDs with
  pl.n_rows = (size_t)pl.kpad * ld;                                       // doubles: y, e
  pl.n_cols = (size_t)pl.kpad * p;                                        // doubles: S, XX, tilde, b
  pl.n_part = (size_t)pl.G * (MRR_MB + 1) * UVB_W; pl.n_dB = (size_t)(MRR_MB + 1) * UVB_W;
  pl.n_tpart = (size_t)UVB_NP * 3 * UVB_W; pl.n_res = (size_t)pl.kpad * 6;
  pl.n_slot = (size_t)pl.groups * pl.nsolve * pl.ngl;
  pl.n_bout = (size_t)p * k; pl.n_xb = want_xb ? (size_t)n * k : 0;
  pl.ws_bytes = x_bytes + 4 * (size_t)p + 4 * std::max<size_t>(pl.n_gram, 1) + std::max<size_t>(pl.n_zm, 1) + 8 * (size_t)pl.groups * ld + 8 * (2 * pl.n_rows + 4 * pl.n_cols + pl.n_part + pl.n_dB + pl.n_tpart + pl.n_res) +
                8 * 2 * (size_t)pl.kpad /* db2, mu0 */ + sizeof(UvbTrait) * (size_t)pl.kpad + 4 * pl.n_slot + 8 * (pl.n_bout + pl.n_xb);
  return pl;
}
extern "C" int bwgr_debug_uvb_plan(int64_t n, int64_t p, int64_t k, int64_t out[BWGR_UVB_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "uvb plan: null pointer");
  if (n < 1 || p < 1 || k < 1) return fail(BWGR_EINVAL, "uvb plan: n = %lld, p = %lld, k = %lld (each at least 1)", (long long)n, (long long)p, (long long)k);
  const int64_t ld = (n + 127) / 128 * 128;
  const UvbPlan pl = uvb_plan(n, ld, p, k, (size_t)ld * p, -1, -1, true);
  out[0] = UVB_W; out[1] = pl.groups; out[2] = UVB_ST; out[3] = pl.ngl; out[4] = (int64_t)pl.lds_solve; out[5] = (int64_t)pl.lds_pass;
  out[6] = pl.G; out[7] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

// (bwgr_uvbeta_dense's plan, above its first user: the dense leg of bwgr_uvbeta2 carves its LDS up by the same rule)
// The plan, decided here and nowhere else (bwgr_debug_uvbd_plan exposes it to the CPU tests): whether a trait's residual lives in its
// workgroup's LDS or in a global workspace, the workgroup size, the dynamic LDS bytes and the bytes of that workspace.
struct UvbdPlan { int64_t lds_rows; bool e_in_lds; int threads; size_t lds_bytes, ws_bytes; };
static UvbdPlan uvbd_plan(int64_t n, int64_t q, int64_t k) {
  (void)q;   // (the per-column values live in global memory: the LDS carve-up does not depend on q)
  UvbdPlan pl;
  pl.lds_rows = (int64_t)((UVBD_LDS_MAX - UVBD_LDS_FIXED) / sizeof(double));
  pl.e_in_lds = n <= pl.lds_rows;
  pl.threads = (int)std::min<int64_t>(UVBD_TMAX, (n + 63) / 64 * 64);   // one row per thread up to 1024 rows, whole waves
  pl.lds_bytes = UVBD_LDS_FIXED + (pl.e_in_lds ? sizeof(double) * (size_t)n : 0);
  pl.ws_bytes = pl.e_in_lds ? 0 : sizeof(double) * (size_t)n * (size_t)k;
  return pl;
}

// ---- what bwgr_uvbeta, bwgr_uvbeta2 and bwgr_uvbeta_dense do alike ----
static int uvb_accept(const char *who, int64_t k, int64_t kmax, int variant, int maxit) {
  if (k < 1 || k > kmax) return fail(BWGR_EINVAL, "%s: k = %lld traits (at least 1)", who, (long long)k);
  if (variant < BWGR_UVB_D || variant > BWGR_UVB_Z) return fail(BWGR_EINVAL, "%s: unknown variant %d (0 solver1x, 1 solver1xF, 2 xsolver1xF, 3 zsolver1xF)", who, variant);
  if (maxit < 0) return fail(BWGR_EINVAL, "%s: maxit = %d", who, maxit);
  return BWGR_OK;
}
// Y on the traits' own rows, as submat_f / subvec_f select them (:1495-1503): nt, mu (:1413), the centred y (:1414), vy = y'y / (nt - 1) (:1419;
// y'Y = y'y: sum y = 0).  A trait without a row is an all-NaN trait: a zero column, no sweeps (:1510, :1713, :1811)
static int uvb_read(const char *who, const double *Y, int64_t n, int64_t k, int64_t ld, int64_t ycols, TraitSet &S) {
  S = read_traits(Y, n, k, ld, ycols, RowRule::NotOne);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "%s: trait %lld has one observed row (the variances divide by n - 1)", who, (long long)S.bad);
  return BWGR_OK;
}
static int z_unpadded(const char *who, const double *Z, int64_t n, int64_t q, int64_t ldz, std::vector<double> &Zc) {
  int64_t r = 0, j = 0;
  if (!compact_z(Z, n, q, ldz, Zc, &r, &j)) return fail(BWGR_EINVAL, "%s: Z[%lld, %lld] is not finite", who, (long long)r, (long long)j);
  return BWGR_OK;
}
// trait t's results: a trait without rows gives mu = h2 = 0 and no variances; xsolver1xF (noVar) estimates none
struct UvbOut { double *mu, *h2, *ve, *vb, *cnv; int *its; };
static void uvb_result(const UvbOut &o, int64_t t, bool none, int variant, double mu, double ve, double vb, double vy, double cnv, int its) {
  const bool noVar = variant == BWGR_UVB_X;
  if (o.mu) o.mu[t] = none ? 0.0 : mu;
  if (o.h2) o.h2[t] = none ? 0.0 : (noVar ? NAN : 1.0 - ve / vy);                                          // :1802
  if (o.ve) o.ve[t] = (none || noVar) ? NAN : ve;
  if (o.vb) o.vb[t] = (none || noVar) ? NAN : vb;
  if (o.cnv) o.cnv[t] = cnv;
  o.its[t] = its;
}

// the LDS slots of every solve workgroup: the first ngl distinct patterns among its 16 traits (UvbTrait::slot; -1: read from global memory)
static std::vector<int> uvb_slots(std::vector<UvbTrait> &tr, const UvbPlan &pl) {
  std::vector<int> slotpat(pl.n_slot, -1);
  for (int64_t g = 0; g < pl.groups; ++g)
    for (int sb = 0; sb < pl.nsolve; ++sb) {
      int *sp = slotpat.data() + ((size_t)g * pl.nsolve + sb) * pl.ngl;
      int used = 0;
      for (int tl = 0; tl < UVB_ST; ++tl) {
        UvbTrait &u = tr[(size_t)(g * UVB_W + sb * UVB_ST + tl)];
        if (u.nt == 0.0) continue;
        for (int s = 0; s < used && u.slot < 0; ++s) if (sp[s] == u.pat) u.slot = s;
        if (u.slot < 0 && used < pl.ngl) { sp[used] = u.pat; u.slot = used++; }
      }
    }
  return slotpat;
}

// a trait of uvb_run on the host; lam, lam1: the lambdas of the next sweep (UvbTrait::lam, Uvb2Trait::lam)
struct UvbState {
  double nt = 0, mu = 0, sumy = 0, vy = 0, TrXSX = 0, ve = NAN, vb = NAN, ve0 = 0, vb0 = 0, cnv = NAN, lam = 0; int its = 0; bool active = false;
  double TrXSX1 = 0, vb1 = NAN, vb01 = 0, lam1 = 0; bool skip1 = false, skip2 = false;   // (the dense design's; skip: TrXSX of that design is 0)
};
// a sweep's sums for one trait: of e, e'y, e'e over its rows; b'b, tilde'b and sum (delta b)^2 over the markers; leg: the dense leg's (or null)
struct UvbSums { double se, ey, ee, bb, tb, db2; const double *leg; };
// The tail of a trait that ran (:1433-1441, :1636-1644, :1739-1741, :1794-1801; leg given: solver2x's, :1478-1486, over q1 dense columns):
// mu, the variances, the lambdas, cnv and whether it goes on.  Returns mu0 = mean(e), which the caller takes off e.
static double uvb_update(UvbState &q, const UvbSums &s, int variant, int maxit, double logtol, double df0, int64_t p, int64_t q1) {
  const double m0 = s.se / q.nt;                                             // mu0 = mean(e); the sums below are those of e - mu0
  q.mu += m0;
  const double ey1 = s.ey - m0 * q.sumy, ee1 = s.ee - 2.0 * m0 * s.se + q.nt * m0 * m0;
  double d1 = 0.0;
  if (s.leg) {
    q.ve = (ee1 + ey1 + q.ve0) / (2.0 * q.nt - 1.0 + df0);                   // :1479-1481
    if (!q.skip1) {
      d1 = s.leg[0];
      q.vb1 = (s.leg[2] + s.leg[1] + q.vb01) / (q.TrXSX1 + (double)q1 + df0);   // :1482, :1484
      q.lam1 = q.ve / q.vb1;                                                 // :1485
    }
    if (!q.skip2) {
      q.vb = (s.tb + s.bb + q.vb0) / (q.TrXSX + (double)p + df0);            // :1483-1484
      q.lam = q.ve / q.vb;
    }
  } else if (variant == BWGR_UVB_D || variant == BWGR_UVB_F) {
    q.ve = (ey1 + ee1 + q.ve0) / (2.0 * q.nt - 1.0 + df0);                   // :1434-1436
    q.vb = (s.bb + s.tb + q.vb0) / (q.TrXSX + (double)p + df0);              // :1437-1439
    q.lam = q.ve / q.vb;
  } else if (variant == BWGR_UVB_Z) {
    q.ve = (ey1 + q.ve0) / (q.nt + df0);                                     // :1795-1796
    q.vb = (s.tb + q.vb0) / (q.TrXSX + df0);                                 // :1797-1798
    q.lam = q.ve / q.vb;
  }
  q.cnv = s.leg ? log10(d1 + s.db2) : log10(s.db2);                          // :1486; :1440
  ++q.its;
  if (q.cnv < logtol || q.its == maxit || std::isnan(q.cnv)) q.active = false;   // :1441, :1487
  return m0;
}

// The engine of bwgr_uvbeta and bwgr_uvbeta2.  D = nullptr: one design, the panel (solver1x and its kin).  D given (variant D only): solver2x
// (:1446-1493) -- in every sweep the dense design D->Z is walked first (k_uvb2_leg, uvb2.hip.h), then the panel, against one residual; each
// design has its own lambda and variance update; the panel's outputs are b_out and vb_out, the dense design's D->b1 and D->vb1.
struct Uvb2Dense { const double *Z; int64_t q, ldz; double *b1, *vb1; };
static int uvb_run(const char *who, bwgr_panel *P, const double *Y, int64_t k, int variant, int maxit, double tol, double df0, const Uvb2Dense *D, double *b_out,
                   double *mu_out, double *h2_out, double *ve_out, double *vb_out, int *its_out, double *cnv_out, double *xb_out) {
  if (!P || !Y || !b_out || !its_out || (D && (!D->Z || !D->b1))) return fail(BWGR_EINVAL, "%s: null pointer", who);
  CHK(uvb_accept(who, k, INT64_MAX, variant, maxit));
  if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: the panel holds fp32 genotypes; %s takes int8 panels only", who, who);
  if (D && (D->q < 1 || D->q > 0x7FFFFF00ll || D->ldz < P->data->n))
    return fail(BWGR_EINVAL, "%s: q = %lld columns of Z, ldz = %lld (q at least 1 and at most 2147483392, the int32 column ids; ldz at least n = %lld)", who, (long long)D->q, (long long)D->ldz, (long long)P->data->n);
  HIPCHK(hipSetDevice(P->data->device));
  const int64_t n = P->data->n, p = P->data->p, ld = P->data->plan.ld;
  const size_t nq = D ? (size_t)D->q : 0;
  std::vector<double> Zc;   // Z without its padding
  if (D) CHK(z_unpadded(who, D->Z, n, D->q, D->ldz, Zc));
  const int R = P->data->plan.R;
  // (the int32 pattern Grams sum over at most n rows: n * max|x|^2 < 2^31 holds for every int8 panel, panel_build_gram)
  UvbPlan pl = uvb_plan(n, ld, p, k, P->data->plan.x_bytes, -1, -1, xb_out != nullptr);   // (the pattern counts follow once Y has been read)
  const int64_t groups = pl.groups, kpad = pl.kpad;
  // ---- host set-up ----
  TraitSet S;
  CHK(uvb_read(who, Y, n, k, ld, kpad, S));
  const std::vector<double> &y = S.y;
  std::vector<UvbState> T((size_t)k);
  for (int64_t t = 0; t < k; ++t) {
    UvbState &q = T[(size_t)t];
    q.nt = S.nt[(size_t)t]; q.mu = S.mu[(size_t)t]; q.sumy = S.sumy[(size_t)t]; q.vy = S.vy[(size_t)t];
    q.active = q.nt > 0 && maxit > 0;
  }
  // per group of 64 traits: the observed-row word of every row, and the missingness patterns -- traits with the same observed rows share one masked Gram
  const UvbTrait idle = {0.0, 0.0, 0, -1, 0, 0};
  std::vector<UvbTrait> tr((size_t)kpad, idle);
  std::vector<unsigned long long> zb((size_t)groups * ld);
  std::vector<uint8_t> zm;
  std::vector<int> npat((size_t)groups, 0);
  std::vector<size_t> zm_off((size_t)groups, 0);
  for (int64_t g = 0; g < groups; ++g) {
    const int64_t t0 = g * UVB_W;
    const int kg = (int)std::min<int64_t>(UVB_W, k - t0);
    pack_row_bits(S, t0, kg, zb.data() + (size_t)g * ld);
    const Patterns pg = find_patterns(S, t0, t0 + kg);
    npat[(size_t)g] = (int)pg.rep.size(); zm_off[(size_t)g] = zm.size();
    append_byte_masks(S, pg.rep.data(), npat[(size_t)g], zm);
    for (int tl = 0; tl < kg; ++tl)
      if (pg.id[(size_t)tl] >= 0) { tr[(size_t)(t0 + tl)].nt = S.nt[(size_t)(t0 + tl)]; tr[(size_t)(t0 + tl)].pat = pg.id[(size_t)tl]; }
  }
  {
    int64_t npat_total = 0;
    for (int v : npat) npat_total += v;
    pl = uvb_plan(n, ld, p, k, P->data->plan.x_bytes, *std::max_element(npat.begin(), npat.end()), npat_total, xb_out != nullptr);
  }
  const std::vector<int> slotpat = uvb_slots(tr, pl);
  // ---- device arrays and uploads ----
  hipStream_t st = P->stream;
  CumulativeOrder order((size_t)p), order1(nq);
  std::vector<double> res(pl.n_res), db2h((size_t)kpad), mu0((size_t)kpad, 0.0);   // (copied to and from asynchronously: declared before the holder)
  std::vector<Uvb2Trait> tr1(D ? (size_t)kpad : 0);   // (the dense leg's: these too are copied to and from asynchronously)
  std::vector<double> leg(D ? (size_t)kpad * UVB2_NLEG : 0), trx1(D ? (size_t)kpad : 0);
  DevBufs bufs(st);
  const int64_t nblk = pl.nblk;
  const size_t nl = (size_t)ld, np = (size_t)p;
  int8_t *Xs = bufs.get<int8_t>(pl.x_bytes);
  int32_t *ordd = bufs.get<int32_t>(np), *gram = bufs.get<int32_t>(pl.n_gram);
  uint8_t *zmd = bufs.get<uint8_t>(pl.n_zm);   // (= zm.size())
  unsigned long long *zbd = bufs.get<unsigned long long>((size_t)groups * nl);
  double *yd = bufs.get<double>(pl.n_rows), *ed = bufs.get<double>(pl.n_rows);
  double *Sd = bufs.get<double>(pl.n_cols), *XXd = bufs.get<double>(pl.n_cols), *tilde = bufs.get<double>(pl.n_cols), *bd = bufs.get<double>(pl.n_cols);
  double *part = bufs.get<double>(pl.n_part), *dB = bufs.get<double>(pl.n_dB), *tpart = bufs.get<double>(pl.n_tpart), *resd = bufs.get<double>(pl.n_res);
  double *db2 = bufs.get<double>((size_t)kpad), *mu0d = bufs.get<double>((size_t)kpad);
  UvbTrait *trd = bufs.get<UvbTrait>((size_t)kpad);
  int *slotd = bufs.get<int>(pl.n_slot);
  double *bout = bufs.get<double>(pl.n_bout), *xbd = xb_out ? bufs.get<double>(pl.n_xb) : nullptr;
  if (bufs.failed()) return no_memory(who);
  // the dense design's arrays: Z, the traits' per-column values, the leg's sums; the leg's launch shape is uvbd_plan's
  const UvbdPlan dpl = uvbd_plan(n, D ? D->q : 1, k);
  Uvb2Args da;
  Uvb2Trait *tr1d = nullptr;
  int32_t *ord1d = nullptr;
  if (D) {
    const size_t nc = (size_t)kpad * nq;
    double *Zd = bufs.get<double>((size_t)n * nq), *c1 = bufs.get<double>(5 * nc), *trxd = bufs.get<double>((size_t)kpad), *legd = bufs.get<double>((size_t)kpad * UVB2_NLEG);
    tr1d = bufs.get<Uvb2Trait>((size_t)kpad); ord1d = bufs.get<int32_t>(nq);
    if (bufs.failed()) return no_memory(who);
    da.Z = Zd; da.n = n; da.q = D->q; da.ld = ld; da.y = yd; da.e = ed; da.zm = zmd; da.tr = tr1d; da.order = ord1d;
    da.zbar = c1; da.XX = c1 + nc; da.tilde = c1 + 2 * nc; da.b = c1 + 3 * nc; da.dlt = c1 + 4 * nc; da.trx = trxd; da.leg = legd;
    for (int64_t t = 0; t < kpad; ++t) {
      Uvb2Trait &u = tr1[(size_t)t];
      u.lam = 0.0; u.nt = tr[(size_t)t].nt; u.moff = (int64_t)(zm_off[(size_t)(t / UVB_W)] + (size_t)tr[(size_t)t].pat * nl); u.run = 0; u.pad_ = 0;
    }
    HIPCHK(h2d(st, Zd, Zc.data(), Zc.size()));
    HIPCHK(h2d(st, tr1d, tr1.data(), tr1.size()));
    HIPCHK(zero(st, c1, 5 * nc));                                                                     // b_1 = 0, :1458
    HIPCHK(zero(st, trxd, (size_t)kpad));
    HIPCHK(zero(st, legd, (size_t)kpad * UVB2_NLEG));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb2_leg<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVBD_LDS_MAX));
  }
  if (!zm.empty()) HIPCHK(h2d(st, zmd, zm.data(), zm.size()));
  HIPCHK(h2d(st, zbd, zb.data(), zb.size()));
  HIPCHK(h2d(st, yd, y.data(), pl.n_rows));
  HIPCHK(h2d(st, ed, y.data(), pl.n_rows));                                                           // e = y, :1422
  HIPCHK(h2d(st, trd, tr.data(), tr.size()));
  HIPCHK(h2d(st, slotd, slotpat.data(), pl.n_slot));
  HIPCHK(zero(st, bd, pl.n_cols));                                                                    // b = 0, :1421
  HIPCHK(zero(st, dB, pl.n_dB));
  HIPCHK(zero(st, part, pl.n_part));
  HIPCHK(zero(st, tpart, pl.n_tpart));
  HIPCHK(zero(st, resd, pl.n_res));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvb_pass), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVB_PASS_LDS));
  // the traits of group g that have rows / that still run
  auto mask_of = [&](int64_t g, bool running) {
    unsigned long long m = 0;
    for (int tl = 0; tl < UVB_W; ++tl) {
      const int64_t t = g * UVB_W + tl;
      if (t < k && (running ? T[(size_t)t].active : T[(size_t)t].nt > 0)) m |= 1ull << tl;
    }
    return m;
  };
  // sums over the markers of a group, partials in a fixed order, into resd[g][3 .. 4]
  auto cols = [&](int64_t g, int mode, unsigned long long act) {
    const size_t oc = (size_t)g * UVB_W * np;
    hipLaunchKernelGGL(k_uvb_cols, dim3(UVB_NP), dim3(256), 0, st, (const double *)(bd + oc), (const double *)(tilde + oc), (const double *)(XXd + oc), p, mode, act, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, UVB_NP, 2 * UVB_W, resd + (size_t)g * 6 * UVB_W + 3 * UVB_W);
  };
  for (int64_t g = 0; g < groups; ++g) {
    const unsigned long long have = mask_of(g, false);
    if (!have) continue;
    const int kg = (int)std::min<int64_t>(UVB_W, k - g * UVB_W);
    const size_t oc = (size_t)g * UVB_W * np, orow = (size_t)g * UVB_W * nl;
    hipLaunchKernelGGL(k_uvb_setup, dim3((unsigned)nblk), dim3(256), 0, st, (const int8_t *)P->data->X, R, p, ld, (const unsigned long long *)(zbd + (size_t)g * nl),
                       (const double *)(yd + orow), (const UvbTrait *)(trd + g * UVB_W), kg, Sd + oc, XXd + oc, tilde + oc);
    cols(g, 1, have);
  }
  if (D) {   // (after the copies of y and the masks above, on the same stream)
    hipLaunchKernelGGL(k_uvb2_setup, dim3((unsigned)k), dim3(dpl.threads), UVBD_LDS_FIXED, st, da);
    HIPCHK(hipMemcpyAsync(trx1.data(), da.trx, sizeof(double) * kpad, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, res.data(), resd, sizeof(double) * pl.n_res));
  for (int64_t t = 0; t < k; ++t) {
    UvbState &q = T[(size_t)t];
    if (q.nt == 0.0) continue;
    q.TrXSX = res[(size_t)(t / UVB_W) * 6 * UVB_W + 3 * UVB_W + (size_t)(t % UVB_W)];                    // :1418
    const double MSx = q.TrXSX / (q.nt - 1.0);                                                             // :1419
    if (variant == BWGR_UVB_X) { q.lam = q.TrXSX / (double)p; continue; }                      // lambda = XX.mean(), :1730
    q.ve = q.vy * 0.5; q.vb = (q.vy * 0.5) / MSx;                                                          // :1420
    q.lam = q.ve / q.vb; q.vb0 = q.vb * df0; q.ve0 = q.ve * df0;                               // :1423
    if (!D) continue;
    // solver2x's set-up of the two designs (:1455-1462).  A design with TrXSX = 0 on this trait's rows is skipped: its lambda is never
    // formed and its vb stays NaN; every XX of it is 0, so the panel leg leaves such a trait's b and e as they are
    q.skip2 = q.TrXSX == 0.0;
    if (q.skip2) { q.vb = NAN; q.vb0 = 0.0; q.lam = 0.0; }
    q.TrXSX1 = trx1[(size_t)t];
    q.skip1 = q.TrXSX1 == 0.0;
    if (q.skip1) continue;
    q.vb1 = (q.vy * 0.5) / (q.TrXSX1 / (q.nt - 1.0));                                                      // :1456-1457
    q.lam1 = q.ve / q.vb1; q.vb01 = q.vb1 * df0;                                               // :1461-1462
  }
  // ---- sweeps ----
  const int cps = (int)((size_t)R / 16);
  const double logtol = log10(tol), thr = variant == BWGR_UVB_F ? 0.00001 : 0.0;
  for (int sweep = 0; sweep < maxit; ++sweep) {
    bool any = false;
    for (int64_t t = 0; t < k; ++t) { tr[(size_t)t].lam = T[(size_t)t].lam; tr[(size_t)t].active = T[(size_t)t].active ? 1 : 0; any = any || T[(size_t)t].active; }
    if (!any) break;
    HIPCHK(h2d(st, ordd, order.next(sweep).data(), np));                                                   // :1428 (cumulative, as there)
    HIPCHK(h2d(st, trd, tr.data(), tr.size()));
    hipLaunchKernelGGL(k_permute_cols, dim3(8192), dim3(256), 0, st, (const uint4 *)P->data->X, (uint4 *)Xs, (const int32_t *)ordd, p, P->data->plan.K, cps);
    HIPCHK(zero(st, db2, (size_t)kpad));
    if (D) {
      for (int64_t t = 0; t < k; ++t) { tr1[(size_t)t].lam = T[(size_t)t].lam1; tr1[(size_t)t].run = (T[(size_t)t].active && !T[(size_t)t].skip1) ? 1 : 0; }
      HIPCHK(h2d(st, ord1d, order1.next(sweep).data(), nq));                                               // :1468 (cumulative, as there)
      HIPCHK(h2d(st, tr1d, tr1.data(), tr1.size()));
    }
    for (int64_t g = 0; g < groups; ++g) {
      const unsigned long long act = mask_of(g, true);
      if (!act) continue;
      const size_t oc = (size_t)g * UVB_W * np, orow = (size_t)g * UVB_W * nl;
      const int ng = npat[(size_t)g];
      if (D) {   // the dense leg (:1470-1473) of the group's running traits, in front of the panel's; one workgroup per trait of the group
        const unsigned kg = (unsigned)std::min<int64_t>(UVB_W, k - g * UVB_W);
        Uvb2Args ga = da;
        const size_t o1 = (size_t)g * UVB_W * nq;
        ga.y += orow; ga.e += orow; ga.tr += g * UVB_W; ga.zbar += o1; ga.XX += o1; ga.tilde += o1; ga.b += o1; ga.dlt += o1; ga.trx += g * UVB_W; ga.leg += (size_t)g * UVB_W * UVB2_NLEG;
        if (dpl.e_in_lds) hipLaunchKernelGGL(k_uvb2_leg<true>, dim3(kg), dim3(dpl.threads), dpl.lds_bytes, st, ga);
        else hipLaunchKernelGGL(k_uvb2_leg<false>, dim3(kg), dim3(dpl.threads), dpl.lds_bytes, st, ga);
      }
      int nsolve = 0;
      for (int sb = 0; sb < pl.nsolve; ++sb) if ((act >> (sb * UVB_ST)) & 0xFFFFull) nsolve = sb + 1;
      hipLaunchKernelGGL(k_mrr_gram, dim3((unsigned)nblk, (unsigned)((ng + 3) / 4)), dim3(256), 0, st, (const int8_t *)Xs, R, p, ld, (const uint8_t *)(zmd + zm_off[(size_t)g]), ng, gram);
      for (int64_t blk = 0; blk <= nblk; ++blk) {
        UvbPassArgs pa; pa.Xs = Xs; pa.R = R; pa.p = p; pa.ld = ld; pa.zb = zbd + (size_t)g * nl; pa.e = ed + orow; pa.dB = dB; pa.part = part;
        pa.prev = blk > 0 ? (int)(blk - 1) : -1; pa.next = blk < nblk ? (int)blk : -1; pa.act = act;
        hipLaunchKernelGGL(k_uvb_pass, dim3(pl.G), dim3(256), pl.lds_pass, st, pa);
        if (blk == nblk) break;
        UvbSolveArgs sa; sa.part = part; sa.G = pl.G; sa.order = ordd; sa.blk = (int)blk; sa.p = p; sa.gram = gram; sa.npat = ng; sa.S = Sd + oc; sa.XX = XXd + oc;
        sa.b = bd + oc; sa.dB = dB; sa.db2 = db2 + g * UVB_W; sa.tr = trd + g * UVB_W; sa.slotpat = slotd + (size_t)g * pl.nsolve * pl.ngl; sa.ngl = pl.ngl; sa.thr = thr;
        hipLaunchKernelGGL(k_uvb_solve, dim3(nsolve), dim3(256), pl.lds_solve, st, sa);
      }
      hipLaunchKernelGGL(k_uvb_rows, dim3(UVB_NP, UVB_W), dim3(256), 0, st, (const double *)(ed + orow), (const double *)(yd + orow), ld, act, tpart);
      hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, UVB_NP, 3 * UVB_W, resd + (size_t)g * 6 * UVB_W);
      cols(g, 0, act);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(db2h.data(), db2, sizeof(double) * kpad, hipMemcpyDeviceToHost, st));
    if (D) HIPCHK(hipMemcpyAsync(leg.data(), da.leg, sizeof(double) * kpad * UVB2_NLEG, hipMemcpyDeviceToHost, st));
    HIPCHK(d2h(st, res.data(), resd, sizeof(double) * pl.n_res));
    // the tail of every trait that ran
    for (int64_t t = 0; t < k; ++t) {
      mu0[(size_t)t] = 0.0;
      if (!T[(size_t)t].active) continue;
      const double *rg = res.data() + (size_t)(t / UVB_W) * 6 * UVB_W + (size_t)(t % UVB_W);
      const UvbSums sums = {rg[0], rg[UVB_W], rg[2 * UVB_W], rg[3 * UVB_W], rg[4 * UVB_W], db2h[(size_t)t], D ? leg.data() + (size_t)t * UVB2_NLEG : nullptr};
      mu0[(size_t)t] = uvb_update(T[(size_t)t], sums, variant, maxit, logtol, df0, p, D ? D->q : 0);
    }
    HIPCHK(h2d(st, mu0d, mu0.data(), mu0.size()));
    for (int64_t g = 0; g < groups; ++g) {
      unsigned long long ran = 0;
      for (int tl = 0; tl < UVB_W; ++tl) if (tr[(size_t)(g * UVB_W + tl)].active) ran |= 1ull << tl;   // (tr.active still says who ran this sweep)
      if (!ran) continue;
      hipLaunchKernelGGL(k_uvb_mu_shift, dim3((unsigned)uvb_shift_grid(n), UVB_W), dim3(TAIL_THREADS), 0, st, ed + (size_t)g * UVB_W * nl,
                         (const unsigned long long *)(zbd + (size_t)g * nl), ld, (int)n, ran, (const double *)(mu0d + g * UVB_W));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));   // mu0 is rewritten by the next sweep's tail
  }
  // ---- results ----
  for (int64_t g = 0; g < groups; ++g) {
    const int kg = (int)std::min<int64_t>(UVB_W, k - g * UVB_W);
    const size_t oc = (size_t)g * UVB_W * np;
    hipLaunchKernelGGL(k_uvb_b_out, dim3((unsigned)std::min<int64_t>((p * kg + 255) / 256, 4096)), dim3(256), 0, st, (const double *)(bd + oc), p, kg, bout + (size_t)g * UVB_W * np);
    if (xb_out)
      hipLaunchKernelGGL(k_uvb_xb, dim3((unsigned)uvb_xb_grid(n), (unsigned)((kg + 15) / 16)), dim3(TAIL_THREADS), 0, st, (const int8_t *)P->data->X, R, p, (int)n, (const double *)(bd + oc), kg,
                         xbd + (size_t)g * UVB_W * n);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, b_out, bout, sizeof(double) * pl.n_bout));
  if (xb_out) HIPCHK(d2h(st, xb_out, xbd, sizeof(double) * pl.n_xb));
  if (D) HIPCHK(d2h(st, D->b1, da.b, sizeof(double) * nq * (size_t)k));   // ([trait][q] = q x k, column-major)
  const UvbOut out = {mu_out, h2_out, ve_out, vb_out, cnv_out, its_out};
  for (int64_t t = 0; t < k; ++t) {
    const UvbState &q = T[(size_t)t];
    if (D && D->vb1) D->vb1[t] = q.vb1;
    uvb_result(out, t, q.nt == 0.0, variant, q.mu, q.ve, q.vb, q.vy, q.cnv, q.its);
  }
  return BWGR_OK;
}

extern "C" int bwgr_uvbeta(bwgr_panel *P, const double *Y, int64_t k, int variant, int maxit, double tol, double df0, double *b_out, double *mu_out,
                           double *h2_out, double *ve_out, double *vb_out, int *its_out, double *cnv_out, double *xb_out) {
  return uvb_run("uvbeta", P, Y, k, variant, maxit, tol, df0, nullptr, b_out, mu_out, h2_out, ve_out, vb_out, its_out, cnv_out, xb_out);
}

// solver2x (:1446-1493) for every column of Y: X1 = Z (dense, n x q), X2 = the panel
extern "C" int bwgr_uvbeta2(bwgr_panel *P, const double *Z, int64_t q, int64_t ldz, const double *Y, int64_t k, int maxit, double tol, double df0, double *b1_out,
                            double *b2_out, double *mu_out, double *h2_out, double *ve_out, double *vb1_out, double *vb2_out, int *its_out, double *cnv_out) {
  if (q < 1) return fail(BWGR_EINVAL, "uvbeta2: q = %lld columns of Z (at least 1)", (long long)q);
  if (!Z || !b1_out) return fail(BWGR_EINVAL, "uvbeta2: null pointer");
  const Uvb2Dense D = {Z, q, ldz, b1_out, vb1_out};
  return uvb_run("uvbeta2", P, Y, k, BWGR_UVB_D, maxit, tol, df0, &D, b2_out, mu_out, h2_out, ve_out, vb2_out, its_out, cnv_out, nullptr);
}

// ------------------------------------------------------------------------------------------------
// the same fits on a small dense design, and X B on the panel: the second stage and the products of XSEMF / ZSEMF / YSEMF
// (src/RcppEigen20230423.cpp:1756-1769, :1819-1874): the kernels of uvbd.hip.h
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_debug_uvbd_plan(int64_t n, int64_t q, int64_t k, int64_t out[BWGR_UVBD_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "uvbd plan: null pointer");
  if (n < 1 || q < 1 || k < 1) return fail(BWGR_EINVAL, "uvbd plan: n = %lld, q = %lld, k = %lld (each at least 1)", (long long)n, (long long)q, (long long)k);
  const UvbdPlan pl = uvbd_plan(n, q, k);
  out[0] = pl.lds_rows; out[1] = pl.e_in_lds ? 1 : 0; out[2] = pl.threads; out[3] = (int64_t)pl.lds_bytes; out[4] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

extern "C" int bwgr_uvbeta_dense(int device, const double *Z, int64_t n, int64_t q, int64_t ldz, const double *Y, int64_t k, int variant, int maxit,
                                 double tol, double df0, double *b_out, double *mu_out, double *h2_out, double *ve_out, double *vb_out, int *its_out,
                                 double *cnv_out) {
  if (!Z || !Y || !b_out || !its_out) return fail(BWGR_EINVAL, "uvbeta_dense: null pointer");
  if (n < 1 || q < 1 || q > 0x7FFFFF00ll || ldz < n) return fail(BWGR_EINVAL, "uvbeta_dense: n = %lld rows, q = %lld columns, ldz = %lld (n, q at least 1, ldz at least n)", (long long)n, (long long)q, (long long)ldz);
  CHK(uvb_accept("uvbeta_dense", k, 0x7FFFFFFFll, variant, maxit));
  CHK(require_device(device));
  const UvbdPlan pl = uvbd_plan(n, q, k);
  const size_t nn = (size_t)n, nq = (size_t)q, nk = (size_t)k;
  // ---- host set-up: Z without its padding; Y on the traits' own rows, the masks as 0/1 bytes; every sweep's order ----
  std::vector<double> Zc;
  CHK(z_unpadded("uvbeta_dense", Z, n, q, ldz, Zc));
  TraitSet S;
  CHK(uvb_read("uvbeta_dense", Y, n, k, n, k, S));
  std::vector<UvbdTrait> tr(nk);
  for (size_t t = 0; t < nk; ++t) { tr[t].nt = S.nt[t]; tr[t].mu = S.mu[t]; tr[t].vy = S.vy[t]; }
  std::vector<int32_t> order(std::max<size_t>((size_t)maxit * nq, 1));
  CumulativeOrder ord(nq);
  for (int s = 0; s < maxit; ++s) {                                                                        // :1428 (cumulative, as there)
    const std::vector<int> &o = ord.next(s);
    std::copy(o.begin(), o.end(), order.begin() + (size_t)s * nq);
  }
  std::vector<double> res(nk * UVBD_NRES);
  hipStream_t st = nullptr;   // (the null stream: the holder waits for it before the vectors above go away)
  DevBufs bufs(st);
  double *Zd = bufs.get<double>(nn * nq), *yd = bufs.get<double>(nk * nn), *cols = bufs.get<double>(nk * 3 * nq), *bd = bufs.get<double>(nq * nk);
  double *resd = bufs.get<double>(nk * UVBD_NRES), *ews = pl.e_in_lds ? nullptr : bufs.get<double>(pl.ws_bytes / sizeof(double));
  uint8_t *md = bufs.get<uint8_t>(nk * nn);
  UvbdTrait *trd = bufs.get<UvbdTrait>(nk);
  int32_t *ordd = bufs.get<int32_t>(order.size());
  if (bufs.failed()) return no_memory("uvbeta_dense");
  HIPCHK(h2d(st, Zd, Zc.data(), Zc.size()));
  HIPCHK(h2d(st, yd, S.y.data(), S.y.size()));
  HIPCHK(h2d(st, md, S.obs.data(), S.obs.size()));
  HIPCHK(h2d(st, trd, tr.data(), tr.size()));
  HIPCHK(h2d(st, ordd, order.data(), order.size()));
  HIPCHK(zero(st, bd, nq * nk));                                                                           // b = 0, :1421
  UvbdArgs A;
  A.Z = Zd; A.n = n; A.q = q; A.y = yd; A.m = md; A.tr = trd; A.order = ordd; A.variant = variant; A.maxit = maxit;
  A.logtol = log10(tol); A.df0 = df0; A.thr = variant == BWGR_UVB_F ? 0.00001 : 0.0;
  A.cols = cols; A.e_ws = ews; A.b = bd; A.res = resd;
  if (pl.e_in_lds) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_uvbd_fit<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)UVBD_LDS_MAX));
    hipLaunchKernelGGL(k_uvbd_fit<true>, dim3((unsigned)k), dim3(pl.threads), pl.lds_bytes, st, A);
  } else {
    hipLaunchKernelGGL(k_uvbd_fit<false>, dim3((unsigned)k), dim3(pl.threads), pl.lds_bytes, st, A);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, b_out, bd, sizeof(double) * nq * nk));
  HIPCHK(d2h(st, res.data(), resd, sizeof(double) * nk * UVBD_NRES));
  const UvbOut out = {mu_out, h2_out, ve_out, vb_out, cnv_out, its_out};
  for (int64_t t = 0; t < k; ++t) {
    const double *rt = res.data() + (size_t)t * UVBD_NRES;
    uvb_result(out, t, S.nt[(size_t)t] == 0.0, variant, rt[0], rt[1], rt[2], S.vy[(size_t)t], rt[3], (int)rt[4]);
  }
  return BWGR_OK;
}

// out = X B on the raw int8 genotypes, every row: k_pxb over (row tiles, marker chunks, 16-trait slices), then the chunks' partials in order.
// The chunks: as many as bring the grid to about four workgroups per compute unit, at most 64 and never shorter than one staged tile of B.
static constexpr int PXB_CHUNKS_MAX = 64;     // marker chunks at most (before the chunk is rounded up to whole staged tiles of B)
static constexpr int PXB_FINISH_WG = 4096;    // workgroups of k_pxb_finish at most, 256 entries each per trip
static inline int64_t pxb_finish_grid(int64_t nk) { return std::min<int64_t>((nk + TAIL_THREADS - 1) / TAIL_THREADS, PXB_FINISH_WG); }
struct PxbPlan { int64_t tiles, slices, chunks, chunk; };
static PxbPlan pxb_plan(int64_t ld, int64_t p, int64_t k) {
  PxbPlan pl;
  pl.tiles = (ld + PXB_ROWS - 1) / PXB_ROWS; pl.slices = (k + PXB_TS - 1) / PXB_TS;
  pl.chunks = std::min<int64_t>(std::min<int64_t>(PXB_CHUNKS_MAX, (p + PXB_MT - 1) / PXB_MT), std::max<int64_t>(1, (1024 + pl.tiles * pl.slices - 1) / (pl.tiles * pl.slices)));
  pl.chunk = ((p + pl.chunks - 1) / pl.chunks + PXB_MT - 1) / PXB_MT * PXB_MT;
  pl.chunks = (p + pl.chunk - 1) / pl.chunk;
  return pl;
}
extern "C" int bwgr_panel_xb(bwgr_panel *P, const double *B, int64_t k, double *out) {
  if (!P || !B || !out) return fail(BWGR_EINVAL, "panel_xb: null pointer");
  if (k < 1 || k > 0x7FFFFFFFll) return fail(BWGR_EINVAL, "panel_xb: k = %lld columns (at least 1)", (long long)k);
  if (P->data->is_f32) return fail(BWGR_EINVAL, "panel_xb: the panel holds fp32 genotypes; panel_xb takes int8 panels only");
  HIPCHK(hipSetDevice(P->data->device));
  const int64_t n = P->data->n, p = P->data->p, ld = P->data->plan.ld;
  const int R = P->data->plan.R;
  const PxbPlan xp = pxb_plan(ld, p, k);
  const int64_t tiles = xp.tiles, slices = xp.slices, chunks = xp.chunks, chunk = xp.chunk;
  if (slices > 65535) return fail(BWGR_EINVAL, "panel_xb: k = %lld columns (at most %d per call)", (long long)k, 65535 * PXB_TS);
  hipStream_t st = P->stream;
  DevBufs bufs(st);
  const size_t nk = (size_t)n * (size_t)k;
  double *Bd = bufs.get<double>((size_t)p * (size_t)k), *part = bufs.get<double>((size_t)chunks * nk), *outd = bufs.get<double>(nk);
  if (bufs.failed()) return no_memory("panel_xb");
  HIPCHK(h2d(st, Bd, B, (size_t)p * (size_t)k));
  hipLaunchKernelGGL(k_pxb, dim3((unsigned)tiles, (unsigned)chunks, (unsigned)slices), dim3(256), 0, st, (const int8_t *)P->data->X, R, p, ld, n, (const double *)Bd, (int)k,
                     chunk, part);
  hipLaunchKernelGGL(k_pxb_finish, dim3((unsigned)pxb_finish_grid((int64_t)nk)), dim3(TAIL_THREADS), 0, st, (const double *)part, (int64_t)nk, (int)chunks, outd);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, out, outd, sizeof(double) * nk));
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// relationship kernels: the exact X X' of an int8 panel, the exact X_f X_s' between two, and their fp64 finishes (kernels.hip.h; DESIGN.md
// section 4.6)
// ------------------------------------------------------------------------------------------------
// A product's plan, decided here and nowhere else (bwgr_debug_xxt_plan and bwgr_debug_xyt_plan expose it to the CPU tests): the chunk of
// markers whose int32 sums are exact for the panels' largest |x|, the tiles -- those on and above the diagonal of X X' (sym), every tile of
// the T_r x T_c grid of X_f X_s' -- and how far a chunk is split again so that small n still fills the chip; integer sums make every split
// give the same bits.
struct XxtPlan {
  bool sym = true;                  // X X' of one panel (rows = columns); or X_f X_s' between two
  int64_t chunk = 0, nchunks = 0;   // markers per int32 chunk (the rule's, or the forced one); chunks
  int64_t Tr = 0, Tc = 0, tiles = 0;   // row and column tiles of XXT_TILE rows; tiles computed
  int64_t sub = 1, piece = 0;       // pieces per chunk; markers per piece (whole MFMA steps)
  int64_t wgs = 0;                  // workgroups launched: tiles x chunks x pieces
  bool accumulate = false;          // more than one workgroup per tile: they add into the zeroed int64 tile
  size_t ws_bytes = 0;              // device temporaries of a kernel / kernel2 call with host outputs
};
static constexpr int XXT_SUMD_PARTS = 1024;
static constexpr int XXT_ZERO_WG = 2048;      // workgroups of k_xxt_zero, 256 entries each per trip
static constexpr int KFIN_APPLY_WG = 4096;    // workgroups of k_kfin_apply / k_kfin2_apply, 256 entries each per trip
// nr, xmaxr: the rows' panel (X; the founders); nc, xmaxc: the columns' (sym: the same panel again; the samples)
static int plan_xxt(XxtPlan &pl, bool sym, int64_t nr, int64_t nc, int64_t p, int xmaxr, int xmaxc, int64_t kchunk) {
  pl = XxtPlan();
  pl.sym = sym;
  const char *who = sym ? "xxt" : "xyt", *Xr = sym ? "X" : "X_f", *Xc = sym ? "X" : "X_s";
  CHK(panel_range(nr, p));
  CHK(panel_range(nc, p));
  if (xmaxr < 0 || xmaxr > 128 || xmaxc < 0 || xmaxc > 128) return fail(BWGR_EINVAL, "%s: largest |x| = %d, %d are not int8 panels'", who, xmaxr, xmaxc);
  if (kchunk < 0) return fail(BWGR_EINVAL, "%s: forced chunk %lld < 0", who, (long long)kchunk);
  const int64_t xr = std::max(xmaxr, 1), xc = std::max(xmaxc, 1), x2 = xr * xc;
  if ((long double)x2 * (long double)p >= 9007199254740992.0L)
    return fail(BWGR_EINVAL, "%s: max|x| of %s * max|x| of %s * p = %.3Lg reaches 2^53: the entries of %s %s' would not be exact doubles", who, Xr, Xc,
                (long double)x2 * (long double)p, Xr, Xc);
  // the bounds on X s: the column sums s are the rows' panel's, applied to either panel
  if ((long double)(xr * xr) * (long double)nr * (long double)p >= 9223372036854775808.0L)
    return fail(BWGR_EINVAL, "%s: max|x|^2 * n * p of %s = %.3Lg reaches 2^63: %s s would not fit int64", who, Xr, (long double)(xr * xr) * (long double)nr * (long double)p, Xr);
  if ((long double)x2 * (long double)nr * (long double)p >= 9223372036854775808.0L)
    return fail(BWGR_EINVAL, "%s: max|x| of %s * max|x| of %s * n * p = %.3Lg reaches 2^63: %s s would not fit int64", who, Xr, Xc,
                (long double)x2 * (long double)nr * (long double)p, Xc);
  const int64_t rule = 2147483647ll / x2;
  pl.chunk = kchunk > 0 ? std::min(kchunk, rule) : rule;   // (a forced chunk beyond the rule would not be exact)
  pl.nchunks = (p + pl.chunk - 1) / pl.chunk;
  pl.Tr = (nr + XXT_TILE - 1) / XXT_TILE; pl.Tc = (nc + XXT_TILE - 1) / XXT_TILE;
  pl.tiles = sym ? pl.Tr * (pl.Tr + 1) / 2 : pl.Tr * pl.Tc;
  // pieces: about four workgroups per compute unit where the tiles and chunks alone give fewer, never shorter than sixteen steps
  const int64_t span = std::min(pl.chunk, p), steps = (span + XXT_KSTEP - 1) / XXT_KSTEP;
  const int64_t want = (1024 + pl.tiles * pl.nchunks - 1) / (pl.tiles * pl.nchunks);
  const int64_t sub0 = std::max<int64_t>(1, std::min(want, steps / 16));
  pl.piece = (steps + sub0 - 1) / sub0 * XXT_KSTEP;
  pl.sub = (span + pl.piece - 1) / pl.piece;
  if (pl.nchunks * pl.sub > 65535) return fail(BWGR_EINVAL, "%s: %lld chunks of %lld markers exceed the launch grid (65535); use a longer BWGR_KCHUNK", who, (long long)pl.nchunks, (long long)pl.chunk);
  if (pl.tiles > 0x7FFFFFFFll) return fail(BWGR_EINVAL, "%s: %lld output tiles exceed the launch grid", who, (long long)pl.tiles);
  pl.wgs = pl.tiles * pl.nchunks * pl.sub;
  pl.accumulate = pl.nchunks * pl.sub > 1;
  const int64_t ldr = (nr + 127) / 128 * 128, ldc = (nc + 127) / 128 * 128;   // (at least; a panel's own padding may be larger)
  // kernel: the n x n array; s and q; X s; the diagonal; the partial sums
  if (sym) pl.ws_bytes = (size_t)nr * nr * 8 + (size_t)p * 12 + (size_t)ldr * 8 + (size_t)nr * 8 + (size_t)(XXT_SUMD_PARTS + 1) * 8;
  // kernel2: the two 8-byte arrays; s and q; X_f s, X_s s and the samples' row sums of squares; the founders' diagonal; the partial sums;
  // the two double terms per founder and per sample of the ARC finish
  else pl.ws_bytes = (size_t)nr * nc * 8 + (size_t)nr * nr * 8 + (size_t)p * 12 + (size_t)(ldr + 2 * ldc) * 8 + (size_t)nr * 8 + (size_t)(XXT_SUMD_PARTS + 1) * 8 +
                     (size_t)(nr + nc) * 16;
  return BWGR_OK;
}
extern "C" int bwgr_debug_xxt_plan(int64_t n, int64_t p, int xmax, int64_t kchunk, int64_t out[BWGR_XXT_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "debug_xxt_plan: null pointer");
  XxtPlan pl;
  CHK(plan_xxt(pl, true, n, n, p, xmax, xmax, kchunk));
  const int64_t v[BWGR_XXT_PLAN_NOUT] = {pl.chunk, pl.nchunks, pl.tiles, pl.wgs, (int64_t)pl.ws_bytes, pl.Tr, pl.sub, pl.piece};
  std::copy(v, v + BWGR_XXT_PLAN_NOUT, out);
  return BWGR_OK;
}
extern "C" int bwgr_debug_xyt_plan(int64_t nf, int64_t ns, int64_t p, int xmaxf, int xmaxs, int64_t kchunk, int64_t out[BWGR_XYT_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "debug_xyt_plan: null pointer");
  XxtPlan pl;
  CHK(plan_xxt(pl, false, nf, ns, p, xmaxf, xmaxs, kchunk));
  const int64_t v[BWGR_XYT_PLAN_NOUT] = {pl.chunk, pl.nchunks, pl.tiles, pl.wgs, (int64_t)pl.ws_bytes, pl.Tr, pl.Tc, pl.sub, pl.piece};
  std::copy(v, v + BWGR_XYT_PLAN_NOUT, out);
  return BWGR_OK;
}

// What every entry point checks of a panel it is given; `role` names the panel in the message ("", "founders' ", "samples' ").
static int kern_accept_panel(const bwgr_panel *P, int memloc, const char *who, const char *role) {
  if (!P) return fail(BWGR_EINVAL, "%s: null pointer", who);
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "%s: bad memloc %d", who, memloc);
  if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: the %spanel holds fp32 genotypes; the relationship kernels take int8 panels only", who, role);
  return BWGR_OK;
}
// ... and the last check of a call, once its plan stands: these launches fill the chip, so nothing is enqueued while sweeps of other handles,
// whose workgroups must stay co-resident, are in flight (a pair: the partner's own work is waited for, xyt_order).  Leaves P's device set.
static int kern_accept_guard(bwgr_panel *P, const bwgr_panel *partner, const char *who) {
  HIPCHK(hipSetDevice(P->data->device));
  if (!P->data->sw.occ_guard) return BWGR_OK;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  const int busy = guard_busy(P, P->stream, partner);
  if (busy > 0) return fail(BWGR_EINVAL, "%s: sweeps of other handles hold %d compute units on this device; wait for them (bwgr_chain_sync) and call again", who, busy);
  return BWGR_OK;
}
// what the two one-panel entry points check alike.  Nothing is enqueued before it returns BWGR_OK.
static int xxt_accept(bwgr_panel *P, const void *out, int64_t ldo, int memloc, const char *who, XxtPlan &pl) {
  if (!out) return fail(BWGR_EINVAL, "%s: null pointer", who);
  CHK(kern_accept_panel(P, memloc, who, ""));
  const PanelData *D = P->data;
  if (D->n < 2) return fail(BWGR_EINVAL, "%s: n = %lld (needs 2 rows)", who, (long long)D->n);
  if (ldo < D->n) return fail(BWGR_EINVAL, "%s: leading dimension %lld < n = %lld", who, (long long)ldo, (long long)D->n);
  CHK(plan_xxt(pl, true, D->n, D->n, D->p, D->xmax, D->xmax, D->sw.kchunk));
  return kern_accept_guard(P, nullptr, who);
}
// what the two two-panel entry points check alike.  Nothing is enqueued before it returns BWGR_OK.
static int xyt_accept(bwgr_panel *Pf, bwgr_panel *Ps, int memloc, const char *who, XxtPlan &pl) {
  CHK(kern_accept_panel(Pf, memloc, who, "founders' "));
  CHK(kern_accept_panel(Ps, memloc, who, "samples' "));
  const PanelData *F = Pf->data, *S = Ps->data;
  if (F->p != S->p) return fail(BWGR_EINVAL, "%s: the founders have p = %lld markers, the samples %lld", who, (long long)F->p, (long long)S->p);
  if (F->device != S->device) return fail(BWGR_EINVAL, "%s: the founders are on device %d, the samples on device %d", who, F->device, S->device);
  CHK(plan_xxt(pl, false, F->n, S->n, F->p, F->xmax, S->xmax, F->sw.kchunk));
  return kern_accept_guard(Pf, Ps, who);
}
// the founders' stream goes on after everything pending on the samples' stream
static int xyt_order(bwgr_panel *Pf, bwgr_panel *Ps, DevBufs &bufs, const char *who) {
  if (Ps->stream == Pf->stream) return BWGR_OK;
  hipEvent_t ev = bufs.event(hipEventDisableTiming);
  if (!ev) return fail(BWGR_EHIP, "%s: hipEventCreate failed", who);
  HIPCHK(hipEventRecord(ev, Ps->stream));
  HIPCHK(hipStreamWaitEvent(Pf->stream, ev, 0));
  return BWGR_OK;
}
// The planned product into the device array Gd (int64, row stride ldg), enqueued on Pr's stream: G = X X' over Pr's n rows, both triangles
// (pl.sym; Pc = Pr), or G = X_f X_s' (n_f x n_s) between the founders Pr and the samples Pc.
static int xxt_product(bwgr_panel *Pr, bwgr_panel *Pc, const XxtPlan &pl, long long *Gd, int64_t ldg) {
  const PanelData *A = Pr->data, *B = Pc->data;
  hipStream_t st = Pr->stream;
  XxtArgs a;
  a.XA = (const int8_t *)A->X; a.XB = (const int8_t *)B->X; a.p = A->p; a.RA = A->plan.R; a.RB = B->plan.R; a.nA = (int)A->n; a.nB = (int)B->n;
  a.T = (int)(pl.sym ? pl.Tr : pl.Tc); a.chunk = pl.chunk; a.piece = pl.piece; a.sub = (int)pl.sub; a.accumulate = pl.accumulate ? 1 : 0; a.G = Gd; a.ldg = ldg;
  const dim3 grid((unsigned)pl.tiles, (unsigned)(pl.nchunks * pl.sub));
  if (pl.accumulate) hipLaunchKernelGGL(k_xxt_zero, dim3(XXT_ZERO_WG), dim3(TAIL_THREADS), 0, st, Gd, ldg, a.nA, a.nB, pl.sym ? 1 : 0);
  if (pl.sym) {
    hipLaunchKernelGGL(k_xxt_mfma_i8, grid, dim3(256), 0, st, a);
    const unsigned t32 = (unsigned)((A->n + 31) / 32);
    hipLaunchKernelGGL(k_xxt_mirror, dim3(t32, t32), dim3(32, 8), 0, st, Gd, ldg, a.nA);
  } else {
    hipLaunchKernelGGL(k_xyt_mfma_i8, grid, dim3(256), 0, st, a);
  }
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}
// an nr x nc 8-byte result to the caller's host array
static int kern_to_host(hipStream_t st, void *dst, int64_t ldo, const void *src, int64_t nr, int64_t nc) {
  HIPCHK(hipMemcpy2DAsync(dst, (size_t)ldo * 8, src, (size_t)nc * 8, (size_t)nc * 8, (size_t)nr, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}
// the grid of k_kfin_xs / k_kfin2_rowsq over a panel of ld padded rows: 128 rows per workgroup, the markers split so that the launch fills the chip
static inline dim3 kfin_rows_grid(int64_t ld, int64_t p, int64_t *cpw) {
  const int64_t ysplit = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(65535, (p + 511) / 512), 2048 / (ld / 128) + 1));
  *cpw = (p + ysplit - 1) / ysplit;
  return dim3((unsigned)(ld / 128), (unsigned)((p + *cpw - 1) / *cpw));
}
// c = sum_j (s_j / n)^2 on the host, in marker order from the exact column sums
static double kfin_mean_sq(const std::vector<int32_t> &s, double ninv) {
  double c = 0.0;
  for (size_t j = 0; j < s.size(); ++j) { const double m = (double)s[j] * ninv; c += m * m; }
  return c;
}
// EigenGAU's and EigenGauZ's t = phi (-n (n - 1)) / sum_{i != j} sqrt(G_ii + G_jj - 2 G_ij) (RcppEigen20230423.cpp:37, :1929): the fixed-grid,
// fixed-tree sum over the n x n product G (part: XXT_SUMD_PARTS + 1 doubles), and n (n - 1) formed in double (the reference's int product
// overflows beyond 46 340 rows)
static int kfin_gau_t(hipStream_t st, const long long *G, int64_t ldg, const long long *diag_d, int64_t n, double par, double *part, double *t) {
  double sumd = 0.0;
  hipLaunchKernelGGL(k_kfin_sumd_stage1, dim3(XXT_SUMD_PARTS), dim3(256), 0, st, G, ldg, diag_d, (int)n, part);
  hipLaunchKernelGGL(k_kfin_sumd_stage2, dim3(1), dim3(256), 0, st, part, XXT_SUMD_PARTS, part + XXT_SUMD_PARTS);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(st, &sumd, part + XXT_SUMD_PARTS, sizeof(double)));
  const double nd = (double)n;
  *t = par * (-(nd * (nd - 1.0))) / sumd;
  return BWGR_OK;
}

extern "C" int bwgr_panel_crossprod(bwgr_panel *P, int64_t *G, int64_t ldg, int memloc) {
  XxtPlan pl;
  CHK(xxt_accept(P, G, ldg, memloc, "panel_crossprod", pl));
  const int64_t n = P->data->n;
  DevBufs bufs(P->stream);
  long long *Gd = reinterpret_cast<long long *>(G); int64_t ldd = ldg;
  if (memloc == BWGR_HOST) {
    Gd = bufs.get<long long>((size_t)n * n); ldd = n;
    if (bufs.failed()) return no_memory("panel_crossprod");
  }
  CHK(xxt_product(P, P, pl, Gd, ldd));
  if (memloc == BWGR_HOST) return kern_to_host(P->stream, G, ldg, Gd, n, n);
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

extern "C" int bwgr_panel_kernel(bwgr_panel *P, int kind, double par, int flag, double *K, int64_t ldk, int memloc) {
  if (kind < BWGR_K_GRM || kind > BWGR_K_EIGEN_ARC) return fail(BWGR_EINVAL, "panel_kernel: unknown kind %d", kind);
  XxtPlan pl;
  CHK(xxt_accept(P, K, ldk, memloc, "panel_kernel", pl));
  const PanelData *D = P->data;
  const int64_t n = D->n, p = D->p, ld = D->plan.ld;
  hipStream_t st = P->stream;
  // which inputs the kind needs: the centred product (GRM; EigenGRM / EigenARC with their flag), the column sums (those, and GAU's mean)
  const bool cen = kind == BWGR_K_GRM || ((kind == BWGR_K_EIGEN_GRM || kind == BWGR_K_EIGEN_ARC) && flag != 0);
  const bool cols = cen || kind == BWGR_K_GAU;
  std::vector<long long> diag((size_t)n), rs, q;
  std::vector<int32_t> s;
  DevBufs bufs(st);
  long long *Gd = reinterpret_cast<long long *>(K); int64_t ldd = ldk;
  if (memloc == BWGR_HOST) { Gd = bufs.get<long long>((size_t)n * n); ldd = n; }
  long long *diag_d = bufs.get<long long>((size_t)n), *rs_d = cen ? bufs.get<long long>((size_t)ld) : nullptr, *q_d = cols ? bufs.get<long long>((size_t)p) : nullptr;
  int32_t *s_d = cols ? bufs.get<int32_t>((size_t)p) : nullptr;
  double *part = kind == BWGR_K_EIGEN_GAU ? bufs.get<double>(XXT_SUMD_PARTS + 1) : nullptr;
  if (bufs.failed()) return no_memory("panel_kernel");
  CHK(xxt_product(P, P, pl, Gd, ldd));
  hipLaunchKernelGGL(k_kfin_diag, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Gd, ldd, (int)n, diag_d);
  if (cols) hipLaunchKernelGGL(k_kfin_colstats, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, (int)n, p, s_d, q_d);
  if (cen) {
    HIPCHK(zero(st, rs_d, (size_t)ld));
    int64_t cpw = 0;
    const dim3 g = kfin_rows_grid(ld, p, &cpw);
    hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, p, s_d, cpw, rs_d);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(diag.data(), diag_d, sizeof(long long) * n, hipMemcpyDeviceToHost, st));
  if (cols) { s.resize((size_t)p); q.resize((size_t)p); HIPCHK(hipMemcpyAsync(s.data(), s_d, sizeof(int32_t) * p, hipMemcpyDeviceToHost, st)); HIPCHK(hipMemcpyAsync(q.data(), q_d, sizeof(long long) * p, hipMemcpyDeviceToHost, st)); }
  if (cen) { rs.resize((size_t)n); HIPCHK(hipMemcpyAsync(rs.data(), rs_d, sizeof(long long) * n, hipMemcpyDeviceToHost, st)); }
  HIPCHK(hipStreamSynchronize(st));
  // ---- the global scalars, on the host in a fixed order from the exact integers ----
  const double nd = (double)n, ninv = 1.0 / nd;
  const double c = kfin_mean_sq(s, ninv);   // sum_j mean_j^2 (s is empty where the kind needs no column sums)
  double sumvar = 0.0;               // sum_j fvar(x_j) = sum_j (q_j - s_j^2 / n) / (n - 1)
  __int128 ss = 0, tr = 0;           // sum_j s_j^2 = the sum of all entries of G; its trace
  for (int64_t j = 0; j < (cols ? p : 0); ++j) {
    sumvar += ((double)q[j] - (double)s[j] * (double)s[j] / nd) / (nd - 1.0);
    ss += (__int128)s[j] * s[j];
  }
  for (int64_t i = 0; i < n; ++i) tr += diag[i];
  const auto zz_diag = [&](int64_t i) { double v = (double)diag[i]; if (cen) v = v - ((double)rs[i] * ninv + (double)rs[i] * ninv) + c; return v; };
  KfinArgs a;
  a.G = Gd; a.ldg = ldd; a.n = (int)n; a.kind = kind; a.cen = cen ? 1 : 0; a.diag = diag_d; a.rs = rs_d; a.ninv = ninv; a.c = c; a.scale = 1.0;
  switch (kind) {
    case BWGR_K_GRM: a.scale = flag ? c / 2.0 : sumvar; break;                                          // Sum2pq, :1369-1373
    case BWGR_K_GAU: a.scale = (double)(2 * ((__int128)n * tr - ss)) / (nd * (nd - 1.0)); break;        // md, :1351-1353
    case BWGR_K_EIGEN_GRM: case BWGR_K_EIGEN_ARC: {
      double sd = 0.0;
      for (int64_t i = 0; i < n; ++i) sd += zz_diag(i) + (kind == BWGR_K_EIGEN_GRM ? 1.0 : 0.0);
      a.scale = 1.0 / (sd / nd);                                                                        // tmp, RcppEigen20230423.cpp:18, :50
    } break;
    default: CHK(kfin_gau_t(st, Gd, ldd, diag_d, n, par, part, &a.scale));                              // EigenGAU's tmp, :37
  }
  hipLaunchKernelGGL(k_kfin_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  HIPCHK(hipGetLastError());
  if (memloc == BWGR_HOST) return kern_to_host(st, K, ldk, Gd, n, n);
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// founder-by-sample kernels: the two entries on a pair of int8 panels, EigenArcZ's / EigenGauZ's K_ff and K_fs (kernels.hip.h; DESIGN.md
// section 4.6)
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_panel_crossprod2(bwgr_panel *Pf, bwgr_panel *Ps, int64_t *G, int64_t ldg, int memloc) {
  if (!G) return fail(BWGR_EINVAL, "panel_crossprod2: null pointer");
  if (Pf && Ps && ldg < Ps->data->n) return fail(BWGR_EINVAL, "panel_crossprod2: leading dimension %lld < n_s = %lld", (long long)ldg, (long long)Ps->data->n);
  XxtPlan pl;
  CHK(xyt_accept(Pf, Ps, memloc, "panel_crossprod2", pl));
  const int64_t nf = Pf->data->n, ns = Ps->data->n;
  DevBufs bufs(Pf->stream);
  long long *Gd = reinterpret_cast<long long *>(G); int64_t ldd = ldg;
  if (memloc == BWGR_HOST) {
    Gd = bufs.get<long long>((size_t)nf * ns); ldd = ns;
    if (bufs.failed()) return no_memory("panel_crossprod2");
  }
  CHK(xyt_order(Pf, Ps, bufs, "panel_crossprod2"));
  CHK(xxt_product(Pf, Ps, pl, Gd, ldd));
  if (memloc == BWGR_HOST) return kern_to_host(Pf->stream, G, ldg, Gd, nf, ns);
  HIPCHK(hipStreamSynchronize(Pf->stream));
  return BWGR_OK;
}

extern "C" int bwgr_panel_kernel2(bwgr_panel *Pf, bwgr_panel *Ps, int kind, double par, double *Kff, int64_t ldff, double *Kfs, int64_t ldfs, int memloc) {
  if (kind != BWGR_KZ_ARC && kind != BWGR_KZ_GAU) return fail(BWGR_EINVAL, "panel_kernel2: unknown kind %d", kind);
  if (!Kff || !Kfs) return fail(BWGR_EINVAL, "panel_kernel2: null pointer");
  if (Pf && Ps && ldff < Pf->data->n) return fail(BWGR_EINVAL, "panel_kernel2: leading dimension %lld of Kff < n_f = %lld", (long long)ldff, (long long)Pf->data->n);
  if (Pf && Ps && ldfs < Ps->data->n) return fail(BWGR_EINVAL, "panel_kernel2: leading dimension %lld of Kfs < n_s = %lld", (long long)ldfs, (long long)Ps->data->n);
  XxtPlan pl;
  CHK(xyt_accept(Pf, Ps, memloc, "panel_kernel2", pl));
  const PanelData *F = Pf->data, *S = Ps->data;
  XxtPlan plf;      // K_ff's product is the symmetric one
  CHK(plan_xxt(plf, true, F->n, F->n, F->p, F->xmax, F->xmax, F->sw.kchunk));
  const int64_t nf = F->n, ns = S->n, p = F->p, ldf = F->plan.ld, lds = S->plan.ld;
  const bool arc = kind == BWGR_KZ_ARC;
  hipStream_t st = Pf->stream;
  std::vector<long long> diag((size_t)nf), qs, rf, rs;
  std::vector<int32_t> s;
  std::vector<double> h_r, h_d;     // ARC: r_f | r_s; d_f | d_s
  DevBufs bufs(st);
  long long *Gff = reinterpret_cast<long long *>(Kff), *Gfs = reinterpret_cast<long long *>(Kfs); int64_t ldd_ff = ldff, ldd_fs = ldfs;
  if (memloc == BWGR_HOST) { Gff = bufs.get<long long>((size_t)nf * nf); ldd_ff = nf; Gfs = bufs.get<long long>((size_t)nf * ns); ldd_fs = ns; }
  long long *diag_d = bufs.get<long long>((size_t)nf), *qs_d = bufs.get<long long>((size_t)lds);
  long long *rf_d = arc ? bufs.get<long long>((size_t)ldf) : nullptr, *rs_d = arc ? bufs.get<long long>((size_t)lds) : nullptr, *q_d = arc ? bufs.get<long long>((size_t)p) : nullptr;
  int32_t *s_d = arc ? bufs.get<int32_t>((size_t)p) : nullptr;
  double *r_d = arc ? bufs.get<double>((size_t)(nf + ns)) : nullptr, *d_d = arc ? bufs.get<double>((size_t)(nf + ns)) : nullptr;
  double *part = arc ? nullptr : bufs.get<double>(XXT_SUMD_PARTS + 1);
  if (bufs.failed()) return no_memory("panel_kernel2");
  CHK(xyt_order(Pf, Ps, bufs, "panel_kernel2"));
  CHK(xxt_product(Pf, Pf, plf, Gff, ldd_ff));
  CHK(xxt_product(Pf, Ps, pl, Gfs, ldd_fs));
  hipLaunchKernelGGL(k_kfin_diag, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, Gff, ldd_ff, (int)nf, diag_d);
  int64_t cpw = 0;
  HIPCHK(zero(st, qs_d, (size_t)lds));
  { const dim3 g = kfin_rows_grid(lds, p, &cpw); hipLaunchKernelGGL(k_kfin2_rowsq, g, dim3(256), 0, st, (const int8_t *)S->X, S->plan.R, p, cpw, qs_d); }
  if (arc) {
    hipLaunchKernelGGL(k_kfin_colstats, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, st, (const int8_t *)F->X, F->plan.R, (int)nf, p, s_d, q_d);
    HIPCHK(zero(st, rf_d, (size_t)ldf)); HIPCHK(zero(st, rs_d, (size_t)lds));
    { const dim3 g = kfin_rows_grid(ldf, p, &cpw); hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)F->X, F->plan.R, p, s_d, cpw, rf_d); }
    { const dim3 g = kfin_rows_grid(lds, p, &cpw); hipLaunchKernelGGL(k_kfin_xs, g, dim3(256), 0, st, (const int8_t *)S->X, S->plan.R, p, s_d, cpw, rs_d); }
  }
  HIPCHK(hipGetLastError());
  Kfin2Args a;
  a.kind = arc ? KFIN2_ARC : KFIN2_GAU; a.irow = diag_d; a.icol = diag_d; a.rrow = a.rcol = a.drow = a.dcol = nullptr; a.c = 0.0; a.scale = 1.0;
  const double nd = (double)nf, ninv = 1.0 / nd;
  if (arc) {
    qs.resize((size_t)ns); rf.resize((size_t)nf); rs.resize((size_t)ns); s.resize((size_t)p);
    HIPCHK(hipMemcpyAsync(diag.data(), diag_d, sizeof(long long) * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(qs.data(), qs_d, sizeof(long long) * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rf.data(), rf_d, sizeof(long long) * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rs.data(), rs_d, sizeof(long long) * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s.data(), s_d, sizeof(int32_t) * p, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- the global scalars and the per-row terms, on the host in a fixed order from the exact integers ----
    const double c = kfin_mean_sq(s, ninv);
    h_r.resize((size_t)(nf + ns)); h_d.resize((size_t)(nf + ns));
    for (int64_t i = 0; i < nf; ++i) { const double r = (double)rf[i] * ninv; h_r[i] = r; h_d[i] = (double)diag[i] - (r + r) + c; }
    for (int64_t j = 0; j < ns; ++j) { const double r = (double)rs[j] * ninv; h_r[nf + j] = r; h_d[nf + j] = (double)qs[j] - (r + r) + c; }
    double sd = 0.0;                   // the finished diagonal of K_ff before Kscalar: it depends on d_f alone
    for (int64_t i = 0; i < nf; ++i) sd += kfin2_arc(h_d[i], h_d[i], h_d[i]);
    a.c = c; a.scale = 1.0 / (sd / nd);                                                                 // Kscalar, RcppEigen20230423.cpp:1896
    HIPCHK(h2d(st, r_d, h_r.data(), (size_t)(nf + ns))); HIPCHK(h2d(st, d_d, h_d.data(), (size_t)(nf + ns)));
    a.rrow = r_d; a.drow = d_d;
  } else {
    CHK(kfin_gau_t(st, Gff, ldd_ff, diag_d, nf, par, part, &a.scale));                                  // tmp, :1929
  }
  // K_ff, then K_fs (both read the founders' diagonal, which K_ff's finish overwrites only in G: diag_d is the copy)
  a.G = Gff; a.ldg = ldd_ff; a.nr = (int)nf; a.nc = (int)nf; a.same = 1;
  if (arc) { a.rcol = r_d; a.dcol = d_d; }
  hipLaunchKernelGGL(k_kfin2_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  a.G = Gfs; a.ldg = ldd_fs; a.nc = (int)ns; a.same = 0; a.icol = qs_d;
  if (arc) { a.rcol = r_d + nf; a.dcol = d_d + nf; }
  hipLaunchKernelGGL(k_kfin2_apply, dim3(KFIN_APPLY_WG), dim3(TAIL_THREADS), 0, st, a);
  HIPCHK(hipGetLastError());
  if (memloc == BWGR_HOST) { CHK(kern_to_host(st, Kff, ldff, Gff, nf, nf)); return kern_to_host(st, Kfs, ldfs, Gfs, nf, ns); }
  HIPCHK(hipStreamSynchronize(st));
  return BWGR_OK;
}
