// bwgr_amd/csrc/pegsx_host.hip.h -- the host entry of PEGSX (src/RcppEigenX20251203.cpp:197-573): PEGSZ's effects with a
// fixed design X beside them.  Part of bwgr_hip.hip, after pegs_host.hip.h.  It holds the fit's own algebra: the option checks, the fixed design
// (pegsx_setup.h), TrZSZ, the fixed step, the per-sweep tail (pegs_tail.h), the timing hooks and the outputs; the effect checks, the device arrays
// and every repeated step are MtFit's (mtfit_host.hip.h).  It defines no kernel.
//   once:       host (pegsx_setup.h): masks, patterns, per pattern (M'M)^+, b, the projected y.  Per effect k_mrr_setup_cols (uncentred) or
//               k_pegs_dense_setup or k_pegs_sparse_setup -> ZZ, tilde; k_mrr_tilde(mode 2) on ZZ; k_pegsx_trace_panel / _dense / _sparse ->
//               k_mrr_finish -> TrZSZ
//   per sweep:  per effect in list order: mrr_sweep (panel), k_mrr_linv -> k_pegs_dense_leg (dense) or the sparse legs; k_pegsx_fixed; k_mrr_ey ->
//               k_mrr_tilde(mode 0) per effect -> (host, pegs_tail.h: vb with its prior, NNC, XFA, bending, pinv, ve, cnv)
//   at the end: hat = X b (k_pegs_zb) plus every effect's share as in bwgr_pegs; there is no mu
// ------------------------------------------------------------------------------------------------
// The plan of the fixed step and of the trace kernels, decided here and nowhere else (bwgr_debug_pegsx_plan exposes it to the CPU tests)
struct PegsxPlan { int threads; size_t lds_fixed, ws_bytes; int jc, fc; size_t lds_trace; };
static PegsxPlan pegsx_plan(int64_t n, int f, int k) {
  PegsxPlan pl;
  pl.threads = (int)std::min<int64_t>(PEGSX_TMAX, (n + 63) / 64 * 64);   // one row per thread up to 1024 rows, whole waves
  pl.lds_fixed = pegsx_fixed_lds(f);
  pl.ws_bytes = sizeof(double) * ((size_t)n * f + (size_t)k * f * f + (size_t)f * k);   // X, (M'M)^+ of up to k patterns, b
  pl.jc = PEGSX_JC; pl.fc = PEGSX_FC;
  pl.lds_trace = pegsx_trace_lds(f);
  return pl;
}
static inline int64_t pegsx_trace_grid(int64_t m) { return std::min<int64_t>(((m + PEGSX_JC - 1) / PEGSX_JC + 3) / 4, PEGSX_TRACE_WG); }
extern "C" int bwgr_debug_pegsx_plan(int64_t n, int f, int k, int64_t out[BWGR_PEGSX_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "pegsx plan: null pointer");
  if (n < 1 || f < 1 || f > BWGR_PEGSX_MAXF || k < 1 || k > BWGR_MRR_MAXK)
    return fail(BWGR_EINVAL, "pegsx plan: n = %lld (at least 1), f = %d (1 <= f <= %d), k = %d (1 <= k <= %d)", (long long)n, f, BWGR_PEGSX_MAXF, k, BWGR_MRR_MAXK);
  const PegsxPlan pl = pegsx_plan(n, f, k);
  out[0] = pl.threads; out[1] = (int64_t)pl.lds_fixed; out[2] = (int64_t)pl.ws_bytes; out[3] = pl.jc; out[4] = pl.fc; out[5] = (int64_t)pl.lds_trace;
  return BWGR_OK;
}

// The grids and workgroup sizes bwgr_pegs and bwgr_pegsx launch for n rows and an effect of m columns, from the functions the launch sites call
extern "C" int bwgr_debug_pegs_launch_plan(int64_t n, int64_t m, int64_t out[BWGR_PEGS_LAUNCH_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "pegs launch plan: null pointer");
  if (n < 1 || m < 1) return fail(BWGR_EINVAL, "pegs launch plan: n = %lld, m = %lld (each at least 1)", (long long)n, (long long)m);
  const int64_t tg = pegsx_trace_grid(m), sg = pegs_dense_setup_grid(m);
  out[0] = tg; out[1] = tg * 4 * PEGSX_JC;                       // (the trace kernels run four waves, PEGSX_JC columns each)
  out[2] = sg; out[3] = sg * (TAIL_THREADS / 64);
  out[4] = pegs_dense_plan(n, 1, 1).threads; out[5] = pegsx_plan(n, 1, 1).threads;
  return BWGR_OK;
}

// Timing for tools/pegsx_probe.py, off unless asked for: mode 1 times the set-up kernels with events (outside the sweeps) and every sweep with
// the host clock (a sweep ends in a synchronous copy, so the clock adds no synchronisation); mode 2 also brackets k_pegsx_fixed with events.
static int g_pegsx_timing = 0;
static double g_pegsx_last[BWGR_PEGSX_TIMING_NOUT];
extern "C" int bwgr_debug_pegsx_timing(int mode, double out[BWGR_PEGSX_TIMING_NOUT]) {
  if (mode < 0 || mode > 2) return fail(BWGR_EINVAL, "pegsx timing: mode %d (0: off, 1: set-up and sweeps, 2: and the fixed step)", mode);
  g_pegsx_timing = mode;
  if (out) for (int i = 0; i < BWGR_PEGSX_TIMING_NOUT; ++i) out[i] = g_pegsx_last[i];
  return BWGR_OK;
}
struct PegsxStats {
  double sum = 0.0, mn = 0.0, mx = 0.0; int cnt = 0;
  void add(double v) { mn = cnt ? std::min(mn, v) : v; mx = cnt ? std::max(mx, v) : v; sum += v; ++cnt; }
  void put(double *o) const { o[0] = cnt ? sum / cnt : 0.0; o[1] = mn; o[2] = mx; }
};

extern "C" int bwgr_pegsx_ex(int device, const bwgr_pegs_effect_ex *eff, int neff, const double *X, int64_t ldx, int f, const double *Y, int64_t n, int k, int maxit,
                             double logtol, double covbend, double covMinEv, double df0, int NNC, int XFA, int NumXFA, int InnerGS, int NoInv, double *Tr_out,
                             double *bfix_out, double *const *u_out, double *const *vb_out, double *const *GC_out, double *ve_out, double *hat_out, int *numit_out,
                             double *cnv_out, double *bend_out) {
  static_assert(PEGSX_MAXF == BWGR_PEGSX_MAXF, "the kernels' cap is the header's");
  if (neff < 1) return fail(BWGR_EINVAL, "pegsx: Z_list holds %d effects (at least 1)", neff);
  if (f < 1 || f > BWGR_PEGSX_MAXF) return fail(BWGR_EINVAL, "pegsx: f = %d columns of X; this engine takes 1 <= f <= %d", f, BWGR_PEGSX_MAXF);
  if (!eff || !X || !Y || !u_out || !numit_out) return fail(BWGR_EINVAL, "pegsx: null pointer");
  if (InnerGS) return fail(BWGR_EINVAL, "pegsx: InnerGS is refused: every column is the k x k block solve (LLT in the reference), which has no inner Gauss-Seidel here");
  if (NoInv) return fail(BWGR_EINVAL, "pegsx: NoInv is refused: the block solve works on iG + diag(ZZ / ve), as mrr's does");
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "pegsx: k = %d traits; this engine takes 1 <= k <= %d", k, BWGR_MRR_MAXK);
  if (n < 1) return fail(BWGR_EINVAL, "pegsx: n = %lld rows (at least 1)", (long long)n);
  if (ldx < n) return fail(BWGR_EINVAL, "pegsx: ldx = %lld is below n = %lld", (long long)ldx, (long long)n);
  const PegsxOpts o = {maxit, logtol, covbend, covMinEv, df0, NNC != 0, XFA != 0, NumXFA};
  if (const char *why = pegsx_refuses(o))
    return fail(BWGR_EINVAL, "pegsx: %s (maxit = %d, logtol = %g, covbend = %g, covMinEv = %g, df0 = %g)", why, maxit, logtol, covbend, covMinEv, df0);
  MtList E;                                      // (before the fixed set, which needs its ld, and the fit, whose holder waits for the stream)
  CHK(mt_check_effects("pegsx", "u", eff, neff, n, device, u_out, E));
  const int64_t ld = E.ld;
  // ---- host set-up (:227-260): masks, patterns, (M'M)^+ per pattern, b, the projected y ----
  const FixedSet F = read_fixed(Y, X, n, k, f, ldx, ld);
  if (F.bad_row >= 0) return fail(BWGR_EINVAL, "pegsx: X[%lld, %lld] is not finite", (long long)F.bad_row, (long long)F.bad_col);
  const TraitSet &S = F.S;
  if (S.bad >= 0) return fail(BWGR_EINVAL, "pegsx: trait %d has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns &pat = F.pat;
  std::vector<double> bfk((size_t)f * k);                                                          // b as the kernels hold it: [f][k]
  for (int t = 0; t < k; ++t) for (int c = 0; c < f; ++c) bfk[(size_t)c * k + t] = F.b[(size_t)t * f + c];
  PegsxState T;                                  // (its iG is copied from asynchronously: before the fit, as bfk is)
  MtFit M(E, k);
  M.masks(S, pat);
  M.alloc(hat_out != nullptr, true);
  hipStream_t st = M.st;
  DevBufs &bufs = M.bufs;
  const int npat = M.npat;
  const size_t nn = (size_t)n, nf = (size_t)f;
  int64_t mmax = 1;
  for (const MtEffect &Q : M.eff) mmax = std::max(mmax, Q.m);
  double *Xd = bufs.get<double>(nn * nf), *iXXd = bufs.get<double>((size_t)npat * nf * nf), *bfd = bufs.get<double>(nf * k);
  double *qpart = bufs.get<double>((size_t)pegsx_trace_grid(mmax) * npat);
  const int timing = g_pegsx_timing;
  hipEvent_t ev0 = timing ? bufs.event(hipEventDefault) : hipEvent_t{}, ev1 = timing ? bufs.event(hipEventDefault) : hipEvent_t{};
  if (bufs.failed() || (timing && (!ev0 || !ev1))) return no_memory("pegsx");
  double ms_cols = 0.0, ms_trace = 0.0;
  PegsxStats ms_sweep, ms_fixed;
  auto lap = [&](double &acc) -> hipError_t {       // adds the time between ev0 and now to acc
    hipError_t e_ = hipEventRecord(ev1, st);
    if (e_ == hipSuccess) e_ = hipEventSynchronize(ev1);
    float ms = 0.f;
    if (e_ == hipSuccess) e_ = hipEventElapsedTime(&ms, ev0, ev1);
    acc += ms;
    return e_;
  };
  CHK(M.upload(S, nullptr));                                                                       // e = y, :367; no sums of y: nothing is centred
  HIPCHK(zero(st, M.small, MtFit::SMALL_LEN));
  HIPCHK(h2d(st, Xd, F.X.data(), nn * nf));
  HIPCHK(h2d(st, iXXd, F.iXX.data(), (size_t)npat * nf * nf));
  HIPCHK(h2d(st, bfd, bfk.data(), nf * k));
  const PegsxPlan xpl = pegsx_plan(n, f, k);
  // ---- per effect: ZZ and tilde of the raw columns (:277-290, :325-330), u = 0, TrZSZ (:292-323) ----
  std::vector<double> Tr((size_t)neff * k), szz(k), quad(npat);
  for (int e = 0; e < neff; ++e) {
    const MtEffect &Q = M.eff[(size_t)e];
    const unsigned tg = (unsigned)pegsx_trace_grid(Q.m);
    CHK(M.stage_effect(e));
    if (timing) HIPCHK(hipEventRecord(ev0, st));
    CHK(M.setup_effect(e, 0));
    if (timing) HIPCHK(lap(ms_cols));
    CHK(M.reduce(Q.b(), Q.tilde(), Q.XX(), Q.m, 2, k, nullptr, szz.data()));
    if (timing) HIPCHK(hipEventRecord(ev0, st));
    if (Q.panel) {
      const PanelData *D = Q.leg.P->data;
      hipLaunchKernelGGL(k_pegsx_trace_panel, dim3(tg), dim3(256), xpl.lds_trace, st, (const int8_t *)D->X, D->plan.R, Q.m, ld, (const double *)Xd, n, f,
                         (const uint32_t *)M.zbd, npat, (const double *)iXXd, qpart);
    } else if (Q.sparse) {
      hipLaunchKernelGGL(k_pegsx_trace_sparse, dim3(tg), dim3(256), xpl.lds_trace, st, (const int64_t *)Q.sp.colptr, (const int32_t *)Q.sp.rowidx,
                         (const double *)Q.sp.val, Q.m, (const double *)Xd, n, f, (const uint32_t *)M.zbd, npat, (const double *)iXXd, qpart);
    } else {
      hipLaunchKernelGGL(k_pegsx_trace_dense, dim3(tg), dim3(256), xpl.lds_trace, st, (const double *)Q.dense.Zd, Q.m, ld, (const double *)Xd, n, f,
                         (const uint32_t *)M.zbd, npat, (const double *)iXXd, qpart);
    }
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(lap(ms_trace));
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)qpart, (int)tg, npat, M.small);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, quad.data(), M.small, sizeof(double) * npat));
    for (int t = 0; t < k; ++t) Tr[(size_t)e * k + t] = szz[(size_t)t] - quad[(size_t)pat.id[(size_t)t]];
  }
  pegsx_init(T, k, neff, f, o, S.nt.data(), F.ssy.data(), Tr.data(), nullptr);
  // ---- sweeps ----
  PegsxFixedArgs FA;
  FA.X = Xd; FA.n = n; FA.ld = ld; FA.f = f; FA.zt = M.ztd; FA.e = M.ed; FA.iXX = iXXd; FA.b = bfd;
  std::vector<double> ey(2 * (size_t)k), TH((size_t)neff * k * k), db2((size_t)neff);
  while (T.numit < maxit) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < k; ++t) M.mc.iVe[t] = 1.0 / T.ve[(size_t)t];
    for (int e = 0; e < neff; ++e) CHK(M.sweep_effect(e, T.numit, T.eff[(size_t)e].iG.data()));
    if (timing == 2) HIPCHK(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(k_pegsx_fixed, dim3(k), dim3(xpl.threads), xpl.lds_fixed, st, FA, M.mc);                                        // :502-509
    if (timing == 2) { double ms = 0.0; HIPCHK(lap(ms)); ms_fixed.add(ms); }
    CHK(M.residual_sums(ey.data()));
    for (int e = 0; e < neff; ++e) CHK(M.effect_sums(e, TH.data() + (size_t)e * k * k, &db2[(size_t)e]));
    const bool stop = pegsx_after_sweep(T, o, ey.data(), TH.data(), db2.data(), nullptr);
    if (cnv_out) cnv_out[T.numit - 1] = T.cnv;
    if (timing) ms_sweep.add(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (stop) break;
  }
  if (timing) {
    g_pegsx_last[0] = ms_trace; g_pegsx_last[1] = ms_cols; g_pegsx_last[2] = ms_sweep.cnt;
    ms_sweep.put(g_pegsx_last + 3); ms_fixed.put(g_pegsx_last + 6);
  }
  if (cnv_out && T.numit == 0) cnv_out[0] = T.cnv;
  // ---- results: b, u, the fitted values of every row (:536-540), vb and GC ----
  HIPCHK(d2h(st, bfk.data(), bfd, sizeof(double) * nf * k));
  if (bfix_out) for (int t = 0; t < k; ++t) for (int c = 0; c < f; ++c) bfix_out[(size_t)t * f + c] = bfk[(size_t)c * k + t];   // f x k column-major
  if (hat_out) {
    HIPCHK(zero(st, M.hatd, nn * k));
    hipLaunchKernelGGL(k_pegs_zb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)Xd, n, (int64_t)f, k, (const double *)bfd, M.hatd);
    HIPCHK(hipGetLastError());
  }
  for (int e = 0; e < neff; ++e) {
    CHK(M.read_b(e, u_out[e]));
    if (hat_out) CHK(M.add_effect_hat(e));                                                         // (the staged offset is zero: `small` was zeroed and nothing wrote it)
  }
  if (hat_out) HIPCHK(d2h(st, hat_out, M.hatd, sizeof(double) * nn * k));
  std::vector<double> GC((size_t)neff * k * k);
  pegsx_finish(T, GC.data());
  for (int t = 0; t < k; ++t) if (ve_out) ve_out[t] = T.ve[(size_t)t];
  for (int e = 0; e < neff; ++e) {
    if (bend_out) bend_out[e] = T.eff[(size_t)e].inflate;
    for (int t = 0; t < k; ++t) if (Tr_out) Tr_out[(size_t)e * k + t] = Tr[(size_t)e * k + t];
    for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) {                                       // column-major (symmetric)
      if (vb_out && vb_out[e]) vb_out[e][j * k + i] = T.eff[(size_t)e].vb[(size_t)i * k + j];
      if (GC_out && GC_out[e]) GC_out[e][j * k + i] = GC[(size_t)e * k * k + i * k + j];
    }
  }
  *numit_out = T.numit;
  return BWGR_OK;
}
extern "C" int bwgr_pegsx(int device, const bwgr_pegs_effect *eff, int neff, const double *X, int64_t ldx, int f, const double *Y, int64_t n, int k, int maxit,
                          double logtol, double covbend, double covMinEv, double df0, int NNC, int XFA, int NumXFA, int InnerGS, int NoInv, double *Tr_out,
                          double *bfix_out, double *const *u_out, double *const *vb_out, double *const *GC_out, double *ve_out, double *hat_out, int *numit_out,
                          double *cnv_out, double *bend_out) {
  const std::vector<bwgr_pegs_effect_ex> w = mt_widen(eff, neff);
  return bwgr_pegsx_ex(device, eff ? w.data() : nullptr, neff, X, ldx, f, Y, n, k, maxit, logtol, covbend, covMinEv, df0, NNC, XFA, NumXFA, InnerGS, NoInv, Tr_out,
                       bfix_out, u_out, vb_out, GC_out, ve_out, hat_out, numit_out, cnv_out, bend_out);
}
