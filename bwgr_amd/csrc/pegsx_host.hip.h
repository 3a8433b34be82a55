// bwgr_amd/csrc/pegsx_host.hip.h -- the host entry of PEGSX (src/RcppEigenX20251203.cpp:197-573): PEGSZ's effects with a
// fixed design X beside them.  Part of bwgr_hip.hip, after pegs_host.hip.h, whose structure, effect checks and dense-effect holder it shares; it
// defines no kernel.
//   once:       host (pegsx_setup.h): masks, patterns, per pattern (M'M)^+, b, the projected y.  Per effect k_mrr_setup_cols (uncentred) or
//               k_pegs_dense_setup -> ZZ, tilde; k_mrr_tilde(mode 2) on ZZ; k_pegsx_trace_panel / _dense -> k_mrr_finish -> TrZSZ
//   per sweep:  per effect in list order: mrr_sweep (panel) or k_mrr_linv -> k_pegs_dense_leg (dense); k_pegsx_fixed; k_mrr_ey ->
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

extern "C" int bwgr_pegsx(int device, const bwgr_pegs_effect *eff, int neff, const double *X, int64_t ldx, int f, const double *Y, int64_t n, int k, int maxit,
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
  // ---- the effects: one n, one device, one row padding (bwgr_pegs's checks) ----
  const bwgr_panel *P0 = nullptr;
  for (int e = 0; e < neff; ++e) {
    if (!u_out[e]) return fail(BWGR_EINVAL, "pegsx: null pointer (u of effect %d)", e);
    const bwgr_panel *P = eff[e].panel;
    if (P) {
      if (P->data->is_f32) return fail(BWGR_EINVAL, "pegsx: effect %d's panel holds fp32 genotypes; pegsx takes int8 panels only", e);
      if (P->data->n != n) return fail(BWGR_EINVAL, "pegsx: effect %d has %lld rows, Y %lld", e, (long long)P->data->n, (long long)n);
      if (!P0) P0 = P;
      if (P->data->device != P0->data->device) return fail(BWGR_EINVAL, "pegsx: effect %d's panel is on device %d, the first panel on device %d", e, P->data->device, P0->data->device);
      if (P->data->plan.ld != P0->data->plan.ld)
        return fail(BWGR_EINVAL, "pegsx: effect %d's panel pads its rows to ld = %lld, the first panel to %lld (make the panels with the same block / nwg)", e,
                    (long long)P->data->plan.ld, (long long)P0->data->plan.ld);
    } else {
      if (!eff[e].Z) return fail(BWGR_EINVAL, "pegsx: effect %d has neither a panel nor Z", e);
      if (eff[e].q < 1 || eff[e].q > 0x7FFFFF00ll || eff[e].ldz < n)
        return fail(BWGR_EINVAL, "pegsx: effect %d: q = %lld columns of Z, ldz = %lld (q at least 1, ldz at least n = %lld)", e, (long long)eff[e].q, (long long)eff[e].ldz, (long long)n);
    }
  }
  std::vector<std::vector<double>> Zc((size_t)neff);
  for (int e = 0; e < neff; ++e)
    if (!eff[e].panel) {
      int64_t r = 0, j = 0;
      if (!compact_z(eff[e].Z, n, eff[e].q, eff[e].ldz, Zc[(size_t)e], &r, &j)) return fail(BWGR_EINVAL, "pegsx: effect %d: Z[%lld, %lld] is not finite", e, (long long)r, (long long)j);
    }
  if (P0) HIPCHK(hipSetDevice(P0->data->device)); else CHK(require_device(device));
  const int64_t ld = P0 ? P0->data->plan.ld : (n + 127) / 128 * 128;
  // ---- host set-up (:227-260): masks, patterns, (M'M)^+ per pattern, b, the projected y ----
  const FixedSet F = read_fixed(Y, X, n, k, f, ldx, ld);
  if (F.bad_row >= 0) return fail(BWGR_EINVAL, "pegsx: X[%lld, %lld] is not finite", (long long)F.bad_row, (long long)F.bad_col);
  const TraitSet &S = F.S;
  if (S.bad >= 0) return fail(BWGR_EINVAL, "pegsx: trait %d has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns &pat = F.pat;
  const int npat = (int)pat.rep.size();
  MrrConst mc; memset(&mc, 0, sizeof(mc));
  mc.k = k; mc.npat = npat;
  for (int t = 0; t < k; ++t) { mc.pt[t] = pat.id[(size_t)t]; mc.nt[t] = S.nt[(size_t)t]; }
  std::vector<uint32_t> zt((size_t)ld), zb((size_t)ld);
  std::vector<uint8_t> zm;
  pack_row_bits(S, (int64_t)0, k, zt.data());
  pack_row_bits(S, pat.rep.data(), npat, zb.data());
  append_byte_masks(S, pat.rep.data(), npat, zm);
  std::vector<double> bfk((size_t)f * k);                                                          // b as the kernels hold it: [f][k]
  for (int t = 0; t < k; ++t) for (int c = 0; c < f; ++c) bfk[(size_t)c * k + t] = F.b[(size_t)t * f + c];

  hipStream_t st = P0 ? P0->stream : nullptr;
  std::vector<CumulativeOrder> order;            // (these are copied from asynchronously: declared before the holder, which waits for the stream)
  for (int e = 0; e < neff; ++e) order.emplace_back((size_t)(eff[e].panel ? eff[e].panel->data->p : eff[e].q));
  PegsxState T;
  DevBufs bufs(st);
  const int G = (int)mrr_pass_grid(ld), NP = MRR_NP;
  const size_t nl = (size_t)ld, nn = (size_t)n, nf = (size_t)f;
  int64_t mmax = 1;
  for (int e = 0; e < neff; ++e) mmax = std::max<int64_t>(mmax, eff[e].panel ? eff[e].panel->data->p : eff[e].q);
  uint32_t *zbd = bufs.get<uint32_t>(nl), *ztd = bufs.get<uint32_t>(nl);
  uint8_t *zmd = bufs.get<uint8_t>((size_t)npat * nl);
  double *yd = bufs.get<double>(k * nl), *ed = bufs.get<double>(k * nl);
  double *part = bufs.get<double>((size_t)G * (MRR_MB + 1) * MRR_KMAX), *dB = bufs.get<double>(MRR_MB * MRR_KMAX + MRR_KMAX);
  double *small = bufs.get<double>(1024);            // [0, 512): reduction results; [512, 768): iG; [768, ...): the fitted values' offset (zero)
  double *tpart = bufs.get<double>((size_t)NP * (MRR_KMAX * MRR_KMAX + MRR_KMAX)), *sumyd = bufs.get<double>(MRR_KMAX);
  double *Xd = bufs.get<double>(nn * nf), *iXXd = bufs.get<double>((size_t)npat * nf * nf), *bfd = bufs.get<double>(nf * k);
  double *qpart = bufs.get<double>((size_t)pegsx_trace_grid(mmax) * npat);
  std::vector<MrrLeg> legs((size_t)neff);
  std::vector<PegsDense> dense((size_t)neff);
  int nch_max = 1;
  for (int e = 0; e < neff; ++e) {
    if (eff[e].panel) {
      mrr_leg_alloc(bufs, legs[(size_t)e], eff[e].panel, npat, k);
      nch_max = std::max(nch_max, (int)std::min<int64_t>(64, legs[(size_t)e].p));
    } else {
      PegsDense &D = dense[(size_t)e];
      D.q = eff[e].q;
      const size_t nq = (size_t)D.q, qk = nq * k;
      D.Zd = bufs.get<double>(nn * nq); D.XXd = bufs.get<double>(qk); D.XSXd = bufs.get<double>(qk); D.tilde = bufs.get<double>(qk); D.bd = bufs.get<double>(qk);
      D.Linv = bufs.get<double>(qk * k); D.db2 = bufs.get<double>(MRR_KMAX); D.ordd = bufs.get<int32_t>(nq);
    }
  }
  double *hatd = hat_out ? bufs.get<double>(nn * k) : nullptr, *hpart = (hat_out && P0) ? bufs.get<double>((size_t)nch_max * k * nl) : nullptr;
  double *htmp = (hat_out && P0) ? bufs.get<double>(nn * k) : nullptr;
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
  HIPCHK(h2d(st, zbd, zb.data(), nl));
  HIPCHK(h2d(st, ztd, zt.data(), nl));
  HIPCHK(h2d(st, zmd, zm.data(), zm.size()));
  HIPCHK(h2d(st, yd, S.y.data(), k * nl));
  HIPCHK(h2d(st, ed, S.y.data(), k * nl));                                                         // e = y, :367
  HIPCHK(zero(st, sumyd, (size_t)MRR_KMAX));                                                       // (read by the uncentred set-up, times xbar = 0)
  HIPCHK(zero(st, small, (size_t)1024));
  HIPCHK(h2d(st, Xd, F.X.data(), nn * nf));
  HIPCHK(h2d(st, iXXd, F.iXX.data(), (size_t)npat * nf * nf));
  HIPCHK(h2d(st, bfd, bfk.data(), nf * k));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_linv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
  const PegsxPlan xpl = pegsx_plan(n, f, k);
  auto reduce = [&](const double *b, const double *tilde, const double *XSX, int64_t m, int mode, int nout, double *out) -> hipError_t {
    hipLaunchKernelGGL(k_mrr_tilde, dim3(NP, nout), dim3(256), 0, st, b, tilde, XSX, m, mode, mc, (const double *)nullptr, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, NP, nout, small);
    hipError_t e_ = hipGetLastError();
    return e_ != hipSuccess ? e_ : d2h(st, out, small, sizeof(double) * nout);
  };
  // ---- per effect: ZZ and tilde of the raw columns (:277-290, :325-330), u = 0, TrZSZ (:292-323) ----
  std::vector<double> Tr((size_t)neff * k), szz(k), quad(npat);
  for (int e = 0; e < neff; ++e) {
    const bool pan = eff[e].panel != nullptr;
    const int64_t m = pan ? legs[(size_t)e].p : dense[(size_t)e].q;
    const unsigned tg = (unsigned)pegsx_trace_grid(m);
    if (pan) {
      const MrrLeg &L = legs[(size_t)e];
      const PanelData *D = L.P->data;
      HIPCHK(zero(st, L.bd, (size_t)L.p * k));
      if (timing) HIPCHK(hipEventRecord(ev0, st));
      hipLaunchKernelGGL(k_mrr_setup_cols, dim3((unsigned)mrr_setup_grid(L.p)), dim3(TAIL_THREADS), 0, st, (const int8_t *)D->X, D->plan.R, (int)n, L.p, ld,
                         (const uint32_t *)zbd, (const double *)yd, (const double *)sumyd, mc, 0, L.xbar, L.Sd, L.XXd, L.XSXd, L.tilde);
      HIPCHK(hipGetLastError());
      if (timing) HIPCHK(lap(ms_cols));
      HIPCHK(reduce(L.bd, L.tilde, L.XXd, L.p, 2, k, szz.data()));
      if (timing) HIPCHK(hipEventRecord(ev0, st));
      hipLaunchKernelGGL(k_pegsx_trace_panel, dim3(tg), dim3(256), xpl.lds_trace, st, (const int8_t *)D->X, D->plan.R, L.p, ld, (const double *)Xd, n, f,
                         (const uint32_t *)zbd, npat, (const double *)iXXd, qpart);
    } else {
      const PegsDense &D = dense[(size_t)e];
      HIPCHK(h2d(st, D.Zd, Zc[(size_t)e].data(), Zc[(size_t)e].size()));
      HIPCHK(zero(st, D.bd, (size_t)D.q * k));
      if (timing) HIPCHK(hipEventRecord(ev0, st));
      hipLaunchKernelGGL(k_pegs_dense_setup, dim3((unsigned)pegs_dense_setup_grid(D.q)), dim3(TAIL_THREADS), 0, st, (const double *)D.Zd, n, D.q, ld,
                         (const uint32_t *)ztd, (const double *)yd, mc, D.XXd, D.XSXd, D.tilde);
      HIPCHK(hipGetLastError());
      if (timing) HIPCHK(lap(ms_cols));
      HIPCHK(reduce(D.bd, D.tilde, D.XXd, D.q, 2, k, szz.data()));
      if (timing) HIPCHK(hipEventRecord(ev0, st));
      hipLaunchKernelGGL(k_pegsx_trace_dense, dim3(tg), dim3(256), xpl.lds_trace, st, (const double *)D.Zd, D.q, ld, (const double *)Xd, n, f, (const uint32_t *)zbd, npat,
                         (const double *)iXXd, qpart);
    }
    HIPCHK(hipGetLastError());
    if (timing) HIPCHK(lap(ms_trace));
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)qpart, (int)tg, npat, small);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, quad.data(), small, sizeof(double) * npat));
    for (int t = 0; t < k; ++t) Tr[(size_t)e * k + t] = szz[(size_t)t] - quad[(size_t)pat.id[(size_t)t]];
  }
  pegsx_init(T, k, neff, f, o, S.nt.data(), F.ssy.data(), Tr.data(), nullptr);
  // ---- sweeps ----
  const MrrPlan plan = mrr_plan(k, npat);
  const MrrSweepShared W = {ld, G, npat, ztd, zmd, ed, part, dB, small + 512};
  const PegsDensePlan dpl = pegs_dense_plan(n, 1, k);
  PegsxFixedArgs FA;
  FA.X = Xd; FA.n = n; FA.ld = ld; FA.f = f; FA.zt = ztd; FA.e = ed; FA.iXX = iXXd; FA.b = bfd;
  std::vector<double> ey(2 * (size_t)k), TH((size_t)neff * k * k), db2((size_t)neff), db2t(MRR_KMAX);
  while (T.numit < maxit) {
    const auto t0 = std::chrono::steady_clock::now();
    for (int t = 0; t < k; ++t) mc.iVe[t] = 1.0 / T.ve[(size_t)t];
    for (int e = 0; e < neff; ++e) {
      const std::vector<int> &ord = order[(size_t)e].next(T.numit);
      const double *iG = T.eff[(size_t)e].iG.data();
      if (eff[e].panel) { CHK(mrr_sweep(st, legs[(size_t)e], W, mc, plan, ord, iG)); continue; }
      const PegsDense &D = dense[(size_t)e];
      HIPCHK(h2d(st, D.ordd, ord.data(), (size_t)D.q));
      HIPCHK(h2d(st, W.iGd, iG, (size_t)k * k));
      hipLaunchKernelGGL(k_mrr_linv, dim3((unsigned)((D.q + 63) / 64)), dim3(64), plan.lds_linv, st, (const double *)D.XXd, (const double *)W.iGd, mc, D.q, D.Linv);
      PegsLegArgs A;
      A.Z = D.Zd; A.n = n; A.ld = ld; A.q = (int)D.q; A.zt = ztd; A.e = ed; A.order = D.ordd; A.XX = D.XXd; A.Linv = D.Linv; A.b = D.bd; A.db2 = D.db2;
      hipLaunchKernelGGL(k_pegs_dense_leg, dim3(1), dim3(dpl.threads), dpl.lds_bytes, st, A, mc);
      HIPCHK(hipGetLastError());
    }
    if (timing == 2) HIPCHK(hipEventRecord(ev0, st));
    hipLaunchKernelGGL(k_pegsx_fixed, dim3(k), dim3(xpl.threads), xpl.lds_fixed, st, FA, mc);                                          // :502-509
    if (timing == 2) { double ms = 0.0; HIPCHK(lap(ms)); ms_fixed.add(ms); }
    hipLaunchKernelGGL(k_mrr_ey, dim3(NP, k), dim3(256), 0, st, (const double *)ed, (const double *)yd, ld, k, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, NP, 2 * k, small);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, ey.data(), small, sizeof(double) * 2 * k));
    for (int e = 0; e < neff; ++e) {
      const bool pan = eff[e].panel != nullptr;
      const MrrLeg &L = legs[(size_t)e];
      const PegsDense &D = dense[(size_t)e];
      HIPCHK(reduce(pan ? L.bd : D.bd, pan ? L.tilde : D.tilde, pan ? L.XSXd : D.XSXd, pan ? L.p : D.q, 0, k * k, TH.data() + (size_t)e * k * k));
      HIPCHK(d2h(st, db2t.data(), pan ? L.db2 : D.db2, sizeof(double) * k));
      double s = 0.0;
      for (int t = 0; t < k; ++t) s += db2t[(size_t)t];
      db2[(size_t)e] = s;
    }
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
    HIPCHK(zero(st, hatd, nn * k));
    hipLaunchKernelGGL(k_pegs_zb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)Xd, n, (int64_t)f, k, (const double *)bfd, hatd);
    HIPCHK(hipGetLastError());
  }
  for (int e = 0; e < neff; ++e) {
    const bool pan = eff[e].panel != nullptr;
    const int64_t m = pan ? legs[(size_t)e].p : dense[(size_t)e].q;
    const double *bd = pan ? legs[(size_t)e].bd : dense[(size_t)e].bd;
    std::vector<double> bh((size_t)m * k);
    HIPCHK(d2h(st, bh.data(), bd, sizeof(double) * m * k));
    for (int t = 0; t < k; ++t) for (int64_t j = 0; j < m; ++j) u_out[e][(size_t)t * m + j] = bh[(size_t)j * k + t];   // m x k column-major
    if (!hat_out) continue;
    if (pan) {
      const PanelData *D = legs[(size_t)e].P->data;
      const int nch = (int)std::min<int64_t>(64, m);
      const int64_t cpc = (m + nch - 1) / nch;
      hipLaunchKernelGGL(k_mrr_hat_part, dim3((unsigned)((ld + 255) / 256), nch), dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, m, ld, (int)n, k, bd, cpc, hpart);
      hipLaunchKernelGGL(k_mrr_hat_finish, dim3((unsigned)std::min<int64_t>((n * k + 255) / 256, 4096)), dim3(256), 0, st, (const double *)hpart, nch, ld, (int)n, k,
                         (const double *)(small + 768), htmp);
      hipLaunchKernelGGL(k_pegs_add, dim3((unsigned)std::min<int64_t>((n * k + 255) / 256, 4096)), dim3(256), 0, st, hatd, (const double *)htmp, (int64_t)n * k);
    } else {
      hipLaunchKernelGGL(k_pegs_zb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)dense[(size_t)e].Zd, n, m, k, bd, hatd);
    }
    HIPCHK(hipGetLastError());
  }
  if (hat_out) HIPCHK(d2h(st, hat_out, hatd, sizeof(double) * nn * k));
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
