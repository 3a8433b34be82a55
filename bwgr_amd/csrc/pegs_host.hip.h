// bwgr_amd/csrc/pegs_host.hip.h -- the host entry of PEGS / PEGSZ (src/RcppEigenX20251203.cpp:10-194, :576-808).  Part of
// bwgr_hip.hip, after fits_host.hip.h, whose mrr_sweep runs every panel effect's share of a sweep; it defines no kernel.
//   once:       per panel effect k_mrr_setup_cols (uncentred), per dense effect k_pegs_dense_setup; k_mrr_tilde(mode 2) -> MSx
//   per sweep:  per effect in list order: mrr_sweep (panel) or k_mrr_linv -> k_pegs_dense_leg (dense), all against one residual;
//               k_mrr_ey -> (host: ve) -> k_mrr_tilde(mode 0) per effect -> (host, pegs_tail.h: vb, XFA, NNC, bending, pinv, mu, cnv) ->
//               k_mrr_mu_shift
//   at the end: hat = sum over the effects, in list order, of X b (k_mrr_hat_part / k_mrr_hat_finish) or Z b (k_pegs_zb), plus mu
// ------------------------------------------------------------------------------------------------
// The dense leg's plan, decided here and nowhere else (bwgr_debug_pegs_plan exposes it to the CPU tests)
struct PegsDensePlan { int threads; size_t lds_bytes, ws_bytes; };
static PegsDensePlan pegs_dense_plan(int64_t n, int64_t q, int k) {
  PegsDensePlan pl;
  pl.threads = (int)std::min<int64_t>(PEGS_TMAX, (n + 63) / 64 * 64);   // one row per thread up to 1024 rows, whole waves
  pl.lds_bytes = pegs_leg_lds(pl.threads);
  const size_t nq = (size_t)q, qk = nq * (size_t)k;
  pl.ws_bytes = sizeof(double) * ((size_t)n * nq + 4 * qk + qk * (size_t)k + MRR_KMAX) + sizeof(int32_t) * nq;
  return pl;
}
extern "C" int bwgr_debug_pegs_plan(int64_t n, int64_t q, int k, int64_t out[BWGR_PEGS_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "pegs plan: null pointer");
  if (n < 1 || q < 1 || k < 1 || k > BWGR_MRR_MAXK)
    return fail(BWGR_EINVAL, "pegs plan: n = %lld, q = %lld (each at least 1), k = %d (1 <= k <= %d)", (long long)n, (long long)q, k, BWGR_MRR_MAXK);
  const PegsDensePlan pl = pegs_dense_plan(n, q, k);
  out[0] = pl.threads; out[1] = (int64_t)pl.lds_bytes; out[2] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

// workgroups of k_pegs_dense_setup for an effect of q columns: one column per wave, four per workgroup and trip (bwgr_pegs, bwgr_pegsx and
// bwgr_debug_pegs_launch_plan share it)
static inline int64_t pegs_dense_setup_grid(int64_t q) { return std::min<int64_t>((q + 3) / 4, MRR_SETUP_WG); }

// a dense effect on the device
struct PegsDense {
  int64_t q = 0;
  double *Zd = nullptr, *XXd = nullptr, *XSXd = nullptr, *tilde = nullptr, *bd = nullptr, *Linv = nullptr, *db2 = nullptr;
  int32_t *ordd = nullptr;
};

extern "C" int bwgr_pegs(int device, const bwgr_pegs_effect *eff, int neff, const double *Y, int64_t n, int k, int maxit, double logtol, double covbend,
                         double covMinEv, int XFA, int NNC, int own_text, double *mu_out, double *const *b_out, double *hat_out, double *h2_out,
                         double *const *GC_out, double *bend_out, int *numit_out, double *cnv_out) {
  if (!eff || !Y || !b_out || !numit_out) return fail(BWGR_EINVAL, "pegs: null pointer");
  if (neff < 1) return fail(BWGR_EINVAL, "pegs: %d effects (at least 1)", neff);
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "pegs: k = %d traits; this engine takes 1 <= k <= %d", k, BWGR_MRR_MAXK);
  if (n < 1) return fail(BWGR_EINVAL, "pegs: n = %lld rows (at least 1)", (long long)n);
  const PegsOpts o = {maxit, logtol, covbend, covMinEv, XFA, NNC != 0, own_text != 0};
  if (const char *why = pegs_refuses(k, o))
    return fail(BWGR_EINVAL, "pegs: %s (maxit = %d, logtol = %g, covbend = %g, covMinEv = %g, XFA = %d, k = %d)", why, maxit, logtol, covbend, covMinEv, XFA, k);
  // ---- the effects: one n, one device, one row padding ----
  const bwgr_panel *P0 = nullptr;
  for (int e = 0; e < neff; ++e) {
    if (!b_out[e]) return fail(BWGR_EINVAL, "pegs: null pointer (b of effect %d)", e);
    const bwgr_panel *P = eff[e].panel;
    if (P) {
      if (P->data->is_f32) return fail(BWGR_EINVAL, "pegs: effect %d's panel holds fp32 genotypes; pegs takes int8 panels only", e);
      if (P->data->n != n) return fail(BWGR_EINVAL, "pegs: effect %d has %lld rows, Y %lld", e, (long long)P->data->n, (long long)n);
      if (!P0) P0 = P;
      if (P->data->device != P0->data->device) return fail(BWGR_EINVAL, "pegs: effect %d's panel is on device %d, the first panel on device %d", e, P->data->device, P0->data->device);
      if (P->data->plan.ld != P0->data->plan.ld)
        return fail(BWGR_EINVAL, "pegs: effect %d's panel pads its rows to ld = %lld, the first panel to %lld (make the panels with the same block / nwg)", e,
                    (long long)P->data->plan.ld, (long long)P0->data->plan.ld);
    } else {
      if (!eff[e].Z) return fail(BWGR_EINVAL, "pegs: effect %d has neither a panel nor Z", e);
      if (eff[e].q < 1 || eff[e].q > 0x7FFFFF00ll || eff[e].ldz < n)
        return fail(BWGR_EINVAL, "pegs: effect %d: q = %lld columns of Z, ldz = %lld (q at least 1, ldz at least n = %lld)", e, (long long)eff[e].q, (long long)eff[e].ldz, (long long)n);
    }
  }
  std::vector<std::vector<double>> Zc((size_t)neff);
  for (int e = 0; e < neff; ++e)
    if (!eff[e].panel) {
      int64_t r = 0, j = 0;
      if (!compact_z(eff[e].Z, n, eff[e].q, eff[e].ldz, Zc[(size_t)e], &r, &j)) return fail(BWGR_EINVAL, "pegs: effect %d: Z[%lld, %lld] is not finite", e, (long long)r, (long long)j);
    }
  if (P0) HIPCHK(hipSetDevice(P0->data->device)); else CHK(require_device(device));
  const int64_t ld = P0 ? P0->data->plan.ld : (n + 127) / 128 * 128;
  // ---- host set-up (:22-40, :596-614): nt, mu, the centred y and vy with 1 / (n - 1) ----
  const TraitSet S = read_traits(Y, n, k, ld, k, RowRule::AtLeastTwo);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "pegs: trait %d has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns pat = find_patterns(S, 0, k);
  const int npat = (int)pat.rep.size();
  MrrConst mc; memset(&mc, 0, sizeof(mc));
  mc.k = k; mc.npat = npat;
  for (int t = 0; t < k; ++t) { mc.pt[t] = pat.id[(size_t)t]; mc.nt[t] = S.nt[(size_t)t]; }
  std::vector<uint32_t> zt((size_t)ld), zb((size_t)ld);
  std::vector<uint8_t> zm;
  pack_row_bits(S, (int64_t)0, k, zt.data());
  pack_row_bits(S, pat.rep.data(), npat, zb.data());
  append_byte_masks(S, pat.rep.data(), npat, zm);

  hipStream_t st = P0 ? P0->stream : nullptr;
  std::vector<CumulativeOrder> order;            // (these are copied from asynchronously: declared before the holder, which waits for the stream)
  for (int e = 0; e < neff; ++e) order.emplace_back((size_t)(eff[e].panel ? eff[e].panel->data->p : eff[e].q));
  PegsState T;
  std::vector<double> d(k), zero_off(k, 0.0);
  DevBufs bufs(st);
  const int G = (int)mrr_pass_grid(ld), NP = MRR_NP;
  const size_t nl = (size_t)ld, nn = (size_t)n;
  uint32_t *zbd = bufs.get<uint32_t>(nl), *ztd = bufs.get<uint32_t>(nl);
  uint8_t *zmd = bufs.get<uint8_t>((size_t)npat * nl);
  double *yd = bufs.get<double>(k * nl), *ed = bufs.get<double>(k * nl);
  double *part = bufs.get<double>((size_t)G * (MRR_MB + 1) * MRR_KMAX), *dB = bufs.get<double>(MRR_MB * MRR_KMAX + MRR_KMAX);
  double *small = bufs.get<double>(1024);            // [0, 512): reduction results; [512, 768): iG; [768, ...): mu shift, the fitted values' offset
  double *tpart = bufs.get<double>((size_t)NP * (MRR_KMAX * MRR_KMAX + MRR_KMAX)), *sumyd = bufs.get<double>(MRR_KMAX);
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
  if (bufs.failed()) return no_memory("pegs");
  HIPCHK(h2d(st, zbd, zb.data(), nl));
  HIPCHK(h2d(st, ztd, zt.data(), nl));
  HIPCHK(h2d(st, zmd, zm.data(), zm.size()));
  HIPCHK(h2d(st, yd, S.y.data(), k * nl));
  HIPCHK(h2d(st, ed, S.y.data(), k * nl));                                                         // e = y, :73
  HIPCHK(h2d(st, sumyd, S.sumy.data(), (size_t)k));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_linv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
  HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
  // a reduction over an effect's m columns of the k^2 products b'tilde (mode 0) or of XSX's k columns (mode 2), partials in a fixed order
  auto reduce = [&](const double *b, const double *tilde, const double *XSX, int64_t m, int mode, int nout, double *out) -> hipError_t {
    hipLaunchKernelGGL(k_mrr_tilde, dim3(NP, nout), dim3(256), 0, st, b, tilde, XSX, m, mode, mc, (const double *)nullptr, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, NP, nout, small);
    hipError_t e_ = hipGetLastError();
    return e_ != hipSuccess ? e_ : d2h(st, out, small, sizeof(double) * nout);
  };
  // ---- per effect: XX, XSX, tilde of the raw columns (:43-51, :66), b = 0, MSx ----
  std::vector<double> MSx((size_t)neff * k);
  for (int e = 0; e < neff; ++e) {
    if (eff[e].panel) {
      const MrrLeg &L = legs[(size_t)e];
      const PanelData *D = L.P->data;
      HIPCHK(zero(st, L.bd, (size_t)L.p * k));
      hipLaunchKernelGGL(k_mrr_setup_cols, dim3((unsigned)mrr_setup_grid(L.p)), dim3(TAIL_THREADS), 0, st, (const int8_t *)D->X, D->plan.R, (int)n, L.p, ld,
                         (const uint32_t *)zbd, (const double *)yd, (const double *)sumyd, mc, 0, L.xbar, L.Sd, L.XXd, L.XSXd, L.tilde);
      HIPCHK(hipGetLastError());
      HIPCHK(reduce(L.bd, L.tilde, L.XSXd, L.p, 2, k, MSx.data() + (size_t)e * k));
    } else {
      const PegsDense &D = dense[(size_t)e];
      HIPCHK(h2d(st, D.Zd, Zc[(size_t)e].data(), Zc[(size_t)e].size()));
      HIPCHK(zero(st, D.bd, (size_t)D.q * k));
      hipLaunchKernelGGL(k_pegs_dense_setup, dim3((unsigned)pegs_dense_setup_grid(D.q)), dim3(TAIL_THREADS), 0, st, (const double *)D.Zd, n, D.q, ld,
                         (const uint32_t *)ztd, (const double *)yd, mc, D.XXd, D.XSXd, D.tilde);
      HIPCHK(hipGetLastError());
      HIPCHK(reduce(D.bd, D.tilde, D.XSXd, D.q, 2, k, MSx.data() + (size_t)e * k));
    }
  }
  {
    int be = 0, bt = 0;
    if (!pegs_init(T, k, neff, S.nt.data(), S.vy.data(), S.mu.data(), MSx.data(), &be, &bt))
      return fail(BWGR_EINVAL, "pegs: effect %d has TrXSX = %g for trait %d (its columns do not vary over the trait's records): the start value ve / MSx is not finite", be,
                  S.nt[(size_t)bt] * MSx[(size_t)be * k + bt], bt);
  }
  // ---- sweeps ----
  const MrrPlan plan = mrr_plan(k, npat);
  const MrrSweepShared W = {ld, G, npat, ztd, zmd, ed, part, dB, small + 512};
  const PegsDensePlan dpl = pegs_dense_plan(n, 1, k);
  std::vector<double> ey(2 * (size_t)k), TH((size_t)neff * k * k), db2((size_t)neff), db2t(MRR_KMAX);
  while (T.numit < maxit) {
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
    const bool stop = pegs_after_sweep(T, o, ey.data(), TH.data(), db2.data(), d.data(), nullptr);
    HIPCHK(h2d(st, small + 768, d.data(), (size_t)k));
    hipLaunchKernelGGL(k_mrr_mu_shift, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, ed, (const uint32_t *)ztd, ld, (int)n, k, (const double *)(small + 768));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));              // (d is rewritten by the next sweep's tail)
    if (cnv_out) cnv_out[T.numit - 1] = T.cnv;
    if (stop) break;
  }
  if (cnv_out && T.numit == 0) cnv_out[0] = T.cnv;
  // ---- results: b, the fitted values of every row (:176-177, :777-781), h2 and GC ----
  if (hat_out) {
    HIPCHK(zero(st, hatd, nn * k));
    HIPCHK(h2d(st, small + 768, zero_off.data(), (size_t)k));
  }
  for (int e = 0; e < neff; ++e) {
    const bool pan = eff[e].panel != nullptr;
    const int64_t m = pan ? legs[(size_t)e].p : dense[(size_t)e].q;
    const double *bd = pan ? legs[(size_t)e].bd : dense[(size_t)e].bd;
    std::vector<double> bh((size_t)m * k);
    HIPCHK(d2h(st, bh.data(), bd, sizeof(double) * m * k));
    for (int t = 0; t < k; ++t) for (int64_t j = 0; j < m; ++j) b_out[e][(size_t)t * m + j] = bh[(size_t)j * k + t];   // m x k column-major
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
  if (hat_out) {
    HIPCHK(d2h(st, hat_out, hatd, sizeof(double) * nn * k));
    for (int t = 0; t < k; ++t) for (int64_t r = 0; r < n; ++r) hat_out[(size_t)t * nn + (size_t)r] += T.mu[(size_t)t];
  }
  std::vector<double> h2(k), GC((size_t)neff * k * k);
  pegs_finish(T, h2.data(), GC.data());
  for (int t = 0; t < k; ++t) {
    if (mu_out) mu_out[t] = T.mu[(size_t)t];
    if (h2_out) h2_out[t] = h2[(size_t)t];
  }
  for (int e = 0; e < neff; ++e) {
    if (bend_out) bend_out[e] = T.eff[(size_t)e].inflate;
    if (GC_out && GC_out[e])
      for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC_out[e][j * k + i] = GC[(size_t)e * k * k + i * k + j];   // column-major (symmetric)
  }
  *numit_out = T.numit;
  return BWGR_OK;
}
