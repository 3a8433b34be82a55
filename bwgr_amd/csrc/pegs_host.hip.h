// bwgr_amd/csrc/pegs_host.hip.h -- the host entry of PEGS / PEGSZ (src/RcppEigenX20251203.cpp:10-194, :576-808) and of
// PEGS_sparse / PEGSZ_sparse (:811-1007, :1010-1250; section 4.12), which are the same fit on sparse effects under `text` 1 and 2.  Part of
// bwgr_hip.hip, after kernels_host.hip.h. It holds the fit's own algebra: the option checks, the start values and the per-sweep tail (pegs_tail.h),
// the mu shift and the outputs; the effect checks, the device arrays and every repeated step are MtFit's (mtfit_host.hip.h).  It defines no kernel.
//   once:       per panel effect k_mrr_setup_cols (uncentred), per dense effect k_pegs_dense_setup, per sparse effect k_pegs_sparse_setup;
//               k_mrr_tilde(mode 2) -> MSx
//   per sweep:  per effect in list order: mrr_sweep (panel), k_mrr_linv -> k_pegs_dense_leg (dense) or k_mrr_linv -> k_pegs_sparse_leg /
//               k_pegs_sparse_leg_disjoint (sparse), all against one residual;
//               k_mrr_ey -> (host: ve) -> k_mrr_tilde(mode 0) per effect -> (host, pegs_tail.h: vb, XFA, NNC, bending, pinv, mu, cnv) ->
//               k_mrr_mu_shift
//   at the end: hat = sum over the effects, in list order, of X b (k_mrr_hat_part / k_mrr_hat_finish), Z b (k_pegs_zb) or S b (k_pegs_sparse_hat),
//               plus mu
// ------------------------------------------------------------------------------------------------
// text: 0 PEGSZ's, 1 PEGS's own (PEGS_sparse is text 1 on a sparse effect), 2 PEGSZ_sparse's (include/bwgr.h lists what the sparse texts change)
extern "C" int bwgr_pegs_ex(int device, const bwgr_pegs_effect_ex *eff, int neff, const double *Y, int64_t n, int k, int maxit, double logtol, double covbend,
                            double covMinEv, int XFA, int NNC, int text, double *mu_out, double *const *b_out, double *hat_out, double *h2_out,
                            double *const *GC_out, double *bend_out, int *numit_out, double *cnv_out) {
  if (!eff || !Y || !b_out || !numit_out) return fail(BWGR_EINVAL, "pegs: null pointer");
  if (neff < 1) return fail(BWGR_EINVAL, "pegs: %d effects (at least 1)", neff);
  if (k < 1 || k > BWGR_MRR_MAXK) return fail(BWGR_EINVAL, "pegs: k = %d traits; this engine takes 1 <= k <= %d", k, BWGR_MRR_MAXK);
  if (n < 1) return fail(BWGR_EINVAL, "pegs: n = %lld rows (at least 1)", (long long)n);
  if (text < 0 || text > 2) return fail(BWGR_EINVAL, "pegs: text = %d (0: PEGSZ's, 1: PEGS's own, 2: PEGSZ_sparse's)", text);
  const PegsOpts o = {maxit, logtol, covbend, covMinEv, XFA, NNC != 0, text == 1, text == 2};
  if (const char *why = pegs_refuses(k, o))
    return fail(BWGR_EINVAL, "pegs: %s (maxit = %d, logtol = %g, covbend = %g, covMinEv = %g, XFA = %d, k = %d)", why, maxit, logtol, covbend, covMinEv, XFA, k);
  MtList E;                                      // (before the traits, which need its ld, and the fit, whose holder waits for the stream)
  CHK(mt_check_effects("pegs", "b", eff, neff, n, device, b_out, E));
  // ---- host set-up (:22-40, :596-614): nt, mu, the centred y and vy with 1 / (n - 1) ----
  const TraitSet S = read_traits(Y, n, k, E.ld, k, RowRule::AtLeastTwo);
  if (S.bad >= 0) return fail(BWGR_EINVAL, "pegs: trait %d has %g observed rows (needs 2)", (int)S.bad, S.nt[(size_t)S.bad]);
  const Patterns pat = find_patterns(S, 0, k);
  PegsState T;
  MtFit M(E, k);
  M.masks(S, pat);
  M.alloc(hat_out != nullptr, true);
  if (M.bufs.failed()) return no_memory("pegs");
  CHK(M.upload(S, S.sumy.data()));                                                                 // e = y, :73
  // ---- per effect: XX, XSX, tilde of the raw columns (:43-51, :66), b = 0, MSx ----
  std::vector<double> MSx((size_t)neff * k);
  for (int e = 0; e < neff; ++e) {
    const MtEffect &F = M.eff[(size_t)e];
    CHK(M.stage_effect(e));
    CHK(M.setup_effect(e, 0));
    CHK(M.reduce(F.b(), F.tilde(), F.XSX(), F.m, 2, k, nullptr, MSx.data() + (size_t)e * k));
  }
  {
    int be = 0, bt = 0;
    if (!pegs_init(T, k, neff, S.nt.data(), S.vy.data(), S.mu.data(), MSx.data(), &be, &bt))
      return fail(BWGR_EINVAL, "pegs: effect %d has TrXSX = %g for trait %d (its columns do not vary over the trait's records): the start value ve / MSx is not finite", be,
                  S.nt[(size_t)bt] * MSx[(size_t)be * k + bt], bt);
  }
  // ---- sweeps ----
  std::vector<double> ey(2 * (size_t)k), TH((size_t)neff * k * k), db2((size_t)neff);
  while (T.numit < maxit) {
    for (int t = 0; t < k; ++t) M.mc.iVe[t] = 1.0 / T.ve[(size_t)t];
    for (int e = 0; e < neff; ++e) CHK(M.sweep_effect(e, T.numit, T.eff[(size_t)e].iG.data()));
    CHK(M.residual_sums(ey.data()));
    for (int e = 0; e < neff; ++e) CHK(M.effect_sums(e, TH.data() + (size_t)e * k * k, &db2[(size_t)e]));
    const bool stop = pegs_after_sweep(T, o, ey.data(), TH.data(), db2.data(), M.d.data(), nullptr);
    CHK(M.mu_shift());
    HIPCHK(hipStreamSynchronize(M.st));            // (d is rewritten by the next sweep's tail)
    if (cnv_out) cnv_out[T.numit - 1] = T.cnv;
    if (stop) break;
  }
  if (cnv_out && T.numit == 0) cnv_out[0] = T.cnv;
  // ---- results: b, the fitted values of every row (:176-177, :777-781), h2 and GC ----
  const size_t nn = (size_t)n;
  if (hat_out) {
    HIPCHK(zero(M.st, M.hatd, nn * k));
    CHK(M.stage_vec(M.off));                       // (zero: mu is added on the host)
  }
  for (int e = 0; e < neff; ++e) {
    CHK(M.read_b(e, b_out[e]));
    if (hat_out) CHK(M.add_effect_hat(e));
  }
  if (hat_out) {
    HIPCHK(d2h(M.st, hat_out, M.hatd, sizeof(double) * nn * k));
    for (int t = 0; t < k; ++t) for (int64_t r = 0; r < n; ++r) hat_out[(size_t)t * nn + (size_t)r] += T.mu[(size_t)t];
  }
  std::vector<double> h2(k), GC((size_t)neff * k * k);
  pegs_finish(T, h2.data(), GC.data());
  *numit_out = T.numit;
  for (int t = 0; t < k; ++t) {
    if (mu_out) mu_out[t] = T.mu[(size_t)t];
    if (h2_out) h2_out[t] = h2[(size_t)t];
  }
  for (int e = 0; e < neff; ++e) {
    if (bend_out) bend_out[e] = T.eff[(size_t)e].inflate;
    if (GC_out && GC_out[e])
      for (int i = 0; i < k; ++i) for (int j = 0; j < k; ++j) GC_out[e][j * k + i] = GC[(size_t)e * k * k + i * k + j];   // column-major (symmetric)
  }
  return BWGR_OK;
}

// the narrow effects as wide ones (at least one entry, so that an empty list is refused for its length and not for a null pointer)
static std::vector<bwgr_pegs_effect_ex> mt_widen(const bwgr_pegs_effect *eff, int neff) {
  std::vector<bwgr_pegs_effect_ex> w((size_t)std::max(neff, 1), bwgr_pegs_effect_ex{nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr, 0});
  for (int e = 0; eff && e < neff; ++e) { w[(size_t)e].panel = eff[e].panel; w[(size_t)e].Z = eff[e].Z; w[(size_t)e].q = eff[e].q; w[(size_t)e].ldz = eff[e].ldz; }
  return w;
}
extern "C" int bwgr_pegs(int device, const bwgr_pegs_effect *eff, int neff, const double *Y, int64_t n, int k, int maxit, double logtol, double covbend,
                         double covMinEv, int XFA, int NNC, int own_text, double *mu_out, double *const *b_out, double *hat_out, double *h2_out,
                         double *const *GC_out, double *bend_out, int *numit_out, double *cnv_out) {
  const std::vector<bwgr_pegs_effect_ex> w = mt_widen(eff, neff);
  return bwgr_pegs_ex(device, eff ? w.data() : nullptr, neff, Y, n, k, maxit, logtol, covbend, covMinEv, XFA, NNC, own_text != 0 ? 1 : 0, mu_out, b_out, hat_out, h2_out,
                      GC_out, bend_out, numit_out, cnv_out);
}
