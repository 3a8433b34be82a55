// bwgr_amd/csrc/wgr_em_host.hip.h -- the host entries of wgr (bwgr_sample_rows, bwgr_wgr, bwgr_wgr_ex) and of the EM / Gauss-Seidel family
// (bwgr_em_order, bwgr_em).  Part of bwgr_hip.hip, which includes it after everything it uses (fail, HIPCHK, DevBufs, no_memory, d2h / h2d /
// d2d / zero, Guard, sum_floats, sweep_args, launch_sweep, the scratch panels, launch_gather_rows, gemv_launch / gemv_hat, g_last_redo); it
// defines no kernel: theirs are wgr.hip.h, em.hip.h, chain.hip.h (k_chain_init) and panel.hip.h.
// ------------------------------------------------------------------------------------------------
// wgr
// ------------------------------------------------------------------------------------------------
// host side of the RNG contract for wgr's row resampling, R/wgr.R:68: Use = sort(sample(n, n*bag, rp)) - 1
static double host_uniform(uint64_t seed, uint32_t marker, uint32_t iter, uint32_t purpose, uint32_t k) {
  uint32_t c0 = marker, c1 = iter, c2 = purpose, c3 = k, k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6) + 0.5) / 9007199254740992.0;
}
static void bag_rows(uint64_t seed, uint32_t iter, int64_t n, int64_t k, int rp, std::vector<int> &use) {
  use.resize((size_t)k);
  if (rp) {
    for (int64_t t = 0; t < k; ++t) { int r = (int)(host_uniform(seed, (uint32_t)t, iter, RNG_BAG, 1) * (double)n); use[(size_t)t] = r >= n ? (int)n - 1 : r; }
  } else {
    std::vector<std::pair<double, int>> kv((size_t)n);
    for (int64_t i = 0; i < n; ++i) kv[(size_t)i] = std::make_pair(host_uniform(seed, (uint32_t)i, iter, RNG_BAG, 0), (int)i);
    std::sort(kv.begin(), kv.end());
    for (int64_t t = 0; t < k; ++t) use[(size_t)t] = kv[(size_t)t].second;
  }
  std::sort(use.begin(), use.end());
}

extern "C" int bwgr_sample_rows(uint64_t seed, uint32_t iter, int64_t n, int64_t k, int rp, int *rows) {
  if (!rows || n < 1 || k < 0 || (!rp && k > n) || n > 0x7FFFFFFFll) return fail(BWGR_EINVAL, "sample_rows: bad arguments (n=%lld, k=%lld, rp=%d)", (long long)n, (long long)k, rp);
  std::vector<int> use;
  bag_rows(seed, iter, n, k, rp, use);
  for (int64_t t = 0; t < k; ++t) rows[t] = use[(size_t)t];
  return BWGR_OK;
}

extern "C" int bwgr_wgr(bwgr_panel *P, const double *y, int it, int bi, int th, int iv, int de, double pi, double df, double R2,
                        uint64_t seed, int rng_mode, double *mu, double *b, double *Vb, double *d, double *Ve, double *hat,
                        double *cxx) {
  return bwgr_wgr_ex(P, y, it, bi, th, iv, de, pi, df, R2, seed, rng_mode, nullptr, nullptr, 0, 1.0, 0, mu, b, Vb, d, Ve, hat, cxx, nullptr, nullptr);
}

// What wgr refuses, and the two counts the call runs on: *nbag_out, the rows an iteration sweeps (n, or n * bag of them), and *mc_out, the
// iterations the posterior means average.  U: null unless the call has a polygenic term.
static int wgr_check(const bwgr_panel *P, const double *y, const double *U, const double *V, double bag, int rp, int it, int bi, int th,
                     int64_t *nbag_out, int *mc_out) {
  if (P && P->data->cen) return refuse_centred("wgr");
  if (!P || !y) return fail(BWGR_EINVAL, "wgr: null pointer");
  if (U && !V) return fail(BWGR_EINVAL, "wgr: eigenvalues missing");
  const bool bagging = (bag != 1.0);
  if (bagging && U) return fail(BWGR_EINVAL, "wgr: bag != 1 with eigK is undefined in the reference (R/wgr.R:73-79 index a subsampled e with full row ids)");
  if (bagging && !(bag > 0.0)) return fail(BWGR_EINVAL, "wgr: bag must be > 0");
  const int64_t nbag = bagging ? (int64_t)((double)P->data->n * bag) : P->data->n;
  if (bagging && nbag < 2) return fail(BWGR_EINVAL, "wgr: n*bag < 2");
  // sample(n, n*bag, FALSE) cannot take more than the population (R errors out, R/wgr.R:68)
  if (bagging && !rp && nbag > P->data->n) return fail(BWGR_EINVAL, "wgr: bag > 1 needs rp = TRUE (cannot take %lld of %lld rows without replacement)", (long long)nbag, (long long)P->data->n);
  if (it < 1 || bi < 0 || th < 1) return fail(BWGR_EINVAL, "wgr: need it >= 1, bi >= 0, th >= 1");
  int mc = 0; for (int q = bi; q <= it; q += th) mc++;                             // post = seq(bi,it,th)
  if (mc < 1) return fail(BWGR_EINVAL, "wgr: seq(bi,it,th) is empty");
  *nbag_out = nbag; *mc_out = mc;
  return BWGR_OK;
}

extern "C" int bwgr_wgr_ex(bwgr_panel *P, const double *y, int it, int bi, int th, int iv, int de, double pi, double df, double R2,
                           uint64_t seed, int rng_mode, const double *U, const double *V, int64_t pk, double bag, int rp,
                           double *mu, double *b, double *Vb, double *d, double *Ve, double *hat, double *cxx, double *u, double *Vk) {
  // ---- set-up: the arguments, the scratch panels, the call's arrays, the start values ----
  if (!U || pk <= 0) { U = nullptr; pk = 0; }
  int64_t nbag = 0; int mc = 0;
  CHK(wgr_check(P, y, U, V, bag, rp, it, bi, th, &nbag, &mc));
  const bool bagging = (bag != 1.0);
  if (bagging) df = df / (bag * bag);                                              // R/wgr.R:20
  if (de) iv = 1;                                                                  // R/wgr.R:9
  HIPCHK(hipSetDevice(P->data->device));
  const int p = (int)P->data->p, n = (int)P->data->n;
  const size_t pd = sizeof(double) * p;
  const Rng rng = make_rng(seed, rng_mode);
  bwgr_panel *PU = nullptr;   // eigenvectors as an fp32 panel (KMUP narrows U to float like any other X)
  bwgr_panel *PB = nullptr;   // the row subsample of this iteration (bag != 1): same markers, nbag rows
  Guard drop([&] { bwgr_panel_destroy(PU); bwgr_panel_destroy(PB); });
  std::vector<int> use_h;     // (copied from asynchronously: declared before the holder, which waits for the stream)
  DevBufs bufs(P->stream);
  if (U) {
    CHK(bwgr_panel_create(&PU, U, BWGR_X_F64, BWGR_HOST, n, pk, n, P->data->device, 0, 0));
    PU->stream = P->stream;
  }
  int *use_d = nullptr;
  if (bagging) {
    CHK(scratch_panel_alloc(&PB, P, nbag, 0, PANEL_ROWS));
    CHK(scratch_alloc(PB));
    use_d = bufs.get<int>((size_t)nbag);
    if (bufs.failed()) return no_memory("wgr");
  }
  const int64_t ldmax = std::max<int64_t>(std::max<int64_t>(P->data->plan.ld, PU ? PU->data->plan.ld : 0), PB ? PB->data->plan.ld : 0);
  const size_t nk = (size_t)std::max<int64_t>(pk, 1), np = (size_t)p;
  const int nchunks = gemv_chunks(P), cpc = gemv_cpc_of(p, nchunks);   // X * coef: fp64 partial products per column chunk
  double *yd = bufs.get<double>(n), *eR = bufs.get<double>(ldmax), *e64 = bufs.get<double>(ldmax);
  double *Ud = bufs.get<double>((size_t)std::max<int64_t>(n * pk, 1)), *Vd = bufs.get<double>(nk), *hR = bufs.get<double>(nk), *Hk = bufs.get<double>(nk), *uhd = bufs.get<double>(n);
  float *hf = bufs.get<float>(nk), *dhf = bufs.get<float>(nk), *xxKf = bufs.get<float>(nk), *Lkf = bufs.get<float>(nk), *vbk = bufs.get<float>(nk);
  ChainScalars *sck = bufs.get<ChainScalars>(1);
  double *xx64 = bufs.get<double>(np), *vx64 = bufs.get<double>(np), *bR = bufs.get<double>(np), *dR = bufs.get<double>(np);
  double *VbR = bufs.get<double>(np), *LR = bufs.get<double>(np), *B = bufs.get<double>(np), *D = bufs.get<double>(np), *VB = bufs.get<double>(np);
  float *bf = bufs.get<float>(np), *dfl = bufs.get<float>(np), *Lf = bufs.get<float>(np), *xxf = bufs.get<float>(np), *vbf = bufs.get<float>(np);
  double *part1 = bufs.get<double>(256), *part2 = bufs.get<double>(256), *hatd = bufs.get<double>(n);
  WgrScalars *ws = bufs.get<WgrScalars>(1);
  ChainScalars *sc = bufs.get<ChainScalars>(1);
  double *gpart = bufs.get<double>((size_t)nchunks * P->data->plan.ld);
  if (bufs.failed()) return no_memory("wgr");
  HIPCHK(h2d(P->stream, yd, y, (size_t)n));
  if (pk > 0) {
    HIPCHK(h2d(P->stream, Ud, U, (size_t)n * pk));
    HIPCHK(h2d(P->stream, Vd, V, nk));
    HIPCHK(zero(P->stream, hR, nk)); HIPCHK(zero(P->stream, Hk, nk));
  }
  const int wpb = 4;
  if (P->data->is_f32) hipLaunchKernelGGL(k_stats64<float>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const float *)P->data->X, P->data->plan.R, n, p, xx64, vx64);
  else hipLaunchKernelGGL(k_stats64<int8_t>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.R, n, p, xx64, vx64);
  hipLaunchKernelGGL(k_dsum_stage1, dim3(256), dim3(256), 0, P->stream, vx64, (int64_t)p, part1, 0);
  hipLaunchKernelGGL(k_dsum_stage1, dim3(256), dim3(256), 0, P->stream, xx64, (int64_t)p, part2, 0);
  hipLaunchKernelGGL(k_wgr_init, dim3(1), dim3(1024), 0, P->stream, yd, eR, n, ldmax, part1, part2, p, df, R2, ws);
  hipLaunchKernelGGL(k_wgr_marker_init, dim3(1024), dim3(256), 0, P->stream, bR, dR, VbR, LR, B, D, VB, p, ws);
  if (bagging) hipLaunchKernelGGL(k_scale_d, dim3(256), dim3(256), 0, P->stream, xx64, (int64_t)p, bag);     // xx = crossprod * bag, R/wgr.R:46
  HIPCHK(hipGetLastError());
  HIPCHK(zero(P->stream, sc, 1));
  const unsigned pg = (unsigned)std::min<int64_t>(2048, (P->data->p + 255) / 256);
  // ---- the iterations ----
  for (int i = 1; i <= it; ++i) {                                                // R/wgr.R:66
    const uint32_t itx = (uint32_t)(i - 1);
    const int accumulate = (i >= bi && ((i - bi) % th) == 0) ? 1 : 0;            // i %in% post
    if (pk > 0) {                                                                // R/wgr.R:70-76
      hipLaunchKernelGGL(k_wgr_pre_k, dim3(64), dim3(256), 0, P->stream, hR, Vd, eR, hf, dhf, xxKf, Lkf, e64, (int)pk, n, ldmax, ws, sck);
      SweepArgs ak = sweep_args(PU, SWF_LAM_VEC, e64, hf, dhf, vbk, xxKf, Lkf, sck, itx, rng);
      ak.marker0 = 0x80000000u;
      CHK(launch_sweep(PU, ak));
      hipLaunchKernelGGL(k_wgr_post_k, dim3(64), dim3(256), 0, P->stream, hf, hR, e64, eR, (int)pk, n);
    }
    hipLaunchKernelGGL(k_wgr_pre, dim3(pg), dim3(256), 0, P->stream, bR, dR, LR, xx64, eR, bf, dfl, Lf, xxf, e64, p, n, ldmax, (float)pi, ws, sc);
    bwgr_panel *PS = bagging ? PB : P;                                           // the panel this iteration sweeps
    if (bagging) {                                                               // R/wgr.R:68 + KMUP2's gathers
      bag_rows(seed, itx, n, nbag, rp, use_h);
      HIPCHK(h2d(P->stream, use_d, use_h.data(), (size_t)nbag));
      launch_gather_rows(P, PB, use_d, nbag);
      CHK(panel_build_gram(PB));                                                 // syncs the stream (use_h stays valid)
      hipLaunchKernelGGL(k_gather_e, dim3(64), dim3(256), 0, P->stream, eR, use_d, (int)nbag, ldmax, e64);
      hipLaunchKernelGGL(k_set_bg, dim3(1), dim3(1), 0, P->stream, sc, (float)n / (float)nbag);
    }
    SweepArgs a = sweep_args(PS, SWF_LAM_VEC | (pi > 0 ? (SWF_SELECT | SWF_ALT_B2) : 0) | (bagging ? SWF_KMUP2 : 0) | (de ? SWF_SERIAL : 0), e64, bf, dfl,
                             vbf, xxf, Lf, sc, itx, rng);
    CHK(launch_sweep(PS, a));                                                    // KMUP / KMUP2, R/wgr.R:85
    hipLaunchKernelGGL(k_wgr_post, dim3(pg), dim3(256), 0, P->stream, bf, dfl, bR, dR, VbR, p, pi > 0 ? 1 : 0, iv, de, df, itx, rng, ws);
    hipLaunchKernelGGL(k_dsum_stage1, dim3(256), dim3(256), 0, P->stream, bR, (int64_t)p, part1, 1);
    if (pk > 0) hipLaunchKernelGGL(k_wgr_vp, dim3(1), dim3(1024), 0, P->stream, hR, Vd, (int)pk, df, itx, rng, ws);   // R/wgr.R:116-119
    hipLaunchKernelGGL(k_wgr_scal, dim3(1), dim3(1024), 0, P->stream, e64, (int)nbag, (double)n * bag, p, part1, iv, df, itx, rng, ws);
    hipLaunchKernelGGL(k_wgr_L, dim3(pg), dim3(256), 0, P->stream, bR, dR, VbR, LR, B, D, VB, p, iv, accumulate, ws);
    gemv_launch<double>(P, bR, nchunks, cpc, gpart);
    hipLaunchKernelGGL(k_wgr_efinish, dim3((n + 255) / 256), dim3(256), 0, P->stream, gpart, P->data->plan.ld, nchunks, n, yd, eR, ws);
    if (pk > 0) hipLaunchKernelGGL(k_uh, dim3((n + 255) / 256), dim3(256), 0, P->stream, Ud, hR, n, (int)pk, 1.0, eR, 1);   // - U %*% h
    hipLaunchKernelGGL(k_wgr_mu, dim3(1), dim3(1024), 0, P->stream, eR, n, iv, accumulate, itx, rng, ws);
    if (pk > 0 && accumulate) hipLaunchKernelGGL(k_wgr_accum_k, dim3(8), dim3(256), 0, P->stream, hR, Hk, (int)pk, ws);
    HIPCHK(hipGetLastError());
    if ((i & 63) == 0) HIPCHK(hipStreamSynchronize(P->stream));                  // bound the launch queue
  }
  // ---- results: the posterior means, HAT and the polygenic term ----
  hipLaunchKernelGGL(k_dsum_stage1, dim3(256), dim3(256), 0, P->stream, D, (int64_t)p, part1, 0);
  hipLaunchKernelGGL(k_wgr_final, dim3(1), dim3(1024), 0, P->stream, B, D, VB, p, (double)mc, part1, iv, ws);
  WgrScalars h; ChainScalars hc;
  HIPCHK(hipMemcpyAsync(&h, ws, sizeof(h), hipMemcpyDeviceToHost, P->stream));
  HIPCHK(hipMemcpyAsync(&hc, sc, sizeof(hc), hipMemcpyDeviceToHost, P->stream));
  HIPCHK(hipStreamSynchronize(P->stream));
  g_last_redo = (int)hc.nredo;
  if (hc.error) return sweep_error(hc.error, "wgr");
  const double B0 = h.B0 / mc;
  gemv_launch<double>(P, B, nchunks, cpc, gpart);                                // HAT = B0 + gen0 %*% B, R/wgr.R:152
  hipLaunchKernelGGL(k_hat64_finish, dim3((n + 255) / 256), dim3(256), 0, P->stream, gpart, P->data->plan.ld, nchunks, n, B0, hatd);
  if (pk > 0) {                                                                  // poly = U0 %*% H; HAT += poly, R/wgr.R:148-150
    hipLaunchKernelGGL(k_uh, dim3((n + 255) / 256), dim3(256), 0, P->stream, Ud, Hk, n, (int)pk, 1.0 / (double)mc, uhd, 0);
    hipLaunchKernelGGL(k_add_vec, dim3((n + 255) / 256), dim3(256), 0, P->stream, hatd, uhd, n);
  }
  HIPCHK(hipGetLastError());
  if (mu) *mu = B0;
  if (Ve) *Ve = h.VE / mc;
  if (cxx) *cxx = h.cxx * bag;                                                   // mean(xx), xx = crossprod * bag
  if (b) HIPCHK(d2h(P->stream, b, B, pd));
  if (d) HIPCHK(d2h(P->stream, d, D, pd));
  if (Vb) { if (iv) HIPCHK(d2h(P->stream, Vb, VB, pd)); else Vb[0] = h.VA / mc; }
  if (hat) HIPCHK(d2h(P->stream, hat, hatd, sizeof(double) * n));
  if (pk > 0 && u) HIPCHK(d2h(P->stream, u, uhd, sizeof(double) * n));
  if (pk > 0 && Vk) *Vk = h.VP / mc;
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// f4: EM / Gauss-Seidel family (emRR, emBA, emBB, emBC, emBCpi, emDE, emBL, emEN, emML), src/Rcpp20260726ai.cpp:80-521, :1502-1545
//
// Deterministic coordinate updates -- b_j = (X_j.e + xx_j b_j)/(xx_j + lambda_j), i.e. the affine sweep with the variates
// switched off, or the member's soft-selection / soft-threshold update (lane_em) -- in a marker order that the reference re-shuffles before every sweep (std::shuffle with
// std::mt19937(i), :103 ...).  The exact blocked sweep needs the Gram blocks of consecutive markers, so every sweep
//   (1) shuffles the order on the host with the very library call the reference makes,
//   (2) gathers the columns of the resident panel into a scratch panel in that order (one pass over X),
//   (3) rebuilds the scratch panel's diagonal and distance-1 Gram blocks,
//   (4) runs the affine sweep kernel on it (b, xx, lambda gathered; b scattered back),
//   (5) runs the model's tail (variance components, lambda, intercept) in one workgroup.
// ------------------------------------------------------------------------------------------------
// the marker order of sweep `upto` (0-based): identity shuffled with std::mt19937(0), (1), ..., (upto) -- the library's own
// std::shuffle, so that the oracle's restatement of it can be pinned (tests/test_em_order.py)
extern "C" int bwgr_em_order(int64_t p, int upto, int32_t *order) {
  if (!order || p < 1 || p > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "em_order: bad arguments");
  CumulativeOrder ord((size_t)p);
  for (int i = 0; i <= upto; ++i) ord.next(i);
  std::copy(ord.current().begin(), ord.current().end(), order);
  return BWGR_OK;
}

// The member's start values, as the reference sets them before its loop, from what the call has read: the member's parameter, df, R2, vy =
// fvar(y), sumvx = vx.sum() and, for emBL, emEN and the lasso, the columns' squared norms xxh on the host.
static EmState em_start(int model, float par, float df, float R2, float vy, float sumvx, int64_t p, const std::vector<float> &xxh) {
  const bool lasso = (model == BWGR_EM_LASSO);
  EmState h; memset(&h, 0, sizeof(h));
  h.df = df; h.vy = vy; h.MSx = sumvx; h.sumvx = sumvx; h.R2 = R2; h.ve = 1.0f;
  if (model == BWGR_EM_BA || model == BWGR_EM_BB) {
    h.ve = 1;                                                                        // :84, :135
    if (model == BWGR_EM_BB) {
      float Pi = par; if (Pi > 0.5f) Pi = 1 - Pi;                                    // :141
      h.Pi = Pi; h.MSx = sumvx * Pi;                                                 // :147
      h.Pi0 = (1 - Pi) / Pi;                                                         // :154
    }
    h.Sb = R2 * (df + 2) * vy / h.MSx;                                               // :96, :148
    h.Se = (1 - R2) * (df + 2) * vy;                                                 // :97, :149
  } else if (model == BWGR_EM_RR) {
    h.Lmb = sumvx;                                                                   // :319
    h.Rho = sumvx * (1 - R2) / R2;                                                   // :320
    h.ve = 0.5f * vy;                                                                // :322
    h.vb = h.ve / sumvx;                                                             // :323
    h.Se = (1 - R2) * (df + 2) * vy;                                                 // :324
    h.Sb = R2 * (df + 2) * vy / sumvx;                                               // :325
  } else if (model == BWGR_EM_DE) {
    h.cxx = sumvx * (1 - R2) / R2;                                                   // :265
  } else if (model == BWGR_EM_ML) {
    h.Lmb = sumvx;                                                                   // :486
  } else if (model == BWGR_EM_BC || model == BWGR_EM_BCPI) {
    float Pi = par; if (Pi > 0.5f) Pi = 1 - Pi;                                      // :197, :1508
    h.Pi = Pi; h.PriorPi = Pi;                                                       // :1511
    h.MSx = sumvx * Pi * (1 - Pi);                                                   // :203, :1512
    h.Sa = R2 * (df + 2) * vy / h.MSx;                                               // :204
    h.Se = (1 - R2) * (df + 2) * vy;                                                 // :205
    h.ve = h.Sa; h.va = h.Se; h.Lmb = h.ve / h.va;                                   // :209-211 (sic)
    h.Pi0 = (1 - Pi) / Pi;                                                           // :213
  } else if (model == BWGR_EM_BL || model == BWGR_EM_EN || lasso) {
    h.alpha = par;
    if (lasso) {
      double sx = 0; for (int64_t j = 0; j < p; ++j) sx += (double)xxh[(size_t)j];
      h.Lmb1 = (float)(sx / (double)p) / (float)p;                                   // Lmb = xx.mean()/p, :1472
    } else if (model == BWGR_EM_BL) {
      double sx = 0; for (int64_t j = 0; j < p; ++j) sx += (double)xxh[(size_t)j];
      h.cxx = (float)(sx / (double)p);                                               // xx.mean(), :368
      const float hh = R2;                                                           // h2 = R2, :359
      h.Lmb1 = h.cxx * ((1 - hh) / hh) * h.alpha * 0.5f;                             // :369
      h.Lmb2 = h.cxx * ((1 - hh) / hh) * (1 - h.alpha);                              // :370
    } else {
      h.cxx = sumvx * (1 - R2) / R2;                                                 // :412
      h.Sy = sqrtf(vy);                                                              // :414
      h.Lmb = h.cxx;                                                                 // :415
      h.Lmb1 = 0.5f * h.Lmb * h.alpha * h.Sy;                                        // :416
      h.Lmb2 = h.Lmb * (1 - h.alpha);                                                // :417
      float tr = 0; for (int64_t k = 0; k < p; ++k) tr += 1.0f / (xxh[(size_t)k] + h.Lmb);   // the reference's own float loop, :418-419
      h.trAC22 = tr;
    }
  }
  return h;
}

// After the last sweep: the fitted values into hatd (n floats on the device) and the member's h2 into *h2_out.  h: the state the last tail
// left; yd, ed, bd, vbd: y, the residual, b and the per-marker variances on the device; y: the caller's.
static int em_fit_h2(bwgr_panel *P, int model, const EmState &h, const float *y, float vy, const float *yd, const double *ed, const float *bd,
                     const float *vbd, float *hatd, float *h2_out) {
  const bool lasso = (model == BWGR_EM_LASSO);
  const int64_t p = P->data->p, n = P->data->n;
  hipStream_t st = P->stream;
  float h2;
  if (model == BWGR_EM_ML) {
    hipLaunchKernelGGL(k_em_fit_ml, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, yd, ed, hatd, (int)n);
    h2 = h.vb * h.MSx / (h.vb * h.MSx + h.ve);                                       // :513
  } else if (lasso) {
    hipLaunchKernelGGL(k_em_fit_ml, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, yd, ed, hatd, (int)n);   // fit = y - e, :1493
    std::vector<double> eh((size_t)n);
    HIPCHK(d2h(st, eh.data(), ed, sizeof(double) * n));
    double s = 0; for (int64_t k = 0; k < n; ++k) s = fma(eh[(size_t)k], (double)y[k], s);
    h2 = 1.0f - ((float)s / (float)(n - 1)) / vy;                                    // :1494
  } else {
    CHK(gemv_hat<float>(P, bd, h.mu, hatd, "em"));                                   // fit = gen*b + mu, :120-121
    if (model == BWGR_EM_DE) {                                                       // h2 = Vb.sum()/(Vb.sum()+Ve), :304
      float sv = 0;
      CHK(sum_floats(st, {{vbd, p, &sv}}, "em"));
      h2 = sv / (sv + h.ve);
    } else if (model == BWGR_EM_BL) {                                                // h2 = 1 - fvar(e)/fvar(y), :396
      std::vector<double> eh((size_t)n);
      HIPCHK(d2h(st, eh.data(), ed, sizeof(double) * n));
      double s = 0; for (int64_t k = 0; k < n; ++k) s += (double)(float)eh[(size_t)k];
      const float m = (float)(s / (double)n);
      double sv = 0; for (int64_t k = 0; k < n; ++k) { const float dev = (float)eh[(size_t)k] - m; const float sq = dev * dev; sv += (double)sq; }
      h2 = 1 - (float)(sv / (double)(float)(n - 1)) / vy;
    } else if (model == BWGR_EM_EN) h2 = h.va * h.cxx / (h.va * h.cxx + h.ve);       // :459
    else h2 = 1 - h.ve / vy;                                                         // :119, :178, :237, :344, :1542
  }
  HIPCHK(hipGetLastError());
  *h2_out = h2;
  return BWGR_OK;
}

// scal[0..5]: the member's variance components as the reference's return list names them (include/bwgr.h)
static void em_scal(int model, const EmState &h, float h2, float *scal) {
  for (int k = 0; k < 6; ++k) scal[k] = 0.0f;
  scal[1] = h.ve; scal[2] = h2;
  if (model == BWGR_EM_RR || model == BWGR_EM_ML) scal[0] = h.vb;
  if (model == BWGR_EM_ML) scal[3] = h.vb * h.MSx;                                   // Va = vb*MSx, :519
  if (model == BWGR_EM_BC || model == BWGR_EM_BCPI) { scal[0] = h.va; scal[3] = h.va * h.MSx; }   // Va, Vg = va*MSx, :243, :1547
  if (model == BWGR_EM_BCPI) scal[4] = h.Pi;
  if (model == BWGR_EM_EN) scal[0] = h.va * h.cxx;                                   // :457
  if (model == BWGR_EM_BL) scal[1] = 0.0f;
  if (model == BWGR_EM_LASSO) { scal[0] = h.Lmb1; scal[1] = 0.0f; }                  // Lmb, :1497
}

extern "C" int bwgr_em(bwgr_panel *P, int model, const float *y, float df, float R2, float par, const float *D, int maxit_in,
                       float *mu, float *b, float *d, float *hat, float *vbvec, float *scal, int *iters) {
  // ---- set-up: the arguments, the scratch panel, the call's arrays, the start values ----
  if (P && P->data->cen) return refuse_centred("em");
  if (!P || !y || !b || !scal) return fail(BWGR_EINVAL, "em: null pointer");
  if (model < BWGR_EM_RR || model > BWGR_EM_LASSO) return fail(BWGR_EINVAL, "em: bad model %d", model);
  if (D && model != BWGR_EM_ML) return fail(BWGR_EINVAL, "em: marker weights D belong to emML only");
  const bool soft = (model == BWGR_EM_BB || model == BWGR_EM_BC || model == BWGR_EM_BCPI);
  const bool lasso = (model == BWGR_EM_LASSO);
  const bool nonaffine = soft || lasso || model == BWGR_EM_BL || model == BWGR_EM_EN;
  if (nonaffine && !P->data->plan.pipelined) return fail(BWGR_EINVAL, "em: this member needs the pipelined sweep engine (k_sweep2), which this panel's geometry does not fit");
  HIPCHK(hipSetDevice(P->data->device));
  const int64_t p = P->data->p, n = P->data->n;
  const bool conv = (model == BWGR_EM_DE || model == BWGR_EM_ML || model == BWGR_EM_EN || lasso);
  const bool shuffled = (model != BWGR_EM_BCPI && !lasso);                            // emBCpi and lasso sweep in natural order, :1523, :1476
  const int maxit = maxit_in > 0 ? maxit_in : (conv ? 300 : 200);                     // :81, :251, :309, :401, :465
  const float tol = (model == BWGR_EM_DE) ? 10e-6f : (model == BWGR_EM_EN) ? 10e-11f : 10e-8f;   // :252, :402, :466
  hipStream_t st = P->stream;
  // scratch panel: same geometry, its own X and Gram; only the diagonal and distance-1 blocks are ever built (lag 2, 32-bit staging)
  bwgr_panel *Q = nullptr;
  Guard drop([&] { bwgr_panel_destroy(Q); });
  CumulativeOrder cum((size_t)p);
  std::vector<int> order = cum.current(), order_next;   // (copied from asynchronously: declared before the holder, which waits for the stream)
  DevBufs bufs(st);
  if (shuffled) {
    CHK(scratch_panel_alloc(&Q, P, n, P->data->plan.K, PANEL_EM));
    if (Q->data->plan.K != P->data->plan.K || Q->data->plan.R != P->data->plan.R || Q->data->plan.m != P->data->plan.m || Q->data->plan.pipelined != P->data->plan.pipelined) return fail(BWGR_EINVAL, "em: scratch panel geometry differs");
    CHK(scratch_alloc(Q));
  }
  bwgr_panel *S = Q ? Q : P;                                                          // the panel the sweeps run on
  const size_t np = (size_t)p, pb = sizeof(float) * np;
  float *yd = bufs.get<float>((size_t)n), *bd = bufs.get<float>(np), *bcd = bufs.get<float>(np), *dd = bufs.get<float>(np);
  float *lamd = bufs.get<float>(np), *vbd = bufs.get<float>(np), *xxd = bufs.get<float>(np);
  float *bq = bufs.get<float>(np), *xxq = bufs.get<float>(np), *lamq = bufs.get<float>(np), *dq = bufs.get<float>(np), *vq = bufs.get<float>(np);
  double *ed = bufs.get<double>((size_t)P->data->plan.ld); int32_t *ordd = bufs.get<int32_t>(np);
  EmState *std_ = bufs.get<EmState>(1); ChainScalars *sc = bufs.get<ChainScalars>(1);
  float *hatd = bufs.get<float>((size_t)n), *Dd = D ? bufs.get<float>(np) : nullptr;
  if (bufs.failed()) return no_memory("em");
  if (D) HIPCHK(h2d(st, Dd, D, np));
  HIPCHK(h2d(st, yd, y, (size_t)n));
  HIPCHK(zero(st, bd, np)); HIPCHK(zero(st, dd, np));
  HIPCHK(d2d(st, xxd, P->data->xx, np));
  // vy = fvar(y) with the library's reduction (float result of fp64 sums, like the fused samplers' setup)
  float vy = 0;
  {
    InitArgs ia; memset(&ia, 0, sizeof(ia));
    ChainScalars h0; memset(&h0, 0, sizeof(h0));
    HIPCHK(h2d(st, sc, &h0, 1));
    ia.y = yd; ia.e = ed; ia.n = (int)n; ia.p = (int)p; ia.ld = P->data->plan.ld; ia.model = BWGR_BAYESRR; ia.pi = 0; ia.df = df; ia.R2 = R2; ia.MSx = P->data->MSx; ia.sc = sc;
    hipLaunchKernelGGL(k_chain_init, dim3(1), dim3(1024), 0, st, ia);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, &h0, sc, sizeof(h0)));
    vy = h0.vy;
  }
  const float sumvx = P->data->MSx;                                                        // vx.sum()
  std::vector<float> hostv, xxh, yxh, bh;
  auto fill = [&](float *dst, float v) { hostv.assign((size_t)p, v); hipError_t e_ = h2d(st, dst, hostv.data(), np); return e_ != hipSuccess ? e_ : hipStreamSynchronize(st); };
  if (model == BWGR_EM_BL || model == BWGR_EM_EN || lasso) {
    xxh.resize((size_t)p);
    HIPCHK(d2h(st, xxh.data(), xxd, pb));
  }
  EmState h = em_start(model, par, df, R2, vy, sumvx, p, xxh);
  if (model == BWGR_EM_BA || model == BWGR_EM_BB) {
    HIPCHK(fill(lamd, 1.0f)); HIPCHK(fill(vbd, 1.0f));                               // vb = 1, Lmb = ve * vb^-1 = 1, :87-88
  } else if (model == BWGR_EM_DE) {
    hipLaunchKernelGGL(k_em_fix_xx, dim3(1024), dim3(256), 0, st, xxd, p);           // :261
    HIPCHK(fill(lamd, (float)p + h.cxx));                                            // :269
  }
  HIPCHK(h2d(st, std_, &h, 1));
  hipLaunchKernelGGL(k_em_init, dim3(1), dim3(1024), 0, st, yd, ed, (int)n, P->data->plan.ld, std_);   // mu, e (overwrites k_chain_init's e)
  HIPCHK(hipGetLastError());
  {
    ChainScalars h0; memset(&h0, 0, sizeof(h0));
    h0.ve = 1.0f; h0.pi = 0.0f; h0.dfp1 = 1.0f;                                      // the sweep's variates are switched off
    h0.C = -0.5f / sqrtf(h.ve);                                                      // :157, :216, :1522
    h0.odds = h.Pi0; h0.lam = h.Lmb1; h0.Sb = h.cxx;                                 // Pi0; Lmb1; emBL's cxx (k_prestage)
    HIPCHK(h2d(st, sc, &h0, 1));
  }
  if (shuffled) order = cum.next(0);                                                  // sweep 0's order
  if (!shuffled) HIPCHK(h2d(st, ordd, order.data(), np));
  const int cps = (int)((size_t)P->data->plan.R * (P->data->is_f32 ? 4 : 1) / 16);
  uint32_t flags = SWF_LAM_VEC;
  if (model == BWGR_EM_BA) flags |= SWF_DELTA2;
  if (soft) flags |= SWF_EM_SEL;
  if (model == BWGR_EM_EN) flags |= SWF_EM_EN;
  if (model == BWGR_EM_BL) flags |= SWF_EM_BL;
  if (lasso) flags |= SWF_EM_LASSO;
  int numit = 0;
  const bool emdbg = P->data->sw.em_debug;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  // ---- the sweeps ----
  for (int i = 0; i < maxit; ++i) {
    const double t_0 = now();
    if (shuffled) {
      // order = sweep i's marker order.  std::shuffle(order.begin(), order.end(), std::mt19937(i)) -- :103, :277, :331, :491 ...,
      // the reference's own call -- was made for sweep 0 before the loop and is made for sweep i+1 below, while the GPU
      // runs sweep i (10-15 ms of host time per sweep at p = 10^6)
      HIPCHK(h2d(st, ordd, order.data(), np));
      hipLaunchKernelGGL(k_permute_cols, dim3(8192), dim3(256), 0, st, (const uint4 *)P->data->X, (uint4 *)Q->data->X, ordd, p, P->data->plan.K, cps);
    }
    if (conv) HIPCHK(d2d(st, bcd, bd, np));                           // bc = b
    hipLaunchKernelGGL(k_em_stage, dim3(1024), dim3(256), 0, st, ordd, p, model, D ? 1 : 0, bd, xxd, lamd, Dd, std_, bq, xxq, lamq);
    HIPCHK(hipGetLastError());
    if (shuffled) CHK(panel_build_gram(Q));
    SweepArgs a = sweep_args(S, (int)flags, ed, bq, dq, vq, xxq, lamq, sc, (uint32_t)i, make_rng(0, BWGR_RNG_DEGENERATE));
    CHK(launch_sweep(S, a));
    hipLaunchKernelGGL(k_em_unstage, dim3(1024), dim3(256), 0, st, ordd, p, bq, bd, (soft || lasso) ? dq : nullptr, (soft || lasso) ? dd : nullptr);
    EmTailArgs t; t.model = model; t.n = (int)n; t.conv = conv ? 1 : 0; t.p = p; t.e = ed; t.y = yd; t.b = bd; t.bc = bcd; t.d = dd;
    t.lam = lamd; t.vbv = vbd; t.xx = xxd; t.st = std_; t.sc = sc;
    hipLaunchKernelGGL(k_em_tail, dim3(1), dim3(1024), 0, st, t);
    HIPCHK(hipGetLastError());
    ++numit;
    const double t_1 = now();
    if (shuffled && i + 1 < maxit) order_next = cum.next(i + 1);
    const double t_2 = now();
    // the convergence test needs cnv (and the sweep's status word)
    ChainScalars hc;
    HIPCHK(hipMemcpyAsync(&h, std_, sizeof(h), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&hc, sc, sizeof(hc), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (emdbg) fprintf(stderr, "em sweep %d: launches %.2f ms, host shuffle %.2f ms, wait %.2f ms\n", i, t_1 - t_0, t_2 - t_1, now() - t_2);
    if (hc.error) return sweep_error(hc.error, "em");
    if (lasso) {   // Lmb from the sweep's yx and b: the reference's own sequential float loop, :1487-1490
      yxh.resize((size_t)p); bh.resize((size_t)p);
      HIPCHK(d2h(st, yxh.data(), dd, pb)); HIPCHK(d2h(st, bh.data(), bd, pb));
      float tmp = 0.0f;
      for (int64_t j = 0; j < p; ++j) tmp += fabsf(yxh[(size_t)j]) - fabsf(bh[(size_t)j] * xxh[(size_t)j]);
      float L = 2.0f * tmp / (float)p;
      L = 2.0f * sqrtf(fabsf(L));
      h.Lmb1 = L;
      HIPCHK(h2d(st, std_, &h, 1));
      HIPCHK(h2d(st, &sc->lam, &h.Lmb1, 1));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (conv && h.cnv < tol) break;                                                  // :296, :452, :510, :1492
    if (shuffled) order.swap(order_next);
  }
  // ---- results ----
  float h2;
  CHK(em_fit_h2(P, model, h, y, vy, yd, ed, bd, vbd, hatd, &h2));
  if (mu) *mu = h.mu;
  HIPCHK(d2h(st, b, bd, pb));
  if (d && soft) HIPCHK(d2h(st, d, dd, pb));
  if (hat) HIPCHK(d2h(st, hat, hatd, sizeof(float) * n));
  if (vbvec && (model == BWGR_EM_BA || model == BWGR_EM_DE || model == BWGR_EM_BB)) HIPCHK(d2h(st, vbvec, vbd, pb));
  em_scal(model, h, h2, scal);
  if (iters) *iters = numit;
  return BWGR_OK;
}
