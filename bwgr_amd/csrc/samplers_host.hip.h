// bwgr_amd/csrc/samplers_host.hip.h -- the host entries of the float samplers: KMUP / KMUP2, the fused chains (bwgr_chain_*), bwgr_bayes and
// the two-panel bwgr_bayes2.  Part of bwgr_hip.hip, which includes it after everything it uses (fail, HIPCHK, DevBufs, no_memory, d2h / h2d /
// zero, Guard, sum_floats, sweep_args, launch_sweep and the sweep's planning and launching, the scratch panels, launch_gather_rows, gemv_hat,
// g_last_redo); it defines no kernel: theirs are chain.hip.h and panel.hip.h.  A chain times its sweeps between the event pairs of its pool
// (bwgr_chain::timing, the holder's events): a sweep takes the next pair and commits it once its launches stand; bwgr_chain_sweep_ms, or a full pool, reads them and rewinds.
// ------------------------------------------------------------------------------------------------
// KMUP
// ------------------------------------------------------------------------------------------------
// one sweep over panel PS with host-side b, d, xx, L and a device residual e64 (ld doubles, padding zero); KMUP and KMUP2
static int kmup_sweep(bwgr_panel *PS, float *b, float *d, const float *xx, const float *L, double *e64, float Ve, float pi, float bg,
                      int kmup2, uint64_t seed, uint32_t iter, int rng_mode, const char *who) {
  DevBufs bufs;
  const size_t p = (size_t)PS->data->p, pb = sizeof(float) * p;
  float *db = bufs.get<float>(p), *dd = bufs.get<float>(p), *dxx = bufs.get<float>(p), *dL = bufs.get<float>(p), *dvb = bufs.get<float>(p);
  ChainScalars *sc = bufs.get<ChainScalars>(1);
  if (bufs.failed()) return no_memory(who);
  HIPCHK(h2d(PS->stream, db, b, p));
  HIPCHK(h2d(PS->stream, dd, d, p));
  HIPCHK(h2d(PS->stream, dxx, xx, p));
  HIPCHK(h2d(PS->stream, dL, L, p));
  ChainScalars h; memset(&h, 0, sizeof(h));
  h.ve = Ve; h.pi = pi; h.C = -0.5f / sqrtf(Ve); h.odds = pi / (1.0f - pi); h.dfp1 = 1.0f; h.bg = bg;
  h.inc_rate = 1.0f - pi;
  HIPCHK(h2d(PS->stream, sc, &h, 1));
  SweepArgs a = sweep_args(PS, SWF_LAM_VEC | (pi > 0 ? (SWF_SELECT | SWF_ALT_B2) : 0) | (kmup2 ? SWF_KMUP2 : 0), e64, db, dd, dvb, dxx, dL, sc, iter,
                           make_rng(seed, rng_mode));
  CHK(launch_sweep(PS, a));
  HIPCHK(hipMemcpyAsync(b, db, pb, hipMemcpyDeviceToHost, PS->stream));
  HIPCHK(hipMemcpyAsync(d, dd, pb, hipMemcpyDeviceToHost, PS->stream));
  HIPCHK(hipMemcpyAsync(&h, sc, sizeof(h), hipMemcpyDeviceToHost, PS->stream));
  HIPCHK(hipStreamSynchronize(PS->stream));
  g_last_redo = (int)h.nredo;
  if (h.error) return sweep_error(h.error, who);
  return BWGR_OK;
}

extern "C" int bwgr_kmup(bwgr_panel *P, float *b, float *d, const float *xx, float *e, const float *L, float Ve,
                         float pi, uint64_t seed, uint32_t iter, int rng_mode) {
  if (P && P->data->cen) return refuse_centred("kmup");
  if (!P || !b || !d || !xx || !e || !L) return fail(BWGR_EINVAL, "kmup: null pointer");
  HIPCHK(hipSetDevice(P->data->device));
  DevBufs bufs;
  float *de = bufs.get<float>((size_t)P->data->n);
  double *de64 = bufs.get<double>((size_t)P->data->plan.ld);
  if (bufs.failed()) return no_memory("kmup");
  HIPCHK(h2d(P->stream, de, e, (size_t)P->data->n));
  hipLaunchKernelGGL(k_f2d, dim3(64), dim3(256), 0, P->stream, de, de64, P->data->n, P->data->plan.ld);
  CHK(kmup_sweep(P, b, d, xx, L, de64, Ve, pi, 0.0f, 0, seed, iter, rng_mode, "kmup"));
  hipLaunchKernelGGL(k_d2f, dim3(64), dim3(256), 0, P->stream, de64, de, P->data->n);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(P->stream, e, de, sizeof(float) * P->data->n));
  return BWGR_OK;
}

// KMUP2(X,Use,b,d,xx,E,L,Ve,pi), src/Rcpp20260726ai.cpp:41-77: the sweep on the row subsample Use (0-based, nuse entries, in
// the caller's order, repeats allowed) of the resident panel.  The rows are gathered into a subsample panel on the device, its
// Gram blocks built, and the sweep runs with KMUP2's conditional mean (numerator + b0, denominator xx*bg + L, bg = n0/nuse).
// e_out receives the nuse residuals of the subsample (:76); E (n0 entries) is not modified.
extern "C" int bwgr_kmup2(bwgr_panel *P, const int *Use, int64_t nuse, float *b, float *d, const float *xx, const float *E,
                          float *e_out, const float *L, float Ve, float pi, uint64_t seed, uint32_t iter, int rng_mode) {
  if (P && P->data->cen) return refuse_centred("kmup2");
  if (!P || !Use || !b || !d || !xx || !E || !e_out || !L) return fail(BWGR_EINVAL, "kmup2: null pointer");
  if (nuse < 2 || nuse > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "kmup2: need 2 <= length(Use) < 2^31 (got %lld)", (long long)nuse);
  for (int64_t k = 0; k < nuse; ++k)
    if (Use[k] < 0 || Use[k] >= P->data->n) return fail(BWGR_EINVAL, "kmup2: Use[%lld] = %d is outside 0..%lld", (long long)k, Use[k], (long long)P->data->n - 1);
  HIPCHK(hipSetDevice(P->data->device));
  bwgr_panel *PB = nullptr;
  CHK(scratch_panel_alloc(&PB, P, nuse, 0, PANEL_ROWS));
  Guard drop([&] { bwgr_panel_destroy(PB); });
  CHK(scratch_alloc(PB));
  DevBufs bufs;
  int *use_d = bufs.get<int>((size_t)nuse);
  float *dE = bufs.get<float>((size_t)P->data->n), *deo = bufs.get<float>((size_t)nuse);
  double *dE64 = bufs.get<double>((size_t)P->data->n), *e64 = bufs.get<double>((size_t)PB->data->plan.ld);
  if (bufs.failed()) return no_memory("kmup2");
  HIPCHK(h2d(P->stream, use_d, Use, (size_t)nuse));
  HIPCHK(h2d(P->stream, dE, E, (size_t)P->data->n));
  launch_gather_rows(P, PB, use_d, nuse);
  HIPCHK(hipGetLastError());
  CHK(panel_build_gram(PB));
  hipLaunchKernelGGL(k_f2d, dim3(64), dim3(256), 0, P->stream, dE, dE64, P->data->n, P->data->n);
  hipLaunchKernelGGL(k_gather_e, dim3(64), dim3(256), 0, P->stream, dE64, use_d, (int)nuse, PB->data->plan.ld, e64);   // e0[k] = E[Use[k]], :49-53
  HIPCHK(hipGetLastError());
  CHK(kmup_sweep(PB, b, d, xx, L, e64, Ve, pi, (float)P->data->n / (float)nuse, 1, seed, iter, rng_mode, "kmup2"));
  hipLaunchKernelGGL(k_d2f, dim3(64), dim3(256), 0, P->stream, e64, deo, nuse);
  HIPCHK(hipGetLastError());
  HIPCHK(d2h(P->stream, e_out, deo, sizeof(float) * (size_t)nuse));
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// fused chains
// ------------------------------------------------------------------------------------------------
static bool per_marker_vb(int model) { return model == BWGR_BAYESA || model == BWGR_BAYESB || model == BWGR_BAYESL || model == BWGR_BAYESDPI; }
static bool has_d(int model) { return model == BWGR_BAYESB || model == BWGR_BAYESC || model == BWGR_BAYESCPI || model == BWGR_BAYESDPI; }

extern "C" int bwgr_chain_destroy(bwgr_chain *C) {
  if (!C) return BWGR_OK;
  if (C->P && C->P->ps_owner == C) C->P->ps_owner = nullptr;   // (a later chain may be allocated at this address)
  if (C->P) C->P->draws.forget(C->sc);                         // ... and so may its scalars: variates drawn ahead for this chain are nobody's now
  if (C->P) { C->P->nchains--; C->P->data->nchains_all--; (void)hipSetDevice(C->P->data->device); }
  delete C;   // (the state arrays and the timing pairs' events: the holder's)
  return BWGR_OK;
}

extern "C" int bwgr_chain_create_sharded(bwgr_chain **out, bwgr_panel *P, int model, const float *y, int memloc, float it,
                                         float bi, float pi, float df, float R2, uint64_t seed, int rng_mode, int64_t marker0,
                                         int64_t p_total, float MSx_total, double *e_ext) {
  if (!out || !P || !y) return fail(BWGR_EINVAL, "chain_create: null pointer");
  *out = nullptr;
  if (model < BWGR_BAYESA || model > BWGR_BAYESDPI) return fail(BWGR_EINVAL, "chain_create: bad model %d", model);
  if (marker0 < 0 || p_total < marker0 + P->data->p || p_total > 0xFFFFFFF0ll) return fail(BWGR_EINVAL, "chain_create: bad shard [%lld,+%lld) of %lld", (long long)marker0, (long long)P->data->p, (long long)p_total);
  HIPCHK(hipSetDevice(P->data->device));
  if (P->data->cen) {
    if (!has_d(model) || !P->data->e3_ready)
      return fail(BWGR_EINVAL, "chain_create: an implicitly centred panel (bwgr_panel_set_centred) runs the selection models BayesB / C / Cpi / Dpi only");
    if (!P->cpre) CHK(own_array(P->own, P->cpre, (size_t)P->data->plan.nblocks + 1, "chain_create"));
  }
  bwgr_chain *C = new bwgr_chain();
  C->P = P; P->nchains++; P->data->nchains_all++; C->model = model; C->itf = it; C->bif = bi; C->iit = (int)it; C->ibi = (int)bi;
  C->pi = pi; C->df = df; C->R2 = R2; C->seed = seed; C->rng_mode = rng_mode;
  C->marker0 = marker0; C->p_total = p_total; C->MSx_eff = MSx_total;
  C->Phi = MSx_total * (1 - R2) / R2;
  Guard drop([&] { bwgr_chain_destroy(C); });
  const size_t pb = sizeof(float) * P->data->p;
  if (!C->own.take({{&C->y, sizeof(float) * P->data->n}, {&C->b, pb}, {&C->d, pb}, {&C->vb, pb}, {&C->lam, pb}, {&C->B, pb}, {&C->D, pb}, {&C->VB, pb}, {&C->sc, sizeof(ChainScalars)}}))
    return no_memory("chain_create");
  if (e_ext) C->e = e_ext;   // (borrowed)
  else CHK(own_array(C->own, C->e, (size_t)P->data->plan.ld, "chain_create"));
  HIPCHK(memloc == BWGR_DEVICE ? d2d(P->stream, C->y, y, (size_t)P->data->n) : h2d(P->stream, C->y, y, (size_t)P->data->n));
  InitArgs ia; ia.y = C->y; ia.e = C->e; ia.n = (int)P->data->n; ia.p = (int)P->data->p; ia.ld = P->data->plan.ld; ia.model = model;
  ia.pi = pi; ia.df = df; ia.R2 = R2; ia.MSx = MSx_total; ia.sc = C->sc;
  hipLaunchKernelGGL(k_chain_init, dim3(1), dim3(1024), 0, P->stream, ia);
  hipLaunchKernelGGL(k_marker_init, dim3(1024), dim3(256), 0, P->stream, C->b, C->d, C->vb, C->lam, C->B, C->D, C->VB, (int)P->data->p, C->sc);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(P->stream));
  drop.release();
  *out = C;
  return BWGR_OK;
}

extern "C" int bwgr_chain_create(bwgr_chain **out, bwgr_panel *P, int model, const float *y, int memloc, float it,
                                 float bi, float pi, float df, float R2, uint64_t seed, int rng_mode) {
  if (!P) return fail(BWGR_EINVAL, "chain_create: null pointer");
  return bwgr_chain_create_sharded(out, P, model, y, memloc, it, bi, pi, df, R2, seed, rng_mode, 0, P->data->p, P->data->MSx, nullptr);
}

static void chain_args(const bwgr_chain *C, int blk_begin, int blk_end, SweepArgs &a) {
  const bwgr_panel *P = C->P;
  const int model = C->model;
  int fl = 0;
  if (has_d(model)) fl |= SWF_SELECT;
  if (model == BWGR_BAYESDPI) fl |= SWF_ALT_B2 | SWF_MH;
  if (per_marker_vb(model)) fl |= SWF_LAM_VEC | SWF_VB_VEC;
  a = sweep_args(P, fl | C->flags_extra, C->e, C->b, C->d, C->vb, P->data->xx, C->lam, C->sc, (uint32_t)C->done, make_rng(C->seed, C->rng_mode));
  a.blk_begin = blk_begin; a.blk_end = blk_end; a.marker0 = (uint32_t)C->marker0;
  if (P->data->cen) {   // implicitly centred columns: the centred squared norms, the column sums, this handle's running block sums
    a.flags |= SWF_CENTRE; a.xx = P->data->xxc; a.csum = P->data->csum; a.cpre = P->cpre; a.ninv = 1.0 / (double)P->data->n;
  }
}

extern "C" int bwgr_chain_sweep_blocks(bwgr_chain *C, int blk_begin, int blk_end) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  bwgr_panel *P = C->P;
  if (blk_begin < 0 || blk_end > P->data->plan.nblocks || blk_begin >= blk_end) return fail(BWGR_EINVAL, "sweep_blocks: bad range [%d,%d) of %lld", blk_begin, blk_end, (long long)P->data->plan.nblocks);
  if (C->done >= C->iit) return fail(BWGR_EINVAL, "sweep_blocks: all %d iterations already run", C->iit);
  HIPCHK(hipSetDevice(P->data->device));
  SweepArgs a;
  chain_args(C, blk_begin, blk_end, a);
  SweepTrain t; t.P[0] = P; t.a[0] = &a;
  CHK(train_begin(t));
  if (!C->timing.next(C->own, &t.ev[0][0], &t.ev[0][1])) return fail(BWGR_EHIP, "sweep_blocks: no event pair for the sweep's timing");
  // the per-marker constants and speculative terms of an iteration depend on the state at its start only (a block's b is
  // untouched until the block is swept), so a chain that sweeps its panel in several ranges -- the exchange rounds of the
  // marker-sharded sampler -- pre-stages all of them with the first range
  bool prestaged = false;
  if (P->ps_owner != C || P->ps_iter != C->done) {
    SweepArgs all = a; all.blk_begin = 0; all.blk_end = (int)P->data->plan.nblocks;
    launch_prestage(P, all, t.pl[0]);
    P->ps_owner = C; P->ps_iter = C->done;
    prestaged = true;
  }
  t.draws_next = prestaged && C->done + 1 < C->iit;   // the next iteration's variates, beside this sweep
  const hipError_t he = train_launch(t);
  if (he != hipSuccess) return fail(BWGR_EHIP, "sweep_blocks: %s", hipGetErrorString(he));   // (the pair, not committed, is the next sweep's)
  train_end(t);
  C->timing.commit();
  if (C->timing.full()) CHK(bwgr_chain_sweep_ms(C, nullptr, nullptr));   // fold: the pool's pairs are read and handed out again
  return BWGR_OK;
}

// One exchange round of the marker-sharded sampler in two calls (the same steps a caller can take with sweep_blocks and
// its own vector arithmetic; here they cost two small launches instead of three framework operations per round):
//   round_sweep: remember e, sweep the blocks [blk_begin, blk_end) (an empty range sweeps nothing), delta = e - e_before
//   <caller: all-reduce(sum) delta over the ranks>
//   round_apply: e = e_before + delta
// delta_dev: ld doubles on the chain's device (the panel's padded row count).
extern "C" int bwgr_chain_round_sweep(bwgr_chain *C, int blk_begin, int blk_end, double *delta_dev) {
  if (!C || !delta_dev) return fail(BWGR_EINVAL, "round_sweep: null pointer");
  bwgr_panel *P = C->P;
  HIPCHK(hipSetDevice(P->data->device));
  if (!C->e0) CHK(own_array(C->own, C->e0, (size_t)P->data->plan.ld, "round_sweep"));
  HIPCHK(d2d(P->stream, C->e0, C->e, (size_t)P->data->plan.ld));
  if (blk_begin < blk_end) CHK(bwgr_chain_sweep_blocks(C, blk_begin, blk_end));
  hipLaunchKernelGGL(k_round_delta, dim3(64), dim3(256), 0, P->stream, C->e, C->e0, delta_dev, P->data->plan.ld);
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}
extern "C" int bwgr_chain_round_apply(bwgr_chain *C, const double *delta_dev) {
  if (!C || !delta_dev) return fail(BWGR_EINVAL, "round_apply: null pointer");
  if (!C->e0) return fail(BWGR_EINVAL, "round_apply: no round_sweep before it");
  bwgr_panel *P = C->P;
  HIPCHK(hipSetDevice(P->data->device));
  hipLaunchKernelGGL(k_round_apply, dim3(64), dim3(256), 0, P->stream, C->e, C->e0, delta_dev, P->data->plan.ld);
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}

extern "C" int bwgr_chain_get_sums(bwgr_chain *C, double sums[2]) {
  if (!C || !sums) return fail(BWGR_EINVAL, "null pointer");
  HIPCHK(hipSetDevice(C->P->data->device));
  ChainScalars h;
  HIPCHK(hipMemcpyAsync(&h, C->sc, sizeof(h), hipMemcpyDeviceToHost, C->P->stream));
  HIPCHK(hipStreamSynchronize(C->P->stream));
  if (h.error) return sweep_error(h.error, "chain");
  sums[0] = h.sum_d; sums[1] = h.sum_b2;
  return BWGR_OK;
}

extern "C" int bwgr_chain_end_iteration(bwgr_chain *C, const double sums_total[2]) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  if (C->done >= C->iit) return fail(BWGR_EINVAL, "end_iteration: all %d iterations already run", C->iit);
  bwgr_panel *P = C->P;
  HIPCHK(hipSetDevice(P->data->device));
  const int model = C->model, i = C->done;
  if (sums_total) hipLaunchKernelGGL(k_set_sums, dim3(1), dim3(1), 0, P->stream, C->sc, sums_total[0], sums_total[1]);
  const int accumulate = (i > C->ibi) ? 1 : 0;   // if(i>ibi), src/Rcpp20260726ai.cpp:624
  TailArgs t; t.e = C->e; t.n = (int)P->data->n; t.p = (int)C->p_total; t.model = model; t.df = C->df; t.R2 = C->R2; t.Phi = C->Phi;
  t.accumulate = accumulate; t.iter = (uint32_t)i; t.rng = make_rng(C->seed, C->rng_mode); t.sc = C->sc;
  hipLaunchKernelGGL(k_tail, dim3(1), dim3(1024), 0, P->stream, t);
  hipLaunchKernelGGL(k_marker_tail, dim3((unsigned)std::min<int64_t>(2048, (P->data->p + 255) / 256)), dim3(256), 0, P->stream,
                     C->b, C->d, C->vb, C->lam, C->B, C->D, C->VB, (int)P->data->p, model, C->Phi, accumulate, C->sc);
  HIPCHK(hipGetLastError());
  C->done++;
  return BWGR_OK;
}

// device-side forms of get_sums / end_iteration(sums_total) for the sharded sampler: the two sums stay on the device (the
// caller all-reduces sums_dev, two doubles, in place), so an iteration needs no host round trip
extern "C" int bwgr_chain_get_sums_dev(bwgr_chain *C, double *sums_dev) {
  if (!C || !sums_dev) return fail(BWGR_EINVAL, "null pointer");
  HIPCHK(hipSetDevice(C->P->data->device));
  hipLaunchKernelGGL(k_get_sums_dev, dim3(1), dim3(1), 0, C->P->stream, C->sc, sums_dev);
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}
extern "C" int bwgr_chain_end_iteration_dev(bwgr_chain *C, const double *sums_total_dev) {
  if (!C || !sums_total_dev) return fail(BWGR_EINVAL, "null pointer");
  HIPCHK(hipSetDevice(C->P->data->device));
  hipLaunchKernelGGL(k_set_sums_dev, dim3(1), dim3(1), 0, C->P->stream, C->sc, sums_total_dev);
  HIPCHK(hipGetLastError());
  return bwgr_chain_end_iteration(C, nullptr);
}

extern "C" int bwgr_chain_run(bwgr_chain *C, int iters) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  if (iters < 0 || C->done + iters > C->iit) return fail(BWGR_EINVAL, "chain_run: %d more iterations would exceed it=%d (done %d)", iters, C->iit, C->done);
  for (int k = 0; k < iters; ++k) {
    CHK(bwgr_chain_sweep_blocks(C, 0, (int)C->P->data->plan.nblocks));
    CHK(bwgr_chain_end_iteration(C, nullptr));
  }
  return BWGR_OK;
}

// Two chains of the same resident panel (C1 on a clone of C0's panel, or the other way round), advanced in lockstep by k_sweep3p: one
// set of streamer workgroups -- one pass over the genotypes -- serves both, each chain keeps its own sequencer.  Selection models on
// panels that have k_sweep3; every sweep of the pair is k_sweep3's (no device-side choice of engine).  Each chain's results are
// bit-identical to a run of its own.  (No reference counterpart: the callers that fit many models on one X -- mcmcCV's loop,
// R/cv.R:113-216 -- are where it plugs in.)
extern "C" int bwgr_chain_run_pair(bwgr_chain *C0, bwgr_chain *C1, int iters) {
  if (C0 && C0->P && C0->P->data->cen) return refuse_centred("chain_run_pair");
  if (!C0 || !C1 || C0 == C1) return fail(BWGR_EINVAL, "chain_run_pair: two distinct chains");
  bwgr_panel *P0 = C0->P, *P1 = C1->P;
  if (P0->data != P1->data || P0 == P1) return fail(BWGR_EINVAL, "chain_run_pair: the chains must sit on two handles (panel and clone) of one resident panel");
  if (iters < 0 || C0->done + iters > C0->iit || C1->done + iters > C1->iit) return fail(BWGR_EINVAL, "chain_run_pair: %d more iterations exceed it", iters);
  SweepArgs t0, t1;
  chain_args(C0, 0, (int)P0->data->plan.nblocks, t0); chain_args(C1, 0, (int)P1->data->plan.nblocks, t1);
  const SweepPlan q0 = plan_sweep(sweep_facts(P0), t0.flags, t0.blk_begin, t0.blk_end, SWEEP_PAIR), q1 = plan_sweep(sweep_facts(P1), t1.flags, t1.blk_begin, t1.blk_end, SWEEP_PAIR);
  if (q0.engine != 3 || q1.engine != 3 || !P0->qsum3 || !P1->qsum3)
    return fail(BWGR_EINVAL, "chain_run_pair: both chains must be selection models on a panel with k_sweep3");
  if (s3p_streamer_lds(P0->data->plan3.R3) > (size_t)160 * 1024) return fail(BWGR_EINVAL, "chain_run_pair: the paired streamers' LDS does not fit");
  HIPCHK(hipSetDevice(P0->data->device));
  // everything of the pair runs on ONE stream, owned by the root panel (it outlives both handles), and both handles move onto it
  // for as long as they run in pairs -- one cross-stream wait each, the first time: a wait per call would sit in a hardware queue
  // that other pairs' streams share, and stall them.  A handle's next sweep alone takes it back (leave_pair_stream).
  // The stream one of the two is on already, else a pair stream that every handle has left, else a new one.
  PanelData *D = P0->data;
  auto is_pair_stream = [&](hipStream_t st) { for (hipStream_t q : D->pair_streams) if (q == st) return true; return false; };
  hipStream_t s0 = nullptr;
  if (is_pair_stream(P0->stream)) s0 = P0->stream;
  else if (is_pair_stream(P1->stream)) s0 = P1->stream;
  for (size_t i = 0; !s0 && i < D->pair_streams.size(); ++i) if (D->pair_users[i] <= 0) s0 = D->pair_streams[i];
  if (!s0) {
    if (!(s0 = D->own.stream(hipStreamNonBlocking, 0))) return fail(BWGR_EHIP, "chain_run_pair: no stream for the pair");
    D->pair_streams.push_back(s0); D->pair_users.push_back(0);
  }
  for (bwgr_panel *PX : {P0, P1}) {
    if (PX->stream == s0) continue;
    HIPCHK(hand_over(PX->own, &PX->handover_ev, s0, PX->stream));
    if (!PX->pre_pair_set) { PX->pre_pair_stream = PX->stream; PX->pre_pair_set = true; }   // (leave_pair_stream takes the handle back)
    pair_stream_count(D, PX->stream, -1); pair_stream_count(D, s0, +1);
    PX->stream = s0;
  }
  // the pair's one launch, resident beside the other streams' sweeps
  int need = 0;
  int rc = sweep_guard(P0, q0, s0, P1, &need);
  for (int k = 0; k < iters && rc == BWGR_OK; ++k) {
    SweepArgs a0, a1;
    chain_args(C0, 0, (int)P0->data->plan.nblocks, a0); chain_args(C1, 0, (int)P1->data->plan.nblocks, a1);
    SweepTrain t; t.n = 2; t.P[0] = P0; t.P[1] = P1; t.a[0] = &a0; t.a[1] = &a1; t.need = need;
    if ((rc = train_begin(t)) != BWGR_OK) break;
    launch_prestage(P0, a0, t.pl[0]); launch_prestage(P1, a1, t.pl[1]);
    P0->ps_owner = C0; P0->ps_iter = C0->done; P1->ps_owner = C1; P1->ps_iter = C1->done;
    if (!C0->timing.next(C0->own, &t.ev[0][0], &t.ev[0][1]) || !C1->timing.next(C1->own, &t.ev[1][0], &t.ev[1][1])) {   // both chains time the launch they share
      rc = fail(BWGR_EHIP, "chain_run_pair: no event pair for the sweep's timing"); break;
    }
    const hipError_t he = train_launch(t);
    if (he != hipSuccess) { rc = fail(BWGR_EHIP, "chain_run_pair: launch failed: %s", hipGetErrorString(he)); break; }
    train_end(t);
    C0->timing.commit(); C1->timing.commit();
    if ((rc = bwgr_chain_end_iteration(C0, nullptr)) != BWGR_OK) break;
    rc = bwgr_chain_end_iteration(C1, nullptr);
    if (C0->timing.full()) (void)bwgr_chain_sweep_ms(C0, nullptr, nullptr);
    if (C1->timing.full()) (void)bwgr_chain_sweep_ms(C1, nullptr, nullptr);
  }
  return rc;
}

extern "C" int bwgr_chain_sync(bwgr_chain *C) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  HIPCHK(hipSetDevice(C->P->data->device));
  HIPCHK(hipStreamSynchronize(C->P->stream));
  ChainScalars h;
  HIPCHK(d2h(C->P->stream, &h, C->sc, sizeof(h)));
  if (h.error) return sweep_error(h.error, "chain");
  return BWGR_OK;
}

extern "C" int bwgr_chain_iterations(const bwgr_chain *C, int *done) {
  if (!C || !done) return fail(BWGR_EINVAL, "null pointer");
  *done = C->done;
  return BWGR_OK;
}

extern "C" int bwgr_chain_sweep_ms(bwgr_chain *C, float *avg_ms, int *launches) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  HIPCHK(hipSetDevice(C->P->data->device));
  HIPCHK(hipStreamSynchronize(C->P->stream));
  Guard rewind([&] { C->timing.rewind(); });   // on a failed read too, which loses this interval's timing and nothing else
  float total = 0; int nl = 0;
  for (size_t k = 0; k < C->timing.used(); ++k) {
    float ms = 0; hipEvent_t e0, e1; C->timing.pair(k, &e0, &e1);
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    total += ms; nl++;
  }
  C->ms_acc += total; C->launch_acc += nl;
  if (avg_ms && launches) {
    *launches = C->launch_acc;
    *avg_ms = C->launch_acc ? C->ms_acc / C->launch_acc : 0.0f;
    C->ms_acc = 0; C->launch_acc = 0;
  }
  return BWGR_OK;
}

extern "C" int bwgr_chain_redo_count(bwgr_chain *C, int *count) {
  if (!C || !count) return fail(BWGR_EINVAL, "null pointer");
  CHK(bwgr_chain_sync(C));
  ChainScalars h;
  HIPCHK(d2h(C->P->stream, &h, C->sc, sizeof(h)));
  *count = (int)h.nredo;
  return BWGR_OK;
}

extern "C" int bwgr_chain_state(bwgr_chain *C, float *b, float *d, float *e, float *vb, float *scal) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  CHK(bwgr_chain_sync(C));
  bwgr_panel *P = C->P;
  const size_t pb = sizeof(float) * P->data->p;
  ChainScalars h;
  HIPCHK(d2h(P->stream, &h, C->sc, sizeof(h)));
  if (b) HIPCHK(d2h(P->stream, b, C->b, pb));
  if (d) HIPCHK(d2h(P->stream, d, C->d, pb));
  if (e) {
    DevBufs bufs;
    float *ef = bufs.get<float>((size_t)P->data->n);
    if (bufs.failed()) return no_memory("chain_state");
    hipLaunchKernelGGL(k_d2f, dim3(64), dim3(256), 0, P->stream, C->e, ef, P->data->n);
    HIPCHK(d2h(P->stream, e, ef, sizeof(float) * P->data->n));
  }
  if (vb) {
    if (per_marker_vb(C->model)) HIPCHK(d2h(P->stream, vb, C->vb, pb));
    else for (int64_t j = 0; j < P->data->p; ++j) vb[j] = h.vb;
  }
  if (scal) { scal[0] = h.mu; scal[1] = h.ve; scal[2] = h.vb; scal[3] = h.pi; }
  return BWGR_OK;
}

extern "C" int bwgr_chain_result(bwgr_chain *C, float *mu, float *b, float *d, float *hat, float *vb, float *ve,
                                 float *h2, float *MSx, float *pi, float *pval) {
  if (!C) return fail(BWGR_EINVAL, "null chain");
  if (C->done != C->iit) return fail(BWGR_EINVAL, "chain_result: %d of %d iterations run", C->done, C->iit);
  CHK(bwgr_chain_sync(C));
  bwgr_panel *P = C->P;
  const size_t pb = sizeof(float) * P->data->p;
  const bool per = per_marker_vb(C->model);
  const float MCMC = C->itf - C->bif;                                              // :626
  DevBufs bufs;
  float *pval_dev = nullptr;
  if (pval) pval_dev = bufs.get<float>((size_t)P->data->p);
  if (bufs.failed()) return no_memory("chain_result");
  if (!C->finalized) {
    hipLaunchKernelGGL(k_final_markers, dim3(1024), dim3(256), 0, P->stream, C->B, C->D, C->VB, pval_dev, (int)P->data->p, MCMC, per ? 1 : 0);
    HIPCHK(hipGetLastError());
    C->finalized = true;
  } else if (pval_dev) {
    hipLaunchKernelGGL(k_final_markers, dim3(1024), dim3(256), 0, P->stream, C->B, C->D, C->VB, pval_dev, (int)P->data->p, 1.0f, per ? 1 : 0);
  }
  ChainScalars h;
  HIPCHK(hipMemcpyAsync(&h, C->sc, sizeof(h), hipMemcpyDeviceToHost, P->stream));
  HIPCHK(hipStreamSynchronize(P->stream));
  const float MU = h.MU / MCMC, VE = h.VE / MCMC;
  float VBs = h.VBs / MCMC, Pi = 0, vg;
  if (C->model == BWGR_BAYESCPI || C->model == BWGR_BAYESDPI) Pi = 1 - h.Pi / MCMC;   // :911
  if (per) {
    CHK(sum_floats(P->stream, {{C->VB, (int64_t)P->data->p, &vg}}, "chain_result"));   // vg = VB.sum()
  } else {
    vg = VBs * C->MSx_eff;
    if (C->model == BWGR_BAYESCPI) vg = VBs * C->MSx_eff / Pi;                         // :913
  }
  if (mu) *mu = MU;
  if (ve) *ve = VE;
  if (h2) *h2 = vg / (vg + VE);
  if (MSx) *MSx = C->MSx_eff;
  if (pi) *pi = Pi;
  if (b) HIPCHK(d2h(P->stream, b, C->B, pb));
  if (d) HIPCHK(d2h(P->stream, d, C->D, pb));
  if (vb) { if (per) HIPCHK(d2h(P->stream, vb, C->VB, pb)); else vb[0] = VBs; }
  if (pval) HIPCHK(d2h(P->stream, pval, pval_dev, pb));
  if (hat) {
    DevBufs fit;
    float *hat_dev = fit.get<float>((size_t)P->data->n);
    if (fit.failed()) return no_memory("chain_result");
    CHK(gemv_hat<float>(P, C->B, MU, hat_dev, "chain_result", P->data->cen));
    HIPCHK(d2h(P->stream, hat, hat_dev, sizeof(float) * P->data->n));
  }
  return BWGR_OK;
}

extern "C" int bwgr_bayes(bwgr_panel *P, int model, const float *y, float it, float bi, float pi, float df, float R2,
                          uint64_t seed, int rng_mode, float *mu, float *b, float *d, float *hat, float *vb, float *ve,
                          float *h2, float *MSx, float *pi_out, float *pval) {
  bwgr_chain *C = nullptr;
  CHK(bwgr_chain_create(&C, P, model, y, BWGR_HOST, it, bi, pi, df, R2, seed, rng_mode));
  Guard drop([&] { bwgr_chain_destroy(C); });
  CHK(bwgr_chain_run(C, (int)it));
  return bwgr_chain_result(C, mu, b, d, hat, vb, ve, h2, MSx, pi_out, pval);
}

// BayesA2 / BayesB2 / BayesRR2, src/Rcpp20260726ai.cpp:990-1218: two chains over two panels sharing the residual
extern "C" int bwgr_bayes2(bwgr_panel *P1, bwgr_panel *P2, int base_model, const float *y, float it, float bi, float pi, float df,
                           float R2, uint64_t seed, int rng_mode, float *mu, float *b1, float *d1, float *vb1, float *b2,
                           float *d2, float *vb2, float *ve, float *hat, float *h2) {
  if ((P1 && P1->data->cen) || (P2 && P2->data->cen)) return refuse_centred("bayes2");
  if (!P1 || !P2 || !y) return fail(BWGR_EINVAL, "bayes2: null pointer");
  if (base_model != BWGR_BAYESA && base_model != BWGR_BAYESB && base_model != BWGR_BAYESRR)
    return fail(BWGR_EINVAL, "bayes2: base model must be BayesA, BayesB or BayesRR (got %d)", base_model);
  if (P1->data->device != P2->data->device || P1->data->n != P2->data->n || P1->data->plan.ld != P2->data->plan.ld || P1->data->plan.K != P2->data->plan.K || P1->data->plan.R != P2->data->plan.R)
    return fail(BWGR_EINVAL, "bayes2: the two panels must share device, rows and slab geometry (n %lld/%lld, %d x %d vs %d x %d rows)",
                (long long)P1->data->n, (long long)P2->data->n, P1->data->plan.K, P1->data->plan.R, P2->data->plan.K, P2->data->plan.R);
  const int64_t p1 = P1->data->p, p2 = P2->data->p, n = P1->data->n;
  if (p1 + p2 > 0xFFFFFFF0ll - 2) return fail(BWGR_EINVAL, "bayes2: p1 + p2 too large");
  HIPCHK(hipSetDevice(P1->data->device));
  hipStream_t s2_saved = P2->stream;
  P2->stream = P1->stream;   // one stream orders the two chains' kernels
  Guard restore([&] { P2->stream = s2_saved; });
  bwgr_chain *C1 = nullptr, *C2 = nullptr;
  Guard drop([&] { bwgr_chain_destroy(C2); bwgr_chain_destroy(C1); });
  DevBufs bufs;
  CHK(bwgr_chain_create_sharded(&C1, P1, base_model, y, BWGR_HOST, it, bi, pi, df, R2, seed, rng_mode, 0, p1 + p2, P1->data->MSx, nullptr));
  CHK(bwgr_chain_create_sharded(&C2, P2, base_model, y, BWGR_HOST, it, bi, pi, df, R2, seed, rng_mode, p1, p1 + p2, P2->data->MSx, C1->e));
  const bool rr = (base_model == BWGR_BAYESRR), per = !rr;
  if (base_model == BWGR_BAYESB) { C1->flags_extra = SWF_ALT_B2; C2->flags_extra = SWF_ALT_B2; }
  if (rr) {
    hipLaunchKernelGGL(k_set_rr2_start, dim3(1), dim3(1), 0, P1->stream, C1->sc);
    hipLaunchKernelGGL(k_set_rr2_start, dim3(1), dim3(1), 0, P1->stream, C2->sc);
  }
  const int iit = (int)it, ibi = (int)bi;
  for (int i = 0; i < iit; ++i) {
    CHK(bwgr_chain_sweep_blocks(C1, 0, (int)P1->data->plan.nblocks));
    CHK(bwgr_chain_sweep_blocks(C2, 0, (int)P2->data->plan.nblocks));
    const int accumulate = (i > ibi) ? 1 : 0;                                        // if(i>ibi), :1047
    Tail2Args t; t.e = C1->e; t.n = (int)n; t.p1 = (int)p1; t.p2 = (int)p2; t.rr = rr ? 1 : 0; t.df = df;
    t.accumulate = accumulate; t.iter = (uint32_t)i; t.rng = make_rng(seed, rng_mode); t.sc1 = C1->sc; t.sc2 = C2->sc;
    hipLaunchKernelGGL(k_tail2, dim3(1), dim3(1024), 0, P1->stream, t);
    hipLaunchKernelGGL(k_marker_tail, dim3((unsigned)std::min<int64_t>(2048, (p1 + 255) / 256)), dim3(256), 0, P1->stream,
                       C1->b, C1->d, C1->vb, C1->lam, C1->B, C1->D, C1->VB, (int)p1, base_model, 0.0f, accumulate, C1->sc);
    hipLaunchKernelGGL(k_marker_tail, dim3((unsigned)std::min<int64_t>(2048, (p2 + 255) / 256)), dim3(256), 0, P1->stream,
                       C2->b, C2->d, C2->vb, C2->lam, C2->B, C2->D, C2->VB, (int)p2, base_model, 0.0f, accumulate, C2->sc);
    HIPCHK(hipGetLastError());
    C1->done++; C2->done++;
  }
  CHK(bwgr_chain_sync(C1));
  CHK(bwgr_chain_sync(C2));
  const float MCMC = it - bi;                                                        // :1049
  hipLaunchKernelGGL(k_final_markers, dim3(1024), dim3(256), 0, P1->stream, C1->B, C1->D, C1->VB, (float *)nullptr, (int)p1, MCMC, per ? 1 : 0);
  hipLaunchKernelGGL(k_final_markers, dim3(1024), dim3(256), 0, P1->stream, C2->B, C2->D, C2->VB, (float *)nullptr, (int)p2, MCMC, per ? 1 : 0);
  HIPCHK(hipGetLastError());
  ChainScalars g1, g2;
  HIPCHK(hipMemcpyAsync(&g1, C1->sc, sizeof(g1), hipMemcpyDeviceToHost, P1->stream));
  HIPCHK(hipMemcpyAsync(&g2, C2->sc, sizeof(g2), hipMemcpyDeviceToHost, P1->stream));
  HIPCHK(hipStreamSynchronize(P1->stream));
  const float MU = g1.MU / MCMC, VE = g1.VE / MCMC, VB1s = g1.VBs / MCMC, VB2s = g2.VBs / MCMC;
  float vg;
  if (per) {                                                                         // vg = VB1.sum() + VB2.sum(), :1051
    float v1 = 0, v2 = 0;
    CHK(sum_floats(P1->stream, {{C1->VB, (int64_t)p1, &v1}, {C2->VB, (int64_t)p2, &v2}}, "bayes2"));
    vg = v1 + v2;
  } else vg = VB1s * P1->data->MSx + VB2s * P2->data->MSx;                                       // :1213
  if (mu) *mu = MU;
  if (ve) *ve = VE;
  if (h2) *h2 = vg / (vg + VE);
  if (b1) HIPCHK(d2h(P1->stream, b1, C1->B, sizeof(float) * p1));
  if (b2) HIPCHK(d2h(P1->stream, b2, C2->B, sizeof(float) * p2));
  if (d1) HIPCHK(d2h(P1->stream, d1, C1->D, sizeof(float) * p1));
  if (d2) HIPCHK(d2h(P1->stream, d2, C2->D, sizeof(float) * p2));
  if (vb1) { if (per) HIPCHK(d2h(P1->stream, vb1, C1->VB, sizeof(float) * p1)); else vb1[0] = VB1s; }
  if (vb2) { if (per) HIPCHK(d2h(P1->stream, vb2, C2->VB, sizeof(float) * p2)); else vb2[0] = VB2s; }
  if (hat) {                                                                         // fit = X1*B1 + X2*B2; fit += MU, :1052-1053
    float *fit1d = bufs.get<float>((size_t)n), *fit2d = bufs.get<float>((size_t)n), *hatd = bufs.get<float>((size_t)n);
    if (bufs.failed()) return no_memory("bayes2");
    CHK(gemv_hat<float>(P1, C1->B, 0.0f, fit1d, "bayes2"));
    CHK(gemv_hat<float>(P2, C2->B, 0.0f, fit2d, "bayes2"));
    hipLaunchKernelGGL(k_hat2, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, P1->stream, fit1d, fit2d, MU, hatd, (int)n);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(P1->stream, hat, hatd, sizeof(float) * n));
  }
  return BWGR_OK;
}
