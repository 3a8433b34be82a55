// bwgr_amd/csrc/sweep_host.hip.h -- a sweep on the host, for every family: its plan (SweepPlan, plan_sweep, bwgr_debug_sweep_plan), the occupancy
// guard that prices the plan, the kernels in front of a sweep (launch_prestage, draws_ahead), the launch train behind the plan (SweepTrain,
// launch_sweep), sweep_args, and the entries that answer from a plan (bwgr_panel_max_concurrent / _max_pairs / _pipeline, bwgr_debug_sweep3_kernel,
// bwgr_debug_withhold).  Part of bwgr_hip.hip, which includes it after the handle structs and before panel_host.hip.h (bwgr_panel_destroy forgets
// the handle's guard entry); it defines no kernel.  It creates and destroys no event or stream: the guard event, the hand-over event and the draws
// group are the handle's holder's, made by the first sweep that needs them and reused; SweepTrain::ev are the caller's (a chain's timing pairs).
// ---- the sweep plan -----------------------------------------------------------------------------------------------------------
// Which engine a sweep runs, how deep, in what launch shape and between which helper kernels is one decision, made by plan_sweep (below) from
// host facts about the panel and the handle (SweepFacts: geometry, Gram range, clones, switches), the sweep's flags and block range, and its
// mode: a sweep alone, the fp64 redo of one, or a pair's.  The launch code executes a plan and decides nothing of its own; the occupancy guard
// prices the plan's spin launches; bwgr_debug_sweep_plan() exposes every field to the CPU tests.
enum SweepMode { SWEEP_ALONE = 0, SWEEP_REDO = 1, SWEEP_PAIR = 2 };   // (PAIR: bwgr_chain_run_pair -- every selection sweep is k_sweep3's, one k_sweep3p launch for two chains, no redo)
// resident: the workgroups of the grid that stay for the sweep (L2 prefetch workgroups beyond the first few leave at once)
struct SpinLaunch { const void *fn; int grid, resident, threads; size_t lds; };
// One launch of k_sweep, k_sweep2 or k_sweep2w: what runs behind the gate (SweepPlan::run) and what redoes a guarded sweep (SweepPlan::redo)
struct EngineLaunch {
  int engine = 1;          // 1 k_sweep, 2 k_sweep2, 4 k_sweep2w
  int lag = 2, nfeed = 0;  // pipeline depth; q feeder workgroups of k_sweep2
  bool g16 = false;        // k_sweep2 on the 16-bit Gram copies
  int fx = 0, nd = 0, npf = 0, ahead = 0, nq = 0, wsub = 0, wK3 = 0;   // k_sweep2w
  int spin = -1;           // its launch among SweepPlan::spins; -1: not launched (every sweep is k_sweep3's)
  int cen = -1;            // k_cen_begin / k_cen_end around it with this mode argument (1: behind the gate, 2: the redo); -1: none
  bool spec = false, cen_tot = false;   // the redo: k_spec of the state just restored, behind k_cen_tot / k_cen_scan (mode 2) on centred columns
};
struct SweepPlan {
  int engine = 1;          // bwgr_panel_pipeline's generation: 1 k_sweep, 2 k_sweep2, 3 k_sweep3 (k_sweep2 beside it while the gate is finite), 4 k_sweep2w
  float gate3 = 0.0f;      // k_sweep3 takes the sweeps of chains below this inclusion rate (decided on the device); 0: never, INFINITY: every one
  EngineLaunch run, redo;  // behind the gate; the fp64 redo (guarded)
  int R3 = 0, K3 = 0, sub = 0, pf = -1, pf2 = -1, dbg3 = 0, qsplit = 0, skip_vb = 0;   // k_sweep3 (dbg3: S3_DMA4 / S3_DMA3, and BWGR_DBG3)
  bool fixed3 = false;     // ... as k_sweep3f, the fixed-shape instantiation
  bool guarded = false;    // the range snapshot in front, k_range_recover and the redo behind (no redo where the snapshot's scratch cannot be had)
  bool draws = false;      // the next iteration's variates drawn beside the sweep (draws_ahead)
  // the helper kernels, in launch order.  launch_prestage: k_escale_reset; k_escale on the gate and k_spec3 (sweep3) with k_cen_tot / k_cen_scan
  // mode 0 between them (cen3); k_escale at infinity (escale_w) and k_affine_inv; k_cen_tot / k_cen_scan mode 1 (cen_pre) and k_spec<int32_t> (spec
  // 1) or k_spec<double> (2) with spec_sel.  launch_engine: k_cen_begin / k_cen_end mode 0 around k_sweep3 (cen3), k_vb_fill behind it
  bool escale_reset = false, sweep3 = false, cen3 = false, escale_w = false, affine_inv = false, cen_pre = false, vb_fill = false;
  int spec = 0, spec_sel = 0;
  bool withhold = false;   // SWF_DEBUG_WITHHOLD on every launch (bwgr_debug_withhold)
  int nspins = 0; SpinLaunch spins[3];   // the launches whose workgroups wait for one another, in launch order: k_sweep3's or the pair's, run's, redo's
};
static void spin_launch(const SpinLaunch &L, hipStream_t st, void **args) { (void)hipLaunchKernel(L.fn, dim3(L.grid), dim3(L.threads), args, L.lds, st); }

// ---- occupancy guard -------------------------------------------------------------------------------------------------------------
// The sweep kernels' workgroups wait for one another (slab-dot exchanges, the sequencer's decisions), so every workgroup of a launch has
// to be resident at once -- beside the workgroups of whatever other handles' sweeps are in flight on the same device.  A launch that would
// not fit spins to its wall-clock bound and ends in BWGR_ETIMEOUT; the guard refuses it up front with BWGR_EINVAL instead, from the
// spin launches of the sweep's plan.
static std::mutex g_guard_mu;
static std::vector<bwgr_panel *> g_guard_panels;   // handles with a guard event (any device)
// the arithmetic (also bwgr_debug_occupancy_fits, which the CPU tests call): a launch of `grid` workgroups, `per_cu` of which fit one
// compute unit, needs ceil(grid / per_cu) units; it fits when those and the `busy` units of other streams' sweeps are within `cus`
static int occupancy_fits(int grid, int per_cu, int cus, int busy, int *need) {
  if (need) *need = 0;
  if (grid < 1 || cus < 1 || busy < 0) return BWGR_EINVAL;
  if (per_cu < 1) return BWGR_EINVAL;
  const int nd = (grid + per_cu - 1) / per_cu;
  if (need) *need = nd;
  return (nd + busy <= cus) ? BWGR_OK : BWGR_EINVAL;
}
extern "C" int bwgr_debug_occupancy_fits(int grid, int per_cu, int cus, int busy, int *need) { return occupancy_fits(grid, per_cu, cus, busy, need); }
static int guard_per_cu(const SpinLaunch &L) {
  static std::mutex mu; static std::vector<std::pair<SpinLaunch, int>> cache;
  std::lock_guard<std::mutex> lk(mu);
  for (auto &c : cache) if (c.first.fn == L.fn && c.first.threads == L.threads && c.first.lds == L.lds) return c.second;
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, L.fn, L.threads, L.lds) != hipSuccess) { (void)hipGetLastError(); nb = 0; }
  cache.push_back({L, nb});
  return nb;
}
static int device_cus(int device) {
  static std::mutex mu; static std::vector<int> cus;
  std::lock_guard<std::mutex> lk(mu);
  if ((int)cus.size() <= device) cus.resize(device + 1, 0);
  if (!cus[device]) { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) cus[device] = prop.multiProcessorCount; else (void)hipGetLastError(); }
  return cus[device];
}
// compute units the plan's spin launches hold: launches of one sweep follow one another on one stream, so the largest of them
static int plan_cus(const SweepPlan &pl, int cus, int busy, int *need_out) {
  int need = 0;
  for (int i = 0; i < pl.nspins; ++i) {
    const SpinLaunch &L = pl.spins[i];
    const int per = guard_per_cu(L);
    int nd = 0;
    if (per < 1) return fail(BWGR_EINVAL, "occupancy guard: a sweep kernel (%d threads, %zu bytes of LDS) does not fit a compute unit", L.threads, L.lds);
    if (occupancy_fits(L.resident, per, cus, busy, &nd) != BWGR_OK)
      return fail(BWGR_EINVAL, "occupancy guard: a sweep launch of %d workgroups (%d per compute unit) needs %d compute units; %d of %d are held by other handles' sweeps "
                  "in flight (their workgroups wait for one another, so all must be resident at once: run fewer chains side by side -- bwgr_panel_max_concurrent -- or "
                  "wait for the others)", L.resident, per, nd, busy, cus);
    need = std::max(need, nd);
  }
  *need_out = need;
  return BWGR_OK;
}
// units held by sweeps in flight on other streams of P's device (handles whose event has completed drop out)
static int guard_busy(const bwgr_panel *P, hipStream_t mine, const bwgr_panel *partner = nullptr) {
  std::vector<std::pair<hipStream_t, int>> per_stream;
  for (bwgr_panel *Q : g_guard_panels) {
    if (Q == P || Q == partner || Q->data->device != P->data->device || Q->guard_cus == 0) continue;   // (a pair's stream waits for both handles' earlier sweeps)
    if (hipEventQuery(Q->guard_ev) == hipSuccess) { Q->guard_cus = 0; continue; }
    (void)hipGetLastError();   // (hipErrorNotReady)
    if (Q->guard_stream == mine) continue;   // the same stream: one after the other
    bool seen = false;
    for (auto &ps : per_stream) if (ps.first == Q->guard_stream) { ps.second = std::max(ps.second, Q->guard_cus); seen = true; }
    if (!seen) per_stream.push_back({Q->guard_stream, Q->guard_cus});
  }
  int busy = 0;
  for (auto &ps : per_stream) busy += ps.second;
  return busy;
}
// The compute units the plan's spin launches hold on stream st; refused with BWGR_EINVAL when they cannot be resident beside the sweeps
// other handles (but partner) have in flight on this device.  BWGR_OCC_GUARD=0 switches the guard off.
static int sweep_guard(const bwgr_panel *P, const SweepPlan &pl, hipStream_t st, const bwgr_panel *partner, int *need) {
  *need = 0;
  if (!P->data->sw.occ_guard) return BWGR_OK;
  const int cus = device_cus(P->data->device);
  if (cus < 1) return BWGR_OK;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  return plan_cus(pl, cus, guard_busy(P, st, partner), need);
}
// after the real launches: this handle holds `need` units until the event behind them completes (no event: no guard entry)
static void guard_mark(bwgr_panel *P, hipStream_t st, int need) {
  if (need <= 0) return;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  if (!P->guard_ev && !(P->guard_ev = P->own.event(hipEventDisableTiming))) return;
  if (!P->guard_listed) { g_guard_panels.push_back(P); P->guard_listed = true; }
  if (P->guard_cus > 0 && P->guard_stream == st && hipEventQuery(P->guard_ev) != hipSuccess) { (void)hipGetLastError(); need = std::max(need, P->guard_cus); }
  P->guard_cus = need; P->guard_stream = st;
  (void)hipEventRecord(P->guard_ev, st);
}
// before the handle is deleted (guard_busy queries other handles' events under the mutex): unlisted here, its event goes with its holder
static void guard_forget(bwgr_panel *P) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  for (size_t i = 0; i < g_guard_panels.size(); ++i) if (g_guard_panels[i] == P) { g_guard_panels.erase(g_guard_panels.begin() + i); break; }
  P->guard_listed = false; P->guard_cus = 0; P->guard_stream = nullptr;
}

// polled words are zeroed before every launch (epochs count within a launch)
static int reset_exchange(bwgr_panel *P) {
  if (P->data->plan.pipelined) {
    HIPCHK(hipMemsetAsync(P->xchg, 0, P->xchg_bytes, P->stream));
  } else if (P->data->plan.K > 1) {
    HIPCHK(hipMemsetAsync(P->xflags, 0, sizeof(uint32_t) * ((size_t)P->data->plan.K + 1) * SW_FLAG_STRIDE, P->stream));
  }
  return BWGR_OK;
}

// the DMA streamer's lane offsets are 32-bit: (columns of the launch) * (rows of a slab) bytes must stay below 4 GiB
static bool stream3_dma_fits(int64_t ncols, int64_t R) { return ncols >= 0 && R > 0 && (uint64_t)ncols * (uint64_t)R < (1ull << 32); }
extern "C" int bwgr_debug_stream3_dma(int64_t ncols, int64_t R) { return stream3_dma_fits(ncols, R) ? 1 : 0; }
// The affine sweeps of an int8 panel with 16-bit Gram staging run k_sweep2w: the block solve as a product with the inverse
// k_affine_inv forms before the sweep (sweep2w.hip.h).
static int winv_alloc(bwgr_panel *P) {
  const size_t nb = (size_t)P->data->plan.nblocks;
  if (!P->winv && !P->own.take({{&P->winv, sizeof(double) * S2W_WDOUBLES * nb}, {&P->qsumw, sizeof(unsigned long long) * 4 * 2 * SW_MAXM * nb}}))   // (up to four copies)
    return no_memory("affine sweep");
  return BWGR_OK;
}

// What plan_sweep reads: host fields of the panel's data and of the handle, nothing on the device.  sweep_facts gathers them from a handle;
// bwgr_debug_sweep_plan fills them for a panel that was never made.
struct SweepFacts {
  const PanelPlan &plan; const Panel3Plan &plan3; const Switches &sw;
  int64_t p;
  bool is_f32, gram16, e3_ready, gx12;   // (gx12: the distance-1 / 2 records exist)
  int winv_nd;
  bool crowded, is_root; int nclones;
  bool withhold;                         // bwgr_debug_withhold is on
};
static SweepFacts sweep_facts(const bwgr_panel *P) {
  const PanelData *D = P->data;
  return SweepFacts{D->plan, D->plan3, D->sw, D->p, D->is_f32 != 0, D->gram16, D->e3_ready, D->gx12 != nullptr, D->winv_nd, D->crowded, P->is_root, D->nclones, P->debug_withhold != 0};
}

// The plan of one sweep of blocks [blk_begin, blk_end) with these flags, in this mode (SWEEP_REDO: the fp64 launch that redoes a fixed-point
// sweep which left its range -- the plan of a guarded sweep alone holds it as `redo`).  Host arithmetic: nothing is enqueued or allocated.
static SweepPlan plan_sweep(const SweepFacts &F, int flags, int blk_begin, int blk_end, SweepMode mode) {
  SweepPlan pl;
  EngineLaunch &E = pl.run;
  const Switches &sw = F.sw; const PanelPlan &pp = F.plan;
  const bool redo = mode == SWEEP_REDO, pair = mode == SWEEP_PAIR;
  const bool sel = (flags & SWF_SELECT) != 0, cen = (flags & SWF_CENTRE) != 0;
  const auto spin = [&](const void *fn, int grid, int resident, int threads, size_t lds) { pl.spins[pl.nspins] = SpinLaunch{fn, grid, resident, threads, lds}; return pl.nspins++; };
  // The selection models' sweeps on a panel that has k_sweep3: the device picks the engine from the chain's current inclusion rate
  // (ChainScalars::inc_rate against the panel's threshold), so both engines' kernels are enqueued and one side leaves at once (a few
  // microseconds per iteration); a threshold >= 1, or a pair run, means k_sweep3 always and the other side is not enqueued at all.
  if (F.e3_ready && sel && !(flags & SWF_EM_ANY) && !redo) pl.gate3 = (sw.eng3_thr >= 1.0f || pair) ? INFINITY : sw.eng3_thr;
  // The affine sweeps of an int8 panel with 16-bit Gram staging: k_sweep2w, with its own streamers (s2w_streamer_fx: 128 rows each,
  // fixed-point residual) where the slab count allows
  const bool winv = sw.winv && pp.pipelined && !F.is_f32 && F.winv_nd >= 1 && pp.K <= 2 * (S2W_QW + S2W_QX) &&
                    !(flags & (SWF_SELECT | SWF_EM_ANY | SWF_SERIAL)) && pp.ldsw > 0 && pp.ldsw <= (size_t)160 * 1024;
  const bool wfx = sw.wfx && (pp.R % S2W_FXR) == 0 && pp.K * (pp.R / S2W_FXR) <= 255;
  E.engine = winv ? 4 : pp.pipelined ? 2 : 1;
  pl.engine = pl.gate3 > 0.0f ? 3 : E.engine;
  // Selection sweeps of k_sweep2: three blocks deep.  (The single-barrier sequencer also knows a fourth level, BWGR_LAG=4: it was
  // the default while k_sweep2 also ran the sparse chains; those are k_sweep3's now, and from 5 % of the markers in the model upwards
  // the third cross term's row fetches cost more than the depth gives -- C4-size BayesC at 5 / 19 / 36 % inclusion: 31.4 / 21.3 /
  // 14.5 iter/s at depth 3 against 30.9 / 19.4 / 9.4 at depth 4; BayesCpi at 51 %: 11.1 against 6.7.)  BWGR_LAG=2|3|4 sets it (A/B tests).
  int lag = 2;
  if (pp.pipelined && sel) {
    // the generic sequencer (32-bit Gram entries, fp32 panels) reads a distance-2 row per accepted marker straight from global memory on
    // one wave: two blocks deep unless asked (us per block at n = 10 000, depth 2 / 3: 1.4 % inclusion 4.53 / 4.67, 10.9 % 5.29 / 14.5,
    // BayesCpi at 52 % 12.7 / 58.0); the 16-bit / single-barrier sequencer stages those rows and knows a third cross term as well
    if (pp.xdist >= 2 && (sw.lag >= 0 || F.gram16)) lag = 3;
    if (pp.xdist >= 3 && F.gram16) lag = 4;   // (a panel with distance-3 blocks fits the lag-4 streamer: plan_panel)
  }
  E.lag = std::min(lag, (sw.lag >= '2' && sw.lag <= '4') ? sw.lag - '0' : 3);
  if (winv) {   // the affine sweeps' product sequencer: as deep as the panel's cross Gram planes reach (BWGR_WLAG caps it)
    E.lag = std::min(F.winv_nd + 1, sw.wlag_cap);
    if (!wfx) E.lag = std::min(E.lag, 4);   // (k_sweep2's streamers hold four tiles)
#ifdef BWGR_EXPERIMENTS
    if (sw.wlag_timing) E.lag = sw.wlag_timing;   // TIMING ONLY: deeper than the cross terms reach (wrong chain)
#endif
  }
  // streamers, sequencer, and for the selection models the q feeders (the affine recurrence is compute-bound: its
  // sequencer gathers q itself under the recurrence, and a feeder hop in its lag-2 chain measured 15 % slower)
  E.nfeed = (pp.pipelined && sel) ? pp.nfeed : 0;
  // selection models: 16-bit staging and the single-barrier sequencer (the affine recurrence is compute-bound and measured faster on
  // the 32-bit blocks: no conversion in its inner loop)
  E.g16 = pp.pipelined && F.gram16 && sel;
  // A chain that has the GPU to itself (a root panel without clones) runs 128-row streamers, two to a slab: 80 compute units instead
  // of 41, 15.98-16.18 against 16.49 ms per sweep at C4 (the same chain bit for bit: the slab dots are integer sums).  With clones
  // alive -- chains side by side, pairs -- every chain keeps the 256-row streamers the concurrency counts assume.  BWGR_SOLO3=0: never.
  const bool alone = F.plan3.solo3 && !F.crowded && F.is_root && F.nclones == 0;
  // The next iteration's variates beside the sweep (draws_ahead): selection models with the logistic step, only for a chain alone (beside
  // other chains or shards the idle compute units it would run on are theirs: five chains side by side 255 -> 226 chain-iter/s, three
  // shards 163 -> 119 iter/s with it); BWGR_DRAWS=0 switches it off
  pl.draws = sel && !(flags & (SWF_MH | SWF_EM_ANY)) && alone && sw.draws;
  if (pl.gate3 > 0.0f) {
    pl.sweep3 = true;
    pl.R3 = F.plan3.R3; pl.sub = F.plan3.sub3; pl.K3 = F.plan3.K3;
#ifdef BWGR_EXPERIMENTS
    pl.dbg3 = sw.dbg3;   // (timing switches, some of which break the chain: the experiment build only)
#endif
    {   // 128-row streamers land their tiles by LDS-DMA (s3_streamer_dma; C4 15.0 -> 13.65 ms per sweep); BWGR_STREAM3=reg: through registers, as the 256-row ones do
      // The DMA streamer forms a tile piece's source as a 32-bit lane offset from the launch's first column (no 64-bit vector arithmetic): only
      // launches whose column range spans less than 4 GiB of one slab take it (p * R < 2^32: 16.7 M markers at R = 256); wider ones keep the
      // register path, whose offsets are size_t.  bwgr_debug_stream3_dma() exposes the rule to the CPU tests.
      const int64_t j_lo = (int64_t)blk_begin * pp.m, j_hi = std::min<int64_t>(F.p, (int64_t)blk_end * pp.m);
      const bool fits32 = stream3_dma_fits(j_hi - j_lo, pp.R);
      if (sw.stream3 != 'r' && fits32) pl.dbg3 |= S3_DMA4;
      if (sw.stream3 == 'd' && fits32) pl.dbg3 |= S3_DMA3;   // (EXPERIMENT: the 256-row streamers too, three tile buffers)
    }
    if (pair) {   // a pair run (bwgr_chain_run_pair): one k_sweep3p launch, K3 streamers and two sequencers, serves both chains; no redo
      const size_t lds = std::max(s3p_streamer_lds(pl.R3), s3_seq_lds(F.plan3.D, F.gram16));
      spin(F.gram16 ? reinterpret_cast<const void *>(k_sweep3p<uint16_t>) : reinterpret_cast<const void *>(k_sweep3p<int32_t>), pl.K3 + 2, pl.K3 + 2, SW_THREADS, lds);
    } else {
      if (alone && pl.R3 == 256 && 2 * pl.K3 + 1 <= 256) { pl.R3 = 128; pl.sub = pp.R / 128; pl.K3 = pp.K * pl.sub; }
      // one more workgroup, on the sequencer's XCD (workgroups with equal index mod 8 share an XCD), warms that XCD's L2 with what the
      // staging waves load (on for a chain alone on the GPU: 15.61 -> 15.37 ms per sweep at C4 on the steadied kernel; beside other chains
      // the workgroup is not counted by bwgr_panel_max_concurrent, so it stays off there; BWGR_PF3=0|1 decides otherwise)
      const bool pf_on = (sw.pf3 >= 0 ? sw.pf3 == '1' : alone) && pl.K3 + 2 <= 256;
      pl.pf = pf_on ? ((pl.K3 + 2 > 8) ? 8 : pl.K3 + 1) : -1;
      const bool pf2_on = pf_on && pl.pf == 8 && F.gram16 && F.gx12 && pl.K3 + 3 > 16 && pl.K3 + 3 <= 256 && sw.pf3b;
      pl.pf2 = pf2_on ? 16 : -1; pl.qsplit = 1; pl.skip_vb = (flags & SWF_VB_VEC) ? 1 : 0;
      const int grid = pl.K3 + 1 + (pf_on ? 1 : 0) + (pf2_on ? 1 : 0);
      const void *fn = F.gram16 ? (cen ? reinterpret_cast<const void *>(k_sweep3<uint16_t, true>) : reinterpret_cast<const void *>(k_sweep3<uint16_t, false>))
                                    : (cen ? reinterpret_cast<const void *>(k_sweep3<int32_t, true>) : reinterpret_cast<const void *>(k_sweep3<int32_t, false>));
      // k_sweep3f (sweep3.hip.h, S3Shape128) is this launch with its geometry as constants and no other role compiled in: taken where the launch is exactly
      // that -- 128 markers a block and their packed stride, 16-bit Gram entries with the distance-1 / 2 records, columns as stored, 128-row DMA streamers
      // with four tile buffers and nothing else asked of dbg3 (the experiment build keeps BWGR_DBG3: the same switches in both kernels), the 4 + 3 digit
      // split; not under the abort hook, whose absent streamer is k_sweep3's.  The same chain bit for bit; bwgr_debug_sweep3_kernel() tells which one runs.
      pl.fixed3 = sw.fixed3 && F.gram16 && !cen && F.gx12 && pp.m == S3Shape128::m && pp.pstride == S3Shape128::pstride &&
                  pl.R3 == 128 && (pl.dbg3 & S3_DMA_ANY) == S3_DMA4 && pl.qsplit == 1 && !F.withhold;
      spin(pl.fixed3 ? reinterpret_cast<const void *>(k_sweep3f) : fn, grid, grid, SW_THREADS, F.plan3.lds3);
    }
  }
  if (!std::isinf(pl.gate3)) {
    if (winv) {
      E.fx = (wfx && !redo) ? 1 : 0;
      if (!E.fx) E.lag = std::min(E.lag, 4);   // (k_sweep2's streamers -- the range-recovery launch, BWGR_WFX=0 -- hold four tiles)
      E.nd = std::min(E.lag - 1, (int)S2W_MAXDIST);
      E.npf = sw.wpf; E.ahead = sw.wahead;   // (npf measured at C2: 0 -> 540, 2 -> 636, 4 -> 685 iter/s; 6 and 8 no better)
      E.wsub = pp.R / S2W_FXR; E.wK3 = pp.K * E.wsub;
      E.nq = sw.wnq ? sw.wnq : (E.wK3 > 48 ? 2 : 1);   // (C2, 40 streamers: one copy 1.10 ms, two 1.21; C4 shape, 80 streamers: 27.8 / 25.6 / 27.6 ms with 1 / 2 / 4)
      // (of the 8 npf workgroups past the sequencer, the npf on its XCD prefetch; the others leave at once)
      const int wgs = E.fx ? E.wK3 : pp.K;
      E.spin = spin(E.fx ? reinterpret_cast<const void *>(k_sweep2w<true>) : reinterpret_cast<const void *>(k_sweep2w<false>), wgs + 1 + 8 * E.npf, wgs + 1 + E.npf, S2W_THREADS, pp.ldsw);
    } else if (pp.pipelined) {
      const void *fn = F.is_f32 ? (sel ? reinterpret_cast<const void *>(k_sweep2<float, true>) : reinterpret_cast<const void *>(k_sweep2<float, false>))
                       : E.g16  ? reinterpret_cast<const void *>(k_sweep2<int8_t, true, uint16_t>)
                       : sel     ? reinterpret_cast<const void *>(k_sweep2<int8_t, true>) : reinterpret_cast<const void *>(k_sweep2<int8_t, false>);
      E.spin = spin(fn, pp.K + 1 + E.nfeed, pp.K + 1 + E.nfeed, SW_THREADS, pp.lds2);
    } else {
      const void *fn = F.is_f32 ? (sel ? reinterpret_cast<const void *>(k_sweep<float, true>) : reinterpret_cast<const void *>(k_sweep<float, false>))
                                 : (sel ? reinterpret_cast<const void *>(k_sweep<int8_t, true>) : reinterpret_cast<const void *>(k_sweep<int8_t, false>));
      E.spin = spin(fn, pp.K, pp.K, SW_THREADS, pp.lds);
    }
  }
  // The fixed-point engines between a snapshot of the state they start from and the fp64 engine that redoes the sweep if they left
  // their range (the reference's update cannot fail, src/Rcpp20260726ai.cpp:681).  Off for the debug abort hook (its launches must time out).
#ifdef BWGR_EXPERIMENTS
  const bool no_recover = sw.no_recover;   // (timing experiments that break the chain on purpose: the experiment build only)
#else
  constexpr bool no_recover = false;
#endif
  if (mode == SWEEP_ALONE && (pl.gate3 > 0.0f || (winv && wfx)) && !F.withhold && !no_recover) {
    const SweepPlan r = plan_sweep(F, flags, blk_begin, blk_end, SWEEP_REDO);
    const SpinLaunch &L = r.spins[r.run.spin];
    pl.redo = r.run; pl.redo.spin = spin(L.fn, L.grid, L.resident, L.threads, L.lds);
    pl.guarded = true;
  }
  // the kernels around the launches (SweepPlan, above)
  const bool behind = E.spin >= 0, fp64 = behind && E.engine == 2;   // (engine 2: what is pipelined and not k_sweep2w)
  pl.cen3 = pl.sweep3 && cen; pl.vb_fill = pl.sweep3 && pl.skip_vb; pl.withhold = F.withhold;
  pl.escale_w = behind && E.engine == 4 && E.fx; pl.affine_inv = behind && E.engine == 4;
  pl.escale_reset = pl.sweep3 || pl.escale_w;
  pl.cen_pre = fp64 && cen && sel; pl.spec = fp64 ? (F.is_f32 ? 2 : 1) : 0; pl.spec_sel = sel ? 1 : 0;
  if (fp64 && cen && sel && !F.is_f32) E.cen = redo ? 2 : 1;
  E.spec = redo && E.engine == 2; E.cen_tot = E.spec && cen && sel;
  return pl;
}

// The plan without a device (test hook): plan_panel and plan_panel3 as bwgr_debug_panel_plan makes them (the switches of the environment, an
// assumed xmax and 16-bit verdict), then plan_sweep for a sweep with these flags over blocks [blk_begin, blk_end) (blk_end <= 0: the whole
// panel) in this mode, on a handle in this state.  The panel is taken to be one whose far blocks fit: e3_ready = plan3.fits, the distance-1 / 2
// records are there exactly when gram16 && plan3.fits, winv_nd = plan.wdist (0 without the 16-bit verdict).  Refused (BWGR_EINVAL) is what the
// library never plans: see include/bwgr.h, where out is described.
static int sweep_kernel_id(const void *fn) {
  const void *const tab[] = {reinterpret_cast<const void *>(k_sweep<int8_t, true>), reinterpret_cast<const void *>(k_sweep<int8_t, false>), reinterpret_cast<const void *>(k_sweep<float, true>),
    reinterpret_cast<const void *>(k_sweep<float, false>), reinterpret_cast<const void *>(k_sweep2<int8_t, true>), reinterpret_cast<const void *>(k_sweep2<int8_t, false>),
    reinterpret_cast<const void *>(k_sweep2<int8_t, true, uint16_t>), reinterpret_cast<const void *>(k_sweep2<float, true>), reinterpret_cast<const void *>(k_sweep2<float, false>),
    reinterpret_cast<const void *>(k_sweep2w<true>), reinterpret_cast<const void *>(k_sweep2w<false>),
    reinterpret_cast<const void *>(k_sweep3<uint16_t, false>), reinterpret_cast<const void *>(k_sweep3<int32_t, false>), reinterpret_cast<const void *>(k_sweep3<uint16_t, true>),
    reinterpret_cast<const void *>(k_sweep3<int32_t, true>), reinterpret_cast<const void *>(k_sweep3p<uint16_t>), reinterpret_cast<const void *>(k_sweep3p<int32_t>), reinterpret_cast<const void *>(k_sweep3f)};
  for (int i = 0; i < (int)(sizeof(tab) / sizeof(tab[0])); ++i) if (tab[i] == fn) return i;
  return -1;
}
extern "C" int bwgr_debug_sweep_plan(int is_f32, int64_t n, int64_t p, int block, int nwg, int kind, int xmax, int gram16, int flags, int blk_begin, int blk_end,
                                     int mode, int state, int64_t out[BWGR_SWEEP_PLAN_NOUT]) {
  if (!out || kind < PANEL_MAIN || kind > PANEL_EM || mode < SWEEP_ALONE || mode > SWEEP_PAIR || state < 0 || state > 15)
    return fail(BWGR_EINVAL, "debug_sweep_plan: null pointer, bad kind, mode or state");
  const Switches sw = read_switches();
  PanelPlan pp;
  CHK(plan_panel(pp, is_f32 != 0, n, p, block, nwg, (PanelKind)kind, sw));
  const bool g16 = gram16 != 0 && pp.has16 && sw.gram16;
  const Panel3Plan p3 = xmax >= 0 ? plan_panel3(pp, sw, g16) : Panel3Plan();
  const SweepFacts F{pp, p3, sw, p, is_f32 != 0, g16, p3.fits, g16 && p3.fits, g16 ? pp.wdist : 0, (state & 4) != 0, !(state & 2), (state & 3) ? 1 : 0, (state & 8) != 0};
  if (blk_end <= 0) { blk_begin = 0; blk_end = (int)pp.nblocks; }
  if (blk_begin < 0 || blk_begin >= blk_end || blk_end > pp.nblocks) return fail(BWGR_EINVAL, "debug_sweep_plan: bad block range");
  if ((state & 7) && kind != PANEL_MAIN) return fail(BWGR_EINVAL, "debug_sweep_plan: only a main panel has clones or shards");
  const bool sel = (flags & SWF_SELECT) != 0, cen = (flags & SWF_CENTRE) != 0;
  if (cen && !(F.e3_ready && sel && !(flags & SWF_EM_ANY))) return fail(BWGR_EINVAL, "debug_sweep_plan: implicitly centred columns are swept by the selection models on a panel with k_sweep3");
  const SweepPlan alone = plan_sweep(F, flags, blk_begin, blk_end, SWEEP_ALONE);
  if (mode == SWEEP_REDO && !alone.guarded) return fail(BWGR_EINVAL, "debug_sweep_plan: this sweep has no redo");
  if (mode == SWEEP_PAIR && (alone.engine != 3 || cen || blk_begin != 0 || blk_end != pp.nblocks || s3p_streamer_lds(p3.R3) > (size_t)160 * 1024))
    return fail(BWGR_EINVAL, "debug_sweep_plan: a pair runs whole sweeps of two selection chains, columns as stored, on a panel with k_sweep3");
  const SweepPlan pl = mode == SWEEP_ALONE ? alone : plan_sweep(F, flags, blk_begin, blk_end, (SweepMode)mode);
  const EngineLaunch &E = pl.run, &Q = pl.redo, &R = mode == SWEEP_REDO ? pl.run : pl.redo;
  uint32_t gate_bits; memcpy(&gate_bits, &pl.gate3, sizeof(gate_bits));
  int64_t v[BWGR_SWEEP_PLAN_NOUT] = {pl.engine, pl.gate3 <= 0.0f ? 0 : std::isinf(pl.gate3) ? 2 : 1, gate_bits, E.lag, E.nfeed, E.g16, pl.R3, pl.K3, pl.sub, pl.pf, pl.pf2, pl.dbg3, pl.qsplit,
                                     pl.skip_vb, pl.fixed3, E.fx, E.nd, E.npf, E.ahead, E.nq, E.wsub, E.wK3, pl.guarded, pl.draws, pl.nspins};
  int k = 25;
  for (int i = 0; i < 3; ++i, k += 5) {
    const SpinLaunch &L = pl.spins[i];
    v[k] = -1;
    if (i < pl.nspins) { v[k] = sweep_kernel_id(L.fn); v[k + 1] = L.grid; v[k + 2] = L.resident; v[k + 3] = L.threads; v[k + 4] = (int64_t)L.lds; }
  }
  if (pl.guarded) { const int64_t r[11] = {Q.engine, Q.lag, Q.nfeed, Q.g16, Q.fx, Q.nd, Q.npf, Q.ahead, Q.nq, Q.wsub, Q.wK3}; std::copy(r, r + 11, v + k); }
  k += 11;
  const int64_t h[16] = {E.spin, Q.spin, pl.escale_reset, pl.sweep3, pl.cen3, pl.escale_w, pl.affine_inv, pl.cen_pre, pl.spec, pl.spec_sel, E.cen, Q.cen, R.spec, R.cen_tot,
                         pl.vb_fill, pl.withhold};
  std::copy(h, h + 16, v + k);
  static_assert(25 + 15 + 11 + 16 == BWGR_SWEEP_PLAN_NOUT, "bwgr_debug_sweep_plan writes every field");
  std::copy(v, v + BWGR_SWEEP_PLAN_NOUT, out);
  return BWGR_OK;
}

static void launch_prestage(bwgr_panel *P, const SweepArgs &a_in, const SweepPlan &pl) {
  SweepArgs a = a_in;
  a.gate3 = pl.gate3;
  const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
  const int64_t tasks = 4ll * (j1 - j0);
  const int sh_add = P->data->sw.sh_add;   // test hook: less headroom, to leave the range on purpose
  int xbits = 0; while ((1 << xbits) < std::max(1, P->data->xmax)) ++xbits;   // (the fixed-point scales: the residual, and what k_prestage knows of the steps times the largest |x|)
  if (pl.escale_reset) hipLaunchKernelGGL(k_escale_reset, dim3(1), dim3(1), 0, P->stream, a.sc);
  // the variates drawn ahead (draws_ahead, below) when they are this very iteration's
  DrawsAhead &dr = P->draws;
  a.draws = nullptr;
  if (dr.matches(a, j0, j1)) { const hipError_t he = hipStreamWaitEvent(P->stream, dr.ready, 0); if (he == hipSuccess) a.draws = dr.buf; else { fprintf(stderr, "bwgr: draws wait failed: %s\n", hipGetErrorString(he)); (void)hipGetLastError(); } }
  if (a.draws) {
    hipLaunchKernelGGL(k_prestage_fin, dim3((unsigned)std::min<int64_t>(2048, (j1 - j0 + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
    { const hipError_t he = hipEventRecord(dr.free, P->stream); if (he != hipSuccess) { fprintf(stderr, "bwgr: draws_free record failed: %s\n", hipGetErrorString(he)); (void)hipGetLastError(); } }
    dr.valid = false;   // (consumed: the buffer is the next iteration's from here)
  } else hipLaunchKernelGGL(k_prestage, dim3((unsigned)std::min<int64_t>(4096, (tasks + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
  if (pl.sweep3) {   // the sweep's fixed-point scale, then the in-block speculative terms on that grid
    hipLaunchKernelGGL(k_escale, dim3(1), dim3(1024), 0, P->stream, a.e, P->data->plan.ld, a.sc, xbits, a.gate3, sh_add);
    if (pl.cen3) {   // the rejected steps' share of sum(e_stored), block by block (the whole panel: launch_prestage is called with every block)
      hipLaunchKernelGGL(k_cen_tot, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, 0);
      hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, a, (int)P->data->plan.nblocks, 0);
    }
    hipLaunchKernelGGL(k_spec3, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, P->data->gram16 ? (const uint16_t *)P->data->gramp16 : (const uint16_t *)nullptr);
  }
  const unsigned nb = (unsigned)(a.blk_end - a.blk_begin);
  if (pl.escale_w) hipLaunchKernelGGL(k_escale, dim3(1), dim3(1024), 0, P->stream, a.e, P->data->plan.ld, a.sc, xbits, INFINITY, sh_add);   // (an affine sweep on the fixed-point streamers: |b0|, the noise terms)
  if (pl.affine_inv) hipLaunchKernelGGL(k_affine_inv, dim3(nb), dim3(512), S2W_INV_LDS, P->stream, a, P->winv, (a.flags & SWF_DELTA2) ? 2.0 : 1.0);
  if (pl.cen_pre) {   // the fp64 engine's share of an implicitly centred iteration (the float steps themselves; runs on k_sweep2's side of the gate)
    hipLaunchKernelGGL(k_cen_tot, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, 1);
    hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, a, (int)P->data->plan.nblocks, 1);
  }
  if (pl.spec == 2) hipLaunchKernelGGL(k_spec<double>, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, pl.spec_sel);
  else if (pl.spec == 1) hipLaunchKernelGGL(k_spec<int32_t>, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, pl.spec_sel);
}

// The next iteration's variates, enqueued beside this iteration's sweep (see k_draws) where the plan says so.  `a` = this iteration's arguments
// over the whole panel.  Failing to set it up is not an error, and is not tried again: k_prestage draws for itself whenever the buffer is not
// this iteration's.
static void draws_ahead(bwgr_panel *P, const SweepArgs &a, const SweepPlan &pl, hipEvent_t before_sweep) {
  DrawsAhead &dr = P->draws;
  if (!pl.draws || dr.unavailable) return;
  if (!dr.buf) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // (lo: the numerically largest = the lowest priority)
    dr.unavailable = hipFuncSetAttribute(reinterpret_cast<const void *>(k_draws), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess ||
                     !P->own.take({{&dr.buf, sizeof(double) * 5 * (size_t)P->data->p}, DevBufs::want_stream(&dr.stream, hipStreamNonBlocking, lo),
                                   DevBufs::want_event(&dr.ready, hipEventDisableTiming), DevBufs::want_event(&dr.free, hipEventDisableTiming)});
    if (dr.unavailable) { (void)hipGetLastError(); return; }
    (void)hipEventRecord(dr.free, P->stream);
  }
  const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
  // after this iteration's k_prestage has read the buffer (draws_free) -- or, the first time, after what is enqueued so far; 160 workgroups with 96 KB of
  // LDS each: at most 160 compute units, none of them one that runs a workgroup of the sweep
  // (... and after the iteration's speculative terms, which are bandwidth-bound and would share the chip with it: the event in front of the sweep)
  { const hipError_t h1 = hipStreamWaitEvent(dr.stream, dr.free, 0), h2 = hipStreamWaitEvent(dr.stream, before_sweep, 0);
    if (h1 != hipSuccess || h2 != hipSuccess) { fprintf(stderr, "bwgr: draws_ahead waits failed: %s / %s\n", hipGetErrorString(h1), hipGetErrorString(h2)); (void)hipGetLastError(); return; } }
  hipLaunchKernelGGL(k_draws, dim3(160), dim3(1024), 96 * 1024, dr.stream, a.rng, a.marker0, a.iter + 1u, a.flags, (const ChainScalars *)a.sc, (int64_t)P->data->p, j0, j1, dr.buf);
  { const hipError_t h1 = hipGetLastError(); const hipError_t h2 = (h1 == hipSuccess) ? hipEventRecord(dr.ready, dr.stream) : hipSuccess;
    if (h1 != hipSuccess || h2 != hipSuccess) { fprintf(stderr, "bwgr: k_draws launch / record failed: %s / %s\n", hipGetErrorString(h1), hipGetErrorString(h2)); (void)hipGetLastError(); dr.valid = false; return; } }
  dr.valid = true; dr.rng = a.rng; dr.iter = a.iter + 1u; dr.marker0 = a.marker0; dr.flags = a.flags & (SWF_SELECT | SWF_VB_VEC);
  dr.j0 = j0; dr.j1 = j1; dr.sc = (const void *)a.sc;
}

// what one launch of k_sweep3 / k_sweep3p needs beside the sweep's own arguments; zeroes the launch's slab-dot sums, takes a new epoch
static void sweep3_args(bwgr_panel *P, const SweepArgs &a, const SweepPlan &pl, Sweep3Args &A) {
  memset(&A, 0, sizeof(A)); A.a = a;
  for (int d = 0; d < S3_MAXD; ++d) A.gx[d] = P->data->g3x[d];
  A.gp = P->data->gram16 ? (const void *)P->data->gramp16 : P->data->gramp;
  A.D = P->data->plan3.D; A.K3 = pl.K3; A.R3 = pl.R3; A.sub = pl.sub; A.g16 = P->data->gram16 ? 1 : 0;
  A.qsum = P->qsum3; A.lists = P->lists3;
  A.gx12 = P->data->gram16 ? P->data->gx12 : nullptr;
  A.dbg = pl.dbg3; A.pf = pl.pf; A.pf2 = pl.pf2; A.qsplit = pl.qsplit; A.skip_vb = pl.skip_vb;
  P->epoch3 = (P->epoch3 + 1) & 0xFFFFFFu; if (P->epoch3 == 0) P->epoch3 = 1;
  A.epoch = P->epoch3;
  (void)hipMemsetAsync(P->qsum3 + (size_t)a.blk_begin * 2 * SW_MAXM, 0, sizeof(unsigned long long) * 2 * SW_MAXM * (size_t)(a.blk_end - a.blk_begin), P->stream);
}
// The launches of the plan behind the helper kernels of launch_prestage: k_sweep3 (for the implicitly centred columns between its scalar terms'
// kernels) and the per-marker variances, then the engine behind the gate -- or, redo, the fp64 engine behind a fixed-point sweep that left its range
static void launch_engine(bwgr_panel *P, const SweepArgs &a_in, const SweepPlan &pl, bool redo) {
  const EngineLaunch &E = redo ? pl.redo : pl.run;
  SweepArgs a = a_in;
  if (pl.withhold) a.flags |= SWF_DEBUG_WITHHOLD;
  a.gate3 = redo ? 0.0f : pl.gate3; a.redo_only = redo ? 1 : 0;
  if (E.spec) {   // the fp64 engine's speculative terms (k_spec) of the state just restored
    if (E.cen_tot) {   // the running block sums on the float steps (the fixed-point launch left them on its grid): every block, then the scan
      SweepArgs all = a; all.blk_begin = 0; all.blk_end = (int)P->data->plan.nblocks;
      hipLaunchKernelGGL(k_cen_tot, dim3((unsigned)P->data->plan.nblocks), dim3(128), 0, P->stream, all, 0, 2);
      hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, all, (int)P->data->plan.nblocks, 2);
    }
    hipLaunchKernelGGL(k_spec<int32_t>, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, pl.spec_sel);
  }
  if (pl.sweep3 && !redo) {
    Sweep3Args A3;
    sweep3_args(P, a, pl, A3);
    if (pl.cen3) hipLaunchKernelGGL(k_cen_begin, dim3(1), dim3(1024), 0, P->stream, a, 0);
    void *args[] = {&A3};
    spin_launch(pl.spins[0], P->stream, args);
    if (pl.cen3) hipLaunchKernelGGL(k_cen_end, dim3(64), dim3(256), 0, P->stream, a, 0);
    if (pl.vb_fill) {   // (every launch: idempotent -- after a range redo the fp64 engine has written the same values from the same expression)
      const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
      hipLaunchKernelGGL(k_vb_fill, dim3((unsigned)std::min<int64_t>(1024, (j1 - j0 + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
    }
  }
  if (E.spin < 0) return;
  const SpinLaunch &L = pl.spins[E.spin];
  a.nfeed = E.nfeed; a.lag = E.lag;
  if (E.engine == 4) {
    S2WArgs A; memset(&A, 0, sizeof(A));
    A.winv = P->winv; A.qsum = P->qsumw; A.fx = E.fx; A.nd = E.nd; A.npf = E.npf; A.ahead = E.ahead; A.sub = E.wsub; A.K3 = E.wK3; A.nq = E.nq;
#ifdef BWGR_EXPERIMENTS
    A.dbg = P->data->sw.dbgw;
#endif
    for (int d = 0; d < S2W_MAXDIST; ++d) A.gxt[d] = P->data->gxt[d < P->data->winv_nd ? d : 0];
    if (A.fx) (void)hipMemsetAsync(P->qsumw + (size_t)a.blk_begin * A.nq * 2 * SW_MAXM, 0, sizeof(unsigned long long) * A.nq * 2 * SW_MAXM * (size_t)(a.blk_end - a.blk_begin), P->stream);
    void *args[] = {&a, &A}; spin_launch(L, P->stream, args);
    return;
  }
  if (E.cen >= 0) hipLaunchKernelGGL(k_cen_begin, dim3(1), dim3(1024), 0, P->stream, a, E.cen);
  SweepArgs ak = a;
  if (E.g16) { ak.gramp = P->data->gramp16; ak.gramx = P->data->gramx16; }
  void *args[] = {&ak}; spin_launch(L, P->stream, args);
  if (E.cen >= 0) hipLaunchKernelGGL(k_cen_end, dim3(64), dim3(256), 0, P->stream, a, E.cen);
}
// the plan's sweep alone: the fixed-point engines between a snapshot of the state they start from and the fp64 redo (plan_sweep); no redo
// when the snapshot's scratch cannot be had
static void launch_sweep_kernel(bwgr_panel *P, const SweepArgs &a, const SweepPlan &pl) {
  const size_t p = (size_t)P->data->p;
  bool guarded = pl.guarded;
  if (guarded && !P->snap_e && !P->own.take({{&P->snap_e, sizeof(double) * (size_t)P->data->plan.ld}, {&P->snap_b, sizeof(float) * p}, {&P->snap_d, sizeof(float) * p}, {&P->snap_vb, sizeof(float) * p}})) guarded = false;
  SnapArgs sn;
  sn.e = a.e; sn.se = P->snap_e; sn.b = a.b; sn.d = a.d; sn.vb = (a.flags & SWF_VB_VEC) ? a.vb : nullptr; sn.sb = P->snap_b; sn.sd = P->snap_d; sn.svb = P->snap_vb;
  sn.ld = P->data->plan.ld; sn.j0 = a.blk_begin * a.m; sn.j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m); sn.sc = a.sc;
  if (guarded) hipLaunchKernelGGL(k_range_snapshot, dim3(256), dim3(256), 0, P->stream, sn);
  launch_engine(P, a, pl, false);
  if (guarded) {
    hipLaunchKernelGGL(k_range_recover, dim3(256), dim3(256), 0, P->stream, sn);
    hipLaunchKernelGGL(k_range_flag, dim3(1), dim3(1), 0, P->stream, a.sc);
    (void)reset_exchange(P);
    launch_engine(P, a, pl, true);
    hipLaunchKernelGGL(k_redo_clear, dim3(1), dim3(1), 0, P->stream, a.sc);
  }
}

// d = +1 / -1: a handle moves onto / off stream st, counted where st is one of the data's pair streams.  The count only tells bwgr_chain_run_pair
// which pair stream is idle, so that a pair which forms again does not make a stream each time: sharing one would still be ordered correctly.
// (A paired handle that the caller gives another stream, bwgr_panel_set_stream, stays counted: that pair stream is not reused.)
static void pair_stream_count(PanelData *D, hipStream_t st, int d) {
  for (size_t i = 0; i < D->pair_streams.size(); ++i) if (D->pair_streams[i] == st) D->pair_users[i] += d;
}
// A handle that a pair run moved onto the pair's stream goes back to the stream it had (its own, or the caller's) when it next sweeps alone:
// one wait, on the handle's stream -- nothing is enqueued on the pair stream, which other pairs' hardware queue shares
static int leave_pair_stream(bwgr_panel *P) {
  if (!P->pre_pair_set) return BWGR_OK;
  HIPCHK(hand_over(P->own, &P->handover_ev, P->pre_pair_stream, P->stream));
  pair_stream_count(P->data, P->stream, -1);
  P->stream = P->pre_pair_stream; P->pre_pair_set = false;
  return BWGR_OK;
}
// ---- the launch train -----------------------------------------------------------------------------------------------------------
// A sweep's steps, written once for every caller (launch_sweep for KMUP, wgr and the EM family; bwgr_chain_sweep_blocks; bwgr_chain_run_pair):
// train_begin, the caller's launch_prestage, train_launch, train_end.  A pair differs in two handles, both on the pair's stream, one launch with
// two argument blocks, no redo, and a guard taken once for the run (need).
struct SweepTrain {
  int n = 1;                      // handles: 1 a sweep alone, 2 a pair
  bwgr_panel *P[2] = {}; SweepArgs *a[2] = {}; SweepPlan pl[2];
  int need = 0;                   // compute units the spin launches hold (occupancy guard)
  hipEvent_t ev[2][2] = {};       // per handle: recorded in front of and behind the spin launches (a chain's sweep timing); null: none
  bool draws_next = false;        // a sweep alone: the next iteration's variates beside it (draws_ahead, over the whole panel, behind ev[0][0])
};
// What is done before anything of the sweep is enqueued (a refused sweep leaves the chain as it was): back from a pair's stream, the plan and
// its depth, the affine engine's scratch, the occupancy guard, then the zeroed exchange words
static int train_begin(SweepTrain &t) {
  for (int i = 0; i < t.n; ++i) {
    bwgr_panel *P = t.P[i]; SweepArgs &a = *t.a[i]; SweepPlan &pl = t.pl[i];
    if (t.n == 1) CHK(leave_pair_stream(P));
    pl = plan_sweep(sweep_facts(P), a.flags, a.blk_begin, a.blk_end, t.n == 2 ? SWEEP_PAIR : SWEEP_ALONE); a.lag = pl.run.lag;
    if (pl.engine == 4) CHK(winv_alloc(P));
    if (t.n == 1) CHK(sweep_guard(P, pl, P->stream, nullptr, &t.need));
    CHK(reset_exchange(P));
  }
  return BWGR_OK;
}
// the spin launches between the caller's events, then the variates drawn ahead; what the runtime said of the launches
static hipError_t train_launch(SweepTrain &t) {
  hipStream_t st = t.P[0]->stream;
  Sweep3Args A[2];
  if (t.n == 2) for (int i = 0; i < 2; ++i) {   // the pair's two argument blocks (their slab-dot sums are zeroed in front of the events)
    SweepArgs a = *t.a[i];
    a.gate3 = t.pl[i].gate3;
    if (t.pl[0].withhold || t.pl[1].withhold) a.flags |= SWF_DEBUG_WITHHOLD;
    sweep3_args(t.P[i], a, t.pl[i], A[i]);
  }
  hipError_t he = hipSuccess;
  for (int i = 0; i < t.n; ++i) if (t.ev[i][0] && he == hipSuccess) he = hipEventRecord(t.ev[i][0], st);
  if (he != hipSuccess) return he;
  if (t.n == 2) { void *args[] = {&A[0], &A[1]}; spin_launch(t.pl[0].spins[0], st, args); }
  else launch_sweep_kernel(t.P[0], *t.a[0], t.pl[0]);
  he = hipGetLastError();
  if (he == hipSuccess && t.draws_next) {
    SweepArgs all = *t.a[0]; all.blk_begin = 0; all.blk_end = (int)t.P[0]->data->plan.nblocks;
    draws_ahead(t.P[0], all, t.pl[0], t.ev[0][0]);
  }
  for (int i = 0; i < t.n; ++i) if (t.ev[i][1] && he == hipSuccess) he = hipEventRecord(t.ev[i][1], st);
  return he;
}
static void train_end(SweepTrain &t) { guard_mark(t.P[0], t.P[0]->stream, t.need); }

static int launch_sweep(bwgr_panel *P, SweepArgs &a) {
  SweepTrain t; t.P[0] = P; t.a[0] = &a;
  CHK(train_begin(t));
  P->ps_owner = nullptr;   // the scratch is about to hold this sweep's constants, nobody's iteration
  launch_prestage(P, a, t.pl[0]);
  HIPCHK(train_launch(t));
  train_end(t);
  return BWGR_OK;
}

static void fill_panel_args(const bwgr_panel *P, SweepArgs &a) {
  a.X = P->data->X; a.ld = P->data->plan.ld; a.gram = P->data->gram;
  a.n = (int)P->data->n; a.p = (int)P->data->p; a.m = P->data->plan.m; a.K = P->data->plan.K; a.R = P->data->plan.R;
  a.blk_begin = 0; a.blk_end = (int)P->data->plan.nblocks;
  a.xpart = P->xpart; a.xflags = P->xflags; a.stamps = P->stamps; a.ps = P->ps;
  a.gramx = P->data->gx[1]; a.gramx2 = P->data->gx[2]; a.xspec2 = P->xspec2; a.gramx3 = P->data->gx[3]; a.xspec3 = P->xspec3; a.lag = 2; a.nfeed = P->data->plan.nfeed; a.gramp = P->data->gramp; a.pstride = P->data->plan.pstride; a.qpart = P->qpart; a.dgran = P->dgran;
}
// The arguments of one sweep over the whole of panel P: every byte zero, then the panel's part, the flags, the state the sweep reads and
// writes, the iteration and the generator.  A caller adds only what is its own (a chain its block range, marker0 and the centred fields).
static SweepArgs sweep_args(const bwgr_panel *P, int flags, double *e, float *b, float *d, float *vb, const float *xx, const float *lam,
                            ChainScalars *sc, uint32_t iter, const Rng &rng) {
  SweepArgs a; memset(&a, 0, sizeof(a));
  fill_panel_args(P, a);
  a.flags = flags;
  a.e = e; a.b = b; a.d = d; a.vb = vb; a.xx = xx; a.lam = lam; a.sc = sc;
  a.iter = iter; a.rng = rng;
  return a;
}

// the plan of a sweep alone over the whole of panel P, as it stands now (clones alive, centred or not), for the entries that answer from a plan
static SweepPlan plan_whole_panel(const bwgr_panel *P, bool selection) {
  const int flags = selection ? (SWF_SELECT | (P->data->cen ? SWF_CENTRE : 0)) : 0;
  return plan_sweep(sweep_facts(P), flags, 0, (int)P->data->plan.nblocks, SWEEP_ALONE);
}

// chains (one per panel or clone) whose sweep kernels fit the chip side by side: each takes nwg + 1 (+ feeders) CUs
extern "C" int bwgr_panel_max_concurrent(const bwgr_panel *P, int selection, int *count) {
  if (!P || !count) return fail(BWGR_EINVAL, "null pointer");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, P->data->device));
  const SweepPlan pl = plan_whole_panel(P, selection != 0);
  // selection on a panel with k_sweep3: the device sends a chain above the engine threshold to k_sweep2 (K + 1 + feeders), and a sweep that
  // leaves the fixed-point range is redone there: the larger of the two (K3 + 1: the streamers of chains side by side, never the solo ones)
  int wgs = P->data->plan.K + 1 + pl.run.nfeed;
  if (pl.engine == 3) wgs = std::max(P->data->plan3.K3 + 1, wgs);
  if (pl.engine == 4) wgs = pl.spins[0].resident;   // streamers, sequencer, L2 prefetchers (the launch's other workgroups leave at once)
  // one sweep workgroup per CU even where the LDS would admit two (small blocks): measured, sharing a CU costs more than it adds
  *count = std::max(1, prop.multiProcessorCount / wgs);
  if (P->data->sw.max_concurrent > 0) *count = P->data->sw.max_concurrent;   // experiments
  return BWGR_OK;
}

// pairs of chains (bwgr_chain_run_pair) that fit side by side: a pair's launch holds K3 + 2 compute units, and about 40 stay free for the
// iterations' small kernels (six pairs at C4 measured slower than five); 0 on a panel without k_sweep3.  BWGR_MAX_PAIRS overrides.
extern "C" int bwgr_panel_max_pairs(const bwgr_panel *P, int *pairs) {
  if (!P || !pairs) return fail(BWGR_EINVAL, "null pointer");
  *pairs = 0;
  if (!P->data->e3_ready || s3p_streamer_lds(P->data->plan3.R3) > (size_t)160 * 1024) return BWGR_OK;
  const int cus = device_cus(P->data->device);
  if (cus < 1) return fail(BWGR_EHIP, "panel_max_pairs: no device properties");
  *pairs = std::max(1, (cus - 40) / (P->data->plan3.K3 + 2));
  if (P->data->sw.max_pairs > 0) *pairs = P->data->sw.max_pairs;
  return BWGR_OK;
}

// Test hook for the abort path: while on != 0 every sweep launched on this panel runs with slab workgroup 0 absent, so the
// workgroups that wait for it spin to their wall-clock bound, raise the shared abort word and the launch reports BWGR_ETIMEOUT.
extern "C" int bwgr_debug_withhold(bwgr_panel *P, int on) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  P->debug_withhold = on ? 1 : 0;
  return BWGR_OK;
}

// Which instantiation of the trajectory engine a selection sweep of the whole panel, as it stands now (clones alive, centred or not), is launched as:
// 0 none (the panel's selection sweeps are not k_sweep3's), 1 k_sweep3 / k_sweep3p, 2 k_sweep3f.  For the tests.
extern "C" int bwgr_debug_sweep3_kernel(const bwgr_panel *P, int *which) {
  if (!P || !which) return fail(BWGR_EINVAL, "null pointer");
  const SweepPlan pl = plan_whole_panel(P, true);
  *which = pl.engine != 3 ? 0 : (pl.fixed3 ? 2 : 1);
  return BWGR_OK;
}

extern "C" int bwgr_panel_pipeline(const bwgr_panel *P, int selection, int info[4]) {
  if (!P || !info) return fail(BWGR_EINVAL, "null pointer");
  const SweepPlan pl = plan_whole_panel(P, selection != 0);
  info[0] = pl.engine;
  info[1] = pl.engine == 3 ? P->data->plan3.D : pl.run.lag;
  info[2] = pl.engine == 3 ? 0 : pl.run.nfeed;
  info[3] = P->data->is_f32 ? 0 : (P->data->gram16 ? 16 : 32);
  return BWGR_OK;
}
