// bwgr_amd/csrc/panel_plan.hip.h -- what a panel is, decided once: PanelPlan / Panel3Plan, their planners plan_panel / plan_panel3 and the
// hook bwgr_debug_panel_plan.  Host arithmetic on the kernels' LDS-size functions, no device.  Part of bwgr_hip.hip, which includes it after the
// error plumbing and switches.h and in front of the handle structs, which hold the plans by value (the rest of the panel's host code, which needs
// the handles, is panel_host.hip.h).
// ---- the panel plan ----------------------------------------------------------------------------------------------------------
// What a panel is -- its block and slab geometry, whether the pipelined engine fits it, which Gram arrays it carries -- is one decision, made by
// plan_panel from the shape, the kind of panel and the switches: host arithmetic, no device (bwgr_debug_panel_plan() exposes it to the CPU
// tests).  panel_alloc allocates what the plan lists; nothing writes to a plan afterwards.  Kinds -- main: bwgr_panel_create's; rows: a row subset
// of one, refilled per call or per iteration (KMUP2, wgr's bagging): no k_sweep3, no far byte planes; em: bwgr_em's shuffled copy: lag 2 on the 32-bit blocks
enum PanelKind { PANEL_MAIN = 0, PANEL_ROWS = 1, PANEL_EM = 2 };
struct PanelPlan {
  int m = 0, K = 0, R = 0;    // markers per block; slab workgroups, rows of each
  int64_t ld = 0, nblocks = 0;
  int pstride = 0, nfeed = 2; // nfeed: q feeder workgroups of k_sweep2 (one gather + sum of K KB takes about a block period at K = 40)
  bool lag4_ok = false;       // the lag-4 streamer (ring of four tiles) fits the LDS at this geometry
  size_t lds = 0, lds2 = 0, ldsw = 0;   // dynamic LDS of k_sweep, k_sweep2, k_sweep2w
  size_t x_bytes = 0, gram_bytes = 0;   // (gram_bytes: per Gram array -- the diagonal blocks, the cross blocks of one distance)
  bool pipelined = false;     // the streamer / sequencer pipeline (k_sweep2 and what builds on it); false: the replicated recurrence (k_sweep)
  int xdist = 1;              // cross Gram arrays gx[1..xdist]: distance 2 for the lag-3 pipeline, 3 for the lag-4 one
  bool has16 = false;         // the 16-bit copies gramp16 / gramx16 for the sequencer (int8 panels)
  int wdist = 0;              // the affine engine's byte planes gxt[] may reach this distance (where every near entry fits 16 bits)
  bool try3 = false;          // k_sweep3 is attempted once the data is there (plan_panel3)
};
template <typename XT> static int max_slab_rows(int m) {
  int best = 0;
  for (int R = 128; R <= 4096; R += 128)
    if (sweep_lds_bytes<XT>(m, R) <= (size_t)160 * 1024 && (size_t)m * R * sizeof(XT) <= (size_t)SW_TCH * 16 * (SW_THREADS - 64)) best = R;
  return best;
}
static int panel_range(int64_t n, int64_t p) {
  if (n < 2 || p < 1) return fail(BWGR_EINVAL, "panel: need n >= 2, p >= 1 (n=%lld p=%lld)", (long long)n, (long long)p);
  if (n > 0x7FFFFF00ll || p > 0x7FFFFF00ll) return fail(BWGR_EINVAL, "panel: n and p must fit 31 bits");
  return BWGR_OK;
}
static int plan_panel(PanelPlan &pl, bool is_f32, int64_t n, int64_t p, int block, int nwg, PanelKind kind, const Switches &sw) {
  pl = PanelPlan();
  CHK(panel_range(n, p));
  const auto lds2_of = [&](int m, int R) { return is_f32 ? sweep2_lds_bytes<float>(m, R) : sweep2_lds_bytes<int8_t>(m, R); };
  const int mmax = is_f32 ? 64 : SW_MAXM;
  int m = block > 0 ? block : mmax;
  if (m > mmax) return fail(BWGR_EINVAL, "panel_create: block %d > %d (limit for this genotype type)", m, mmax);
  m = ((int)std::min<int64_t>(m, ((p + 15) / 16) * 16) + 15) / 16 * 16;
  const int Rmax = is_f32 ? max_slab_rows<float>(m) : max_slab_rows<int8_t>(m);
  // the pipelined engine keeps three tiles per streamer, so it takes fewer rows per slab than k_sweep at small blocks:
  // prefer the largest slab it fits (unless that needs more workgroups than the chip has CUs, or k_sweep is forced)
  int Rpick = Rmax, R2 = 0;
  for (int Rt = 128; Rt <= Rmax; Rt += 128)
    if (lds2_of(m, Rt) <= (size_t)160 * 1024 && (is_f32 || (size_t)m * Rt <= S2I_TILE_BYTES_MAX)) R2 = Rt;   // (an int8 tile must fit its movers' registers)
  if (sw.sweep != '1' && R2 > 0 && (n + R2 - 1) / R2 + 1 + 6 <= 256) Rpick = R2;
  const int K = nwg > 0 ? nwg : (int)((n + Rpick - 1) / Rpick);
  const int R = (int)((((n + K - 1) / K) + 127) / 128) * 128;
  if (K > 256 || R > Rmax) return fail(BWGR_EINVAL, "panel_create: n=%lld needs %d slab workgroups of %d rows (limits: 256 workgroups, %d rows)", (long long)n, K, R, Rmax);
  pl.m = m; pl.K = K; pl.R = R; pl.ld = (int64_t)K * R;
  pl.nblocks = (p + m - 1) / m;
  if (pl.nblocks >= (1ll << 24)) return fail(BWGR_EINVAL, "panel_create: %lld marker blocks; the delta granules carry a 24-bit block epoch", (long long)pl.nblocks);
  pl.pstride = ((m * (m - 1) / 2 + 7) / 8) * 8;
  pl.lds = is_f32 ? sweep_lds_bytes<float>(m, R) : sweep_lds_bytes<int8_t>(m, R);
  pl.lds2 = lds2_of(m, R);
  pl.lag4_ok = !is_f32 && s2i_lds_bytes(m, R, 4) <= (size_t)160 * 1024;
  if (pl.lag4_ok) pl.lds2 = std::max(pl.lds2, s2i_lds_bytes(m, R, 4));
#ifdef BWGR_EXPERIMENTS
  if (!is_f32) pl.ldsw = s2w_lds_bytes(m, R, sw.wlag_timing ? sw.wlag_timing : 6);
#else
  if (!is_f32) pl.ldsw = s2w_lds_bytes(m, R, 6);
#endif   // (room for the deepest pipeline BWGR_WLAG can ask for)
  pl.nfeed = std::min(6, std::max(2, (K + 39) / 40 + 1));   // K = 40: 2, K = 79: 3, K >= 161: 6
  if (sw.nfeed >= 1 && sw.nfeed <= 6) pl.nfeed = sw.nfeed;   // experiments
  // BWGR_SWEEP=1: the A/B switch for tests and profiling; else the pipeline wherever its LDS, its grid and (int8) its movers' registers fit
  pl.pipelined = sw.sweep != '1' && pl.lds2 <= (size_t)160 * 1024 && K + 1 + pl.nfeed <= 256 && (is_f32 || (size_t)m * R <= S2I_TILE_BYTES_MAX);
  pl.x_bytes = (size_t)pl.ld * (size_t)p * (is_f32 ? 4 : 1);
  pl.gram_bytes = (size_t)pl.nblocks * m * m * (is_f32 ? 8 : 4);
  if (pl.pipelined && kind != PANEL_EM) {
    if (pl.nblocks > 2) pl.xdist = 2;
    if (!is_f32 && pl.nblocks > 3 && pl.lag4_ok && sw.lag != '2' && sw.lag != '3') pl.xdist = 3;
    pl.has16 = !is_f32;
  }
  // the byte planes: the near distances from the arrays above, distances 4 and 5 (pipelines five and six blocks deep, BWGR_WLAG) on main panels only
  if (pl.has16 && sw.winv && m <= SW_MAXM)
    for (int d = 1; d <= S2W_MAXDIST && d < pl.nblocks; ++d) {
      if (d <= S2W_NEARD ? d > pl.xdist : (kind != PANEL_MAIN || d > sw.wlag_cap - 1)) break;
      pl.wdist = d;
    }
  pl.try3 = kind == PANEL_MAIN && !is_f32 && pl.pipelined && sw.sweep != '2';   // (BWGR_SWEEP=2 keeps k_sweep2)
  return BWGR_OK;
}

// k_sweep3's share (selection models on int8 panels, sweep3.hip.h), planned once the data is on the device: from the panel plan and whether
// every near Gram entry fits 16 bits (the largest |x| sizes the integer slab-dot sums, which every int8 panel the geometry takes fits: see below)
struct Panel3Plan {
  bool fits = false;
  int R3 = 0, sub3 = 0, K3 = 0;   // rows of a streamer workgroup, streamers per slab, streamer workgroups
  int D = 0;                  // fold-in lag in blocks; cross Gram arrays reach D-1 blocks back
  size_t lds3 = 0;
  bool solo3 = true;          // a chain alone on the GPU runs 128-row streamers (BWGR_SOLO3=0: never)
};
static Panel3Plan plan_panel3(const PanelPlan &pp, const Switches &sw, bool gram16) {
  Panel3Plan q;
  if (!pp.try3) return q;
  q.R3 = (pp.R % 256 == 0) ? 256 : 128;
  if ((sw.r3 == 64 || sw.r3 == 128 || sw.r3 == 256) && pp.R % sw.r3 == 0) { q.R3 = sw.r3; q.solo3 = false; }   // (an explicit height holds for every launch)
  q.sub3 = pp.R / q.R3; q.K3 = pp.K * q.sub3;
  q.D = 12;   // (the streamers fold a list whose words they saw a step ahead: more lag than the fold itself needs -- C4: 12.45 ms at 8, 11.27 at 9, 10.78 at 10, 10.41 at 11, 10.37 at 12, 10.48 at 13)
  // (at least 2: a block's list leaves the sequencer while the next block is in its rounds)
  if (sw.d3 >= 2 && sw.d3 <= S3_MAXD) q.D = sw.d3;
  q.D = (int)std::min<int64_t>(q.D, std::max<int64_t>(2, pp.nblocks));
  q.lds3 = std::max(std::max(s3_streamer_lds(q.R3), std::max(s3_streamer_dma_lds(128), q.R3 == 256 ? s3_streamer_dma_lds(256) : (size_t)0)), s3_seq_lds(q.D, gram16));
  // the slab dots are summed as integers: sum over all rows of |x| * 128 per digit, four digits of 8 bits, 8 bits of arrival count, which
  // asks for ld * xmax < 2^23.  No condition on xmax: K3 <= 255 streamers of R3 <= 256 rows are ld <= 65 280 rows, and 65 280 * 128 < 2^23
  q.fits = q.K3 <= 255 && q.lds3 <= (size_t)160 * 1024 && (size_t)pp.m * q.R3 <= (size_t)4 * 16 * SW_THREADS;
  if (q.fits && sw.solo3 >= 0) q.solo3 = sw.solo3 != '0';
  return q;
}

// The plans without a device (test hook): plan_panel with the switches of the environment, as bwgr_panel_create reads them, and -- given an
// assumed xmax >= 0 and 16-bit verdict -- plan_panel3.  out: see include/bwgr.h.
extern "C" int bwgr_debug_panel_plan(int is_f32, int64_t n, int64_t p, int block, int nwg, int kind, int xmax, int gram16, int64_t out[BWGR_PANEL_PLAN_NOUT]) {
  if (!out || kind < PANEL_MAIN || kind > PANEL_EM) return fail(BWGR_EINVAL, "debug_panel_plan: null pointer or bad kind");
  const Switches sw = read_switches();
  PanelPlan pl;
  CHK(plan_panel(pl, is_f32 != 0, n, p, block, nwg, (PanelKind)kind, sw));
  const Panel3Plan q = xmax >= 0 ? plan_panel3(pl, sw, gram16 != 0) : Panel3Plan();   // (xmax: only whether the data is assumed known)
  const int64_t v[BWGR_PANEL_PLAN_NOUT] = {pl.m, pl.K, pl.R, pl.ld, pl.nblocks, pl.pstride, pl.nfeed, pl.lag4_ok, (int64_t)pl.lds, (int64_t)pl.lds2, (int64_t)pl.ldsw,
                                           (int64_t)pl.x_bytes, (int64_t)pl.gram_bytes, pl.pipelined, pl.xdist, pl.has16, pl.wdist, pl.try3,
                                           q.fits, q.R3, q.sub3, q.K3, q.D, (int64_t)q.lds3, q.solo3};
  std::copy(v, v + BWGR_PANEL_PLAN_NOUT, out);
  return BWGR_OK;
}
