// bwgr_amd/csrc/bwgr_hip.hip -- libbwgr_hip.so, the one translation unit of the C ABI (include/bwgr.h).  This file holds what every family
// shares on the host: error plumbing, the switches, the panel plans, the HIP backend of the holder, the handles and their small helpers, the
// occupancy guard, a sweep's planning and launching, the panel entries, the launch rules of X * coef and the test hooks.  It defines no kernel
// and no family's entry point: the kernels are the *.hip.h files included at the top, the entries the *_host.hip.h files included near the end.
// gfx950 only; there is no CPU path in this library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <string.h>
#include <math.h>
#include <vector>
#include <random>
#include <chrono>
#include <algorithm>
#include <mutex>
#include <atomic>
#include <memory>
#include <utility>
#include <type_traits>
#include "../../include/bwgr.h"
#include "devbufs.h"
#include "traits.h"
#include "csc.h"
#include "rng.hip.h"
#include "sweep.hip.h"
#include "sweep3.hip.h"
#include "sweep2w.hip.h"
#include "sweep3p.hip.h"
#include "mrr.hip.h"
#include "mrr_dense.hip.h"
#include "uvb.hip.h"
#include "uvbd.hip.h"
#include "uvb2.hip.h"
#include "pegs.hip.h"
#include "pegsx.hip.h"
#include "pegs_sparse.hip.h"
#include "pegsx_setup.h"
#include "kernels.hip.h"
#include <stdlib.h>

using namespace bwgr;

// the kernels around the sweep, by family (each says in its header what it holds); the host entries that launch them are included further
// down, where everything they use is defined
#include "panel.hip.h"
#include "chain.hip.h"
#include "wgr.hip.h"
#include "em.hip.h"

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(BWGR_EHIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define CHK(x) do { int r_ = (x); if (r_ != BWGR_OK) return r_; } while (0)

// the status a sweep kernel left in ChainScalars::error
static int sweep_error(uint32_t code, const char *who) {
  // (since round 3 a sweep that leaves the range is redone on the fp64 residual, k_range_recover: this status only surfaces where no fallback
  // is queued -- chains advanced in pairs)
  if (code == 2u) return fail(BWGR_ERANGE, "%s: the residual left the fixed-point range of the sweep (it grew beyond the grid's headroom, about a thousandfold of its starting scale, within one sweep); the chain state is invalid", who);
  return fail(BWGR_ETIMEOUT, "%s: a workgroup exchange timed out inside the sweep kernel (the chain state is invalid)", who);
}
extern "C" const char *bwgr_last_error(void) { return g_err; }
extern "C" int bwgr_abi_version(void) { return BWGR_ABI_VERSION; }
extern "C" int bwgr_device_count(int *count) {
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
  if (count) *count = c;
  return BWGR_OK;
}


// ------------------------------------------------------------------------------------------------
// host objects
// ------------------------------------------------------------------------------------------------

// ------------------------------------------------------------------------------------------------
// The environment switches, every one the library reads, read once: when a root panel is made.  Clones share the
// root's; the scratch panels of KMUP2, bagging and the EM family, and groups take the panels' they are made for.  First-character switches
// hold that character (-1: unset); numeric ones hold their value as parsed (0: unset); the rest their parsed meaning.
struct Switches {
  int sweep = -1, lag = -1, solo3 = -1, stream3 = -1, pf3 = -1;                  // BWGR_SWEEP, BWGR_LAG, BWGR_SOLO3, BWGR_STREAM3, BWGR_PF3
  int r3 = 0, d3 = 0, nfeed = 0, sh_add = 0, max_concurrent = 0, max_pairs = 0;  // BWGR_R3, BWGR_D3, BWGR_NFEED, BWGR_DEBUG_SH_ADD, BWGR_MAX_CONCURRENT, BWGR_MAX_PAIRS
  // BWGR_ENG3_THR: k_sweep3 takes the sweeps whose chains hold fewer than this share of markers in the model; measured crossover at n = 10 000:
  // us per block at 1.4 / 3.7 / 5.8 / 10.9 % inclusion: k_sweep3 2.26 / 3.73 / 5.56 / 12.1, k_sweep2 3.07 / 3.29 / 3.60 / 4.69
  float eng3_thr = 0.03f;
  bool occ_guard = true, pf3b = true, draws = true, gram16 = true;   // BWGR_OCC_GUARD=0, BWGR_PF3B=0, BWGR_DRAWS=0, BWGR_GRAM16=0 switch these off
  // BWGR_WINV=0: the serial recurrence of k_sweep2's sequencer instead of k_sweep2w; BWGR_WFX=0: k_sweep2's streamers under its product sequencer
  // instead of the fixed-point ones; BWGR_WPF / BWGR_WAHEAD / BWGR_WNQ (0: by the streamer count) / BWGR_WLAG (=5|6: distances 4 / 5 through LDS
  // planes -- measured slower: C4-shape BayesA 22.3 / 23.0 / 24.9 ms per sweep at depth 4 / 5 / 6)
  bool winv = true, wfx = true;
  // BWGR_FIXED3=0: k_sweep3 also where a launch matches k_sweep3f, the fixed-shape instantiation (plan_sweep).  The experiment build (-DBWGR_EXPERIMENTS)
  // takes k_sweep3f only when asked, BWGR_FIXED3=1: tools/ab3_probe.py times either one under the BWGR_DBG3 switches.
#ifdef BWGR_EXPERIMENTS
  bool fixed3 = false;
#else
  bool fixed3 = true;
#endif
  int wpf = 4, wahead = 5, wnq = 0, wlag_cap = 4;
  bool group_allow_uncentred = false, group_force_comm = false, em_debug = false;   // BWGR_GROUP_ALLOW_UNCENTRED=1, BWGR_GROUP_FORCE_COMM=1, BWGR_EM_DEBUG
  int64_t kchunk = 0;   // BWGR_KCHUNK: markers per int32 chunk of the X X' product (0: the largest that keeps the int32 sums exact, plan_xxt)
#ifdef BWGR_EXPERIMENTS
  int dbg3 = 0, dbgw = 0, wlag_timing = 0; bool no_recover = false;   // BWGR_DBG3, BWGR_DBGW, BWGR_WLAG_TIMING, BWGR_NO_RECOVER
#endif
};
static Switches read_switches() {
  const auto chr = [](const char *v) { return v ? (int)(unsigned char)v[0] : -1; };
  const auto num = [](const char *v) { return v ? atoi(v) : 0; };
  Switches s;
  s.sweep = chr(getenv("BWGR_SWEEP")); s.lag = chr(getenv("BWGR_LAG")); s.solo3 = chr(getenv("BWGR_SOLO3"));
  s.stream3 = chr(getenv("BWGR_STREAM3")); s.pf3 = chr(getenv("BWGR_PF3"));
  s.r3 = num(getenv("BWGR_R3")); s.d3 = num(getenv("BWGR_D3")); s.nfeed = num(getenv("BWGR_NFEED")); s.sh_add = num(getenv("BWGR_DEBUG_SH_ADD"));
  s.max_concurrent = num(getenv("BWGR_MAX_CONCURRENT")); s.max_pairs = num(getenv("BWGR_MAX_PAIRS"));
  if (const char *v = getenv("BWGR_ENG3_THR")) { const float t = (float)atof(v); if (t > 0.0f) s.eng3_thr = t; }
  s.occ_guard = chr(getenv("BWGR_OCC_GUARD")) != '0'; s.pf3b = chr(getenv("BWGR_PF3B")) != '0'; s.draws = chr(getenv("BWGR_DRAWS")) != '0';
  s.gram16 = chr(getenv("BWGR_GRAM16")) != '0';
  { const int c = chr(getenv("BWGR_FIXED3")); if (c == '0') s.fixed3 = false; else if (c == '1') s.fixed3 = true; }
  s.winv = chr(getenv("BWGR_WINV")) != '0'; s.wfx = chr(getenv("BWGR_WFX")) != '0';
  if (const char *v = getenv("BWGR_WPF")) s.wpf = std::max(0, std::min(8, atoi(v)));
  if (const char *v = getenv("BWGR_WAHEAD")) s.wahead = std::max(1, atoi(v));
  { const int v = num(getenv("BWGR_WNQ")), c = chr(getenv("BWGR_WLAG")); if (v == 1 || v == 2 || v == 4) s.wnq = v; if (c >= '2' && c <= '6') s.wlag_cap = c - '0'; }
  s.group_allow_uncentred = chr(getenv("BWGR_GROUP_ALLOW_UNCENTRED")) == '1'; s.group_force_comm = chr(getenv("BWGR_GROUP_FORCE_COMM")) == '1';
  s.em_debug = getenv("BWGR_EM_DEBUG") != nullptr;
  if (const char *v = getenv("BWGR_KCHUNK")) s.kchunk = std::max<long long>(0, atoll(v));
#ifdef BWGR_EXPERIMENTS
  s.dbg3 = num(getenv("BWGR_DBG3")); s.dbgw = num(getenv("BWGR_DBGW")); s.wlag_timing = num(getenv("BWGR_WLAG_TIMING"));
  s.no_recover = getenv("BWGR_NO_RECOVER") != nullptr;
#endif
  return s;
}

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

// The HIP backend of the holder (devbufs.h), and the only place of this library that allocates or frees device memory.  Its counts are what
// bwgr_debug_live reports: the arrays, streams and events that holders own in this process.
namespace {
struct HipBackend {
  using stream_t = hipStream_t;
  using event_t = hipEvent_t;
  static inline std::atomic<int64_t> live[3];
  static inline thread_local hipError_t last = hipSuccess;   // what the calling thread's last failed alloc() got: the text of its failure
  static void *alloc(size_t bytes) {
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) { last = e; (void)hipGetLastError(); return nullptr; }
    ++live[0];
    return q;
  }
  static void free(void *q) { (void)hipFree(q); --live[0]; }
  static bool stream_create(hipStream_t *s, unsigned flags, int priority) {
    if ((priority ? hipStreamCreateWithPriority(s, flags, priority) : hipStreamCreateWithFlags(s, flags)) != hipSuccess) { (void)hipGetLastError(); return false; }
    ++live[1];
    return true;
  }
  static void stream_sync(hipStream_t s) { (void)hipStreamSynchronize(s); }
  static void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); --live[1]; }
  static bool event_create(hipEvent_t *e, unsigned flags) {
    if (hipEventCreateWithFlags(e, flags) != hipSuccess) { (void)hipGetLastError(); return false; }
    ++live[2];
    return true;
  }
  static void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); --live[2]; }
};
// The device arrays, streams and events of one call (or of one block of it), or of one handle.  get() returns nullptr where the allocation
// fails, and the holder remembers it: the caller reports BWGR_ENOMEM, "<entry>: device allocation failed" (own_array below does; an entry
// of the *_host.hip.h files asks failed() once after the last get of a group).
using DevBufs = DevHolder<HipBackend>;
// Runs f when the scope ends, unless release()d: destroys the object a function is making on its error returns, a call's scratch panels and
// chains on every return, and gives a borrowed stream back.  Declared before the call's DevBufs, so that it runs after the buffers are freed.
template <typename F> struct Guard {
  F f;
  bool armed = true;
  explicit Guard(F f_) : f(f_) {}
  Guard(const Guard &) = delete;
  ~Guard() { if (armed) f(); }
  void release() { armed = false; }
};
}  // namespace
extern "C" int bwgr_debug_live(int64_t out[3]) {
  if (!out) return fail(BWGR_EINVAL, "debug_live: null pointer");
  for (int i = 0; i < 3; ++i) out[i] = HipBackend::live[i].load();
  return BWGR_OK;
}
// a handle's allocation failed: BWGR_ENOMEM, with what the runtime said
static int no_memory(const char *who) { return fail(BWGR_ENOMEM, "%s: device allocation failed (%s)", who, hipGetErrorString(HipBackend::last)); }
// ptr = count elements (bytes, of a void pointer) that `own` owns from now on
template <typename T> static int own_array(DevBufs &own, T *&ptr, size_t count, const char *who) {
  return (ptr = own.get<std::conditional_t<std::is_void<T>::value, unsigned char, T>>(count)) ? BWGR_OK : no_memory(who);
}

// ------------------------------------------------------------------------------------------------
// A resident panel is its data (PanelData) and the handles on it (bwgr_panel).  The root handle is made with the data -- by
// bwgr_panel_create, or as a scratch panel of KMUP2, wgr or bwgr_em -- and frees it; a clone (bwgr_panel_clone) is another handle on the
// same data.  Every handle owns its streams and the scratch its sweeps write.  The data does not change while a clone is alive: it is
// built with the root, and bwgr_panel_set_centred refuses on a clone and while any chain is alive.
// Each of PanelData, bwgr_panel, bwgr_chain and bwgr_group owns its device arrays, streams and long-lived events through a holder (`own`);
// the typed pointers below are aliases, and deleting the struct releases them.  What is allocated lazily as a group is one take().
struct PanelData {
  DevBufs own;                // the genotypes, the Gram family, the statistics, csum / xxc and the pair streams
  int device = 0, is_f32 = 0;
  int64_t n = 0, p = 0;
  PanelPlan plan;             // made with the data (plan_panel)
  Panel3Plan plan3;           // made when the data is built (sweep3_build)
  // what the build found in the data (panel_setup once; panel_build_gram again wherever a scratch panel's rows or columns change)
  float MSx = 0;
  int xmax = 0;               // largest |x| of an int8 panel
  bool gram16 = false;        // the 16-bit copies are exact: every entry in 0..65535
  int winv_nd = 0;            // gxt distances built = the deepest lag the affine sweeps can run, minus one
  bool e3_ready = false;      // this panel has k_sweep3: plan3 fits and every far Gram block fits the staging's element type
  bool crowded = false;       // a shard among three or more on one device: never the solo streamers (bwgr_group_create)
  void *X = nullptr, *gram = nullptr, *gramp = nullptr;
  void *gx[S2W_NEARD + 1] = {};   // gx[d], d = 1 .. plan.xdist: cross Gram blocks X_{b-d}' X_b, int32 (fp64 for float panels)
  uint16_t *gramp16 = nullptr, *gramx16 = nullptr;   // 16-bit copies of gramp and gx[1] (plan.has16)
  int *gram16_bad = nullptr;
  // g3x[d-1]: cross Gram blocks of distance d in the element type k_sweep3 reads: an alias of the panel's array of that distance and type, or an array of its own
  void *g3x[S3_MAXD] = {};
  unsigned char *gx12 = nullptr;   // 16-bit panels: an included marker's distance-1 and distance-2 rows side by side (k_near_rows)
  unsigned char *gxt[S2W_MAXDIST] = {};   // the affine models' cross Gram blocks as the sequencer's MFMA operand (k_gx_planes, sweep2w.hip.h)
  float *xx = nullptr, *vx = nullptr;
  int *xmax_dev = nullptr;
  // implicitly centred columns (bwgr_panel_set_centred; int8 panels with k_sweep3): the column sums, the centred |x_j - mean_j|^2 as floats (what
  // a chain's xx is then)
  bool cen = false;
  int32_t *csum = nullptr; float *xxc = nullptr;
  Switches sw;                // read when the root panel is made
  int nclones = 0;            // live clones: the root's bwgr_panel_destroy refuses while any is alive
  int nchains_all = 0;        // live chains on every handle (bwgr_panel_set_centred refuses while any is alive)
  std::vector<hipStream_t> pair_streams;   // the streams pairs of chains run on (bwgr_chain_run_pair); here, so that they outlive every clone
};

struct bwgr_panel {
  PanelData *data = nullptr;
  bool is_root = false;       // made with the data, which it frees; false: a clone
  DevBufs own;                // the sweep scratch, the exchange words, the lazy groups, a clone's stream, the draws stream and events
  hipStream_t stream = nullptr;
  hipStream_t pre_pair_stream = nullptr; bool pre_pair_set = false;   // the stream this handle ran on before a pair run moved it (restored by its next sweep alone)
  // the sweep scratch (scratch_alloc, and what the first sweep that needs it takes)
  double *xspec2 = nullptr, *xspec3 = nullptr;   // [nblocks][SW_MAXM]: speculative cross terms of the lag-3 / lag-4 pipelines (k_spec)
  PreStage ps = {};
  const void *ps_owner = nullptr; int ps_iter = -1;   // whose sweep constants the scratch holds (a chain pre-stages a whole iteration once)
  double *xpart = nullptr, *qpart = nullptr;
  unsigned long long *dgran = nullptr;
  uint32_t *xflags = nullptr;
  unsigned char *xchg = nullptr; size_t xchg_bytes = 0;   // xflags | dgran | qpart in one allocation: one memset per launch
  unsigned long long *stamps = nullptr;   // diagnostic build only
  unsigned long long *qsum3 = nullptr, *lists3 = nullptr;   // k_sweep3's slab-dot sums and block lists
  uint32_t epoch3 = 0;
  double *snap_e = nullptr; float *snap_b = nullptr, *snap_d = nullptr, *snap_vb = nullptr;   // state before a fixed-point sweep (range recovery)
  double *winv = nullptr;     // [nblocks][S2W_WDOUBLES], written by k_affine_inv before every affine sweep (sweep2w.hip.h)
  unsigned long long *qsumw = nullptr;   // the fixed-point streamers' slab-dot sums [nblocks][SW_MAXM][2]
  double *cpre = nullptr;     // implicitly centred columns: the running block sums of s_k * drej_k of the current iteration
  // k_draws: the next iteration's state-independent variates, drawn on a second (low-priority) stream beside this iteration's sweep
  double *draws = nullptr; hipStream_t draws_stream = nullptr; hipEvent_t draws_ready = nullptr, draws_free = nullptr;
  bool draws_valid = false; Rng draws_rng = {}; uint32_t draws_iter = 0, draws_marker0 = 0; int draws_flags = 0, draws_j0 = 0, draws_j1 = 0; const void *draws_sc = nullptr;
  // occupancy guard: the compute units this handle's enqueued sweeps hold while they run, the stream they run on, and an event behind the last of them
  hipEvent_t guard_ev = nullptr; int guard_cus = 0; hipStream_t guard_stream = nullptr; bool guard_listed = false;
  bool force3 = false;        // a pair run (bwgr_chain_run_pair): every selection sweep is k_sweep3's, whatever the inclusion rate
  int debug_withhold = 0;     // test hook: the next sweeps run with slab workgroup 0 missing (bwgr_debug_withhold)
  int nchains = 0;            // live chains on this handle: panel_destroy refuses while any is alive
};

struct bwgr_chain {
  bwgr_panel *P = nullptr;
  DevBufs own;                        // the state arrays (e: unless the caller gave one)
  int model = 0, iit = 0, ibi = 0, done = 0, rng_mode = 0;
  float itf = 0, bif = 0, pi = 0, df = 0, R2 = 0, Phi = 0;
  uint64_t seed = 0;
  float *y = nullptr, *b = nullptr, *d = nullptr, *vb = nullptr, *lam = nullptr;
  double *e = nullptr;
  float *B = nullptr, *D = nullptr, *VB = nullptr;
  ChainScalars *sc = nullptr;
  int64_t marker0 = 0, p_total = 0;   // sharding: global id of local marker 0, markers over all ranks
  float MSx_eff = 0;                  // MSx over all ranks
  double *e0 = nullptr;               // residual at the start of the current exchange round (sharded stepping)
  int flags_extra = 0;                // two-effect BayesB2: SWF_ALT_B2 (the likelihood comparison uses the drawn alternative)
  std::vector<hipEvent_t> ev;  // pairs around each sweep launch since the last query
  float ms_acc = 0; int launch_acc = 0;
  bool finalized = false;
};

// Concurrent chains (bwgr_panel_clone) want one hardware queue per stream; the runtime's default is four.  Set before the
// first HIP call of the process unless the user chose a value.
__attribute__((constructor)) static void bwgr_more_hw_queues() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

// device -> host copy ordered on the panel's stream (which may be a non-blocking one: the null stream does not wait for it)
static hipError_t d2h(hipStream_t st, void *dst, const void *src, size_t bytes) {
  hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
// host -> device and device -> device copies of count elements, and count elements set to zero bytes, all enqueued on st
template <typename T> static hipError_t h2d(hipStream_t st, T *dst, const T *src, size_t count) { return hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, st); }
template <typename T> static hipError_t d2d(hipStream_t st, T *dst, const T *src, size_t count) { return hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToDevice, st); }
template <typename T> static hipError_t zero(hipStream_t st, T *dst, size_t count) { return hipMemsetAsync(dst, 0, sizeof(T) * count, st); }

static Rng make_rng(uint64_t seed, int mode) {
  Rng g; g.k0 = (uint32_t)seed; g.k1 = (uint32_t)(seed >> 32); g.degenerate = (mode == BWGR_RNG_DEGENERATE); return g;
}

// *sum = the sum of the n floats of v (fp64 partial sums in a fixed order, rounded to float once), for every vector of the list in turn.  The
// scratch -- 256 partial sums and the float on the device -- is this call's own, one for all the vectors.
struct FloatVec { const float *v; int64_t n; float *sum; };
static int sum_floats(hipStream_t st, std::initializer_list<FloatVec> vecs, const char *who) {
  DevBufs bufs;
  double *part = bufs.get<double>(256); float *sum_dev = bufs.get<float>(1);
  if (bufs.failed()) return no_memory(who);
  for (const FloatVec &f : vecs) {
    hipLaunchKernelGGL(k_sum_stage1, dim3(256), dim3(256), 0, st, f.v, f.n, part);
    hipLaunchKernelGGL(k_sum_stage2, dim3(1), dim3(256), 0, st, part, 256, sum_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, f.sum, sum_dev, sizeof(float)));
  }
  return BWGR_OK;
}

// the refusal of every entry point that sweeps the columns as stored
static int refuse_centred(const char *who) {
  return fail(BWGR_EINVAL, "%s: this panel sweeps implicitly centred columns (bwgr_panel_set_centred), which only the fused chains do; call bwgr_panel_set_centred(P, 0) first", who);
}

static int require_device(int device) {
  int c = 0; bwgr_device_count(&c);
  if (c <= 0) return fail(BWGR_ENODEV, "no HIP device visible: libbwgr_hip has no CPU fallback");
  if (device < 0 || device >= c) return fail(BWGR_EINVAL, "device %d out of range (%d visible)", device, c);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(BWGR_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device, prop.gcnArchName);
  HIPCHK(hipSetDevice(device));
  return BWGR_OK;
}

// the words the workgroups poll (flags, delta granules, q words and the feeders' sums) live in one allocation
static int alloc_exchange(bwgr_panel *P) {
  const size_t K = (size_t)P->data->plan.K;
  const size_t fb = (sizeof(uint32_t) * (K + 1) * SW_FLAG_STRIDE + 255) & ~(size_t)255;
  const size_t gb = (sizeof(unsigned long long) * S2_NSLOT * SW_MAXM + 255) & ~(size_t)255;
  const size_t qb = sizeof(double) * S2_NSLOT * (K + 1) * SW_MAXM;
  P->xchg_bytes = fb + gb + qb;
  CHK(own_array(P->own, P->xchg, P->xchg_bytes, "panel scratch"));
  P->xflags = reinterpret_cast<uint32_t *>(P->xchg);
  P->dgran = reinterpret_cast<unsigned long long *>(P->xchg + fb);
  P->qpart = reinterpret_cast<double *>(P->xchg + fb + gb);
  return BWGR_OK;
}
// polled words are zeroed before every launch (epochs count within a launch)
// ---- the sweep plan -----------------------------------------------------------------------------------------------------------
// Which engine a sweep runs, how deep, and in what launch shape is one decision, made by plan_sweep (below) from the panel -- its geometry,
// its Gram range, its clones and pairs, its switches -- and the sweep's flags.  The launch code executes a plan and decides nothing of its own;
// the occupancy guard prices the plan's spin launches.
// resident: the workgroups of the grid that stay for the sweep (L2 prefetch workgroups beyond the first few leave at once)
struct SpinLaunch { const void *fn; int grid, resident, threads; size_t lds; };
struct SweepPlan {
  int engine = 1;          // bwgr_panel_pipeline's generation: 1 k_sweep, 2 k_sweep2, 3 k_sweep3 (k_sweep2 beside it while the gate is finite), 4 k_sweep2w
  float gate3 = 0.0f;      // k_sweep3 takes the sweeps of chains below this inclusion rate (decided on the device); 0: never, INFINITY: every one
  int lag = 2, nfeed = 0;  // pipeline depth; q feeder workgroups of k_sweep2
  bool g16 = false;        // k_sweep2 on the 16-bit Gram copies
  int R3 = 0, K3 = 0, sub = 0, pf = -1, pf2 = -1, dbg3 = 0, qsplit = 0, skip_vb = 0;   // k_sweep3 (dbg3: the DMA streamer bits, and BWGR_DBG3)
  bool fixed3 = false;     // ... as k_sweep3f, the fixed-shape instantiation
  int fx = 0, nd = 0, npf = 0, ahead = 0, nq = 0, wsub = 0, wK3 = 0;                  // k_sweep2w
  bool guarded = false;    // the range snapshot in front, the fp64 redo (plan_sweep(P, a, true)) behind
  bool draws = false;      // the next iteration's variates drawn beside the sweep (draws_ahead)
  int nspins = 0; SpinLaunch spins[3];   // the launches whose workgroups wait for one another: the primary's, then the redo's
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
// after the real launches: this handle holds `need` units until the event behind them completes
static void guard_mark(bwgr_panel *P, hipStream_t st, int need) {
  if (need <= 0) return;
  std::lock_guard<std::mutex> lk(g_guard_mu);
  if (!P->guard_ev) { if (hipEventCreateWithFlags(&P->guard_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); P->guard_ev = nullptr; return; } }
  if (!P->guard_listed) { g_guard_panels.push_back(P); P->guard_listed = true; }
  if (P->guard_cus > 0 && P->guard_stream == st && hipEventQuery(P->guard_ev) != hipSuccess) { (void)hipGetLastError(); need = std::max(need, P->guard_cus); }
  P->guard_cus = need; P->guard_stream = st;
  (void)hipEventRecord(P->guard_ev, st);
}
static void guard_forget(bwgr_panel *P) {
  std::lock_guard<std::mutex> lk(g_guard_mu);
  for (size_t i = 0; i < g_guard_panels.size(); ++i) if (g_guard_panels[i] == P) { g_guard_panels.erase(g_guard_panels.begin() + i); break; }
  if (P->guard_ev) { (void)hipEventDestroy(P->guard_ev); P->guard_ev = nullptr; }
  P->guard_listed = false; P->guard_cus = 0;
}

static int reset_exchange(bwgr_panel *P) {
  if (P->data->plan.pipelined) {
    HIPCHK(hipMemsetAsync(P->xchg, 0, P->xchg_bytes, P->stream));
  } else if (P->data->plan.K > 1) {
    HIPCHK(hipMemsetAsync(P->xflags, 0, sizeof(uint32_t) * ((size_t)P->data->plan.K + 1) * SW_FLAG_STRIDE, P->stream));
  }
  return BWGR_OK;
}

static void launch_gram(bwgr_panel *P, void *g, int dist);   // (with the panel's other Gram launches, below)
// ---- k_sweep3 (sweep3.hip.h): what it needs beside the panel ----
// plan3, then the cross Gram arrays of distance 1 .. D-1 in the element type of the 16-bit (or, failing that, 32-bit) staging
static int sweep3_build(bwgr_panel *P) {
  PanelData *D = P->data; const PanelPlan &pl = D->plan;
  D->e3_ready = false;
  D->plan3 = plan_panel3(pl, D->sw, D->gram16);
  if (!D->plan3.fits) return BWGR_OK;
  const int m = pl.m; const bool g16 = D->gram16;
  const size_t blk_elems = (size_t)pl.nblocks * m * m;
  int bad = 0;
  std::vector<void *> far;   // the arrays made here
  {   // the far blocks; tmp, a whole Gram array, goes once they are built and before the 16-bit verdict is acted on
    DevBufs bufs;
    int32_t *tmp = nullptr;
    for (int d = 1; d < D->plan3.D && d < pl.nblocks; ++d) {
      void *have32 = d <= pl.xdist ? D->gx[d] : nullptr, *have = g16 ? (d == 1 ? (void *)D->gramx16 : nullptr) : have32;
      if (have) { D->g3x[d - 1] = have; continue; }
      void *arr = nullptr;
      CHK(own_array(D->own, arr, blk_elems * (g16 ? 2 : 4), "panel_create"));
      D->g3x[d - 1] = arr; far.push_back(arr);
      if (g16) {
        if (!have32) {
          if (!tmp && !(tmp = bufs.get<int32_t>(blk_elems))) return fail(BWGR_ENOMEM, "panel_create: device allocation failed");
          launch_gram(P, tmp, d);
          have32 = tmp;
        }
        hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)have32 + (size_t)d * m * m, (uint16_t *)arr + (size_t)d * m * m, (int64_t)(pl.nblocks - d) * m * m, D->gram16_bad);
      } else launch_gram(P, arr, d);
      HIPCHK(hipGetLastError());
    }
    if (g16) HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  if (bad) {   // an entry of a far block left the 16-bit range although the near blocks fit: rare; leave the panel to k_sweep2
    for (void *q : far) D->own.drop(q);
    for (void *&g : D->g3x) g = nullptr;
    return BWGR_OK;
  }
  if (g16) {   // 16-bit panels: an included marker's distance-1 / 2 rows in one piece
    CHK(own_array(D->own, D->gx12, (size_t)pl.nblocks * m * 2 * m * 2, "panel_create"));
    hipLaunchKernelGGL(k_near_rows, dim3(4096), dim3(256), 0, P->stream, (const uint16_t *)D->g3x[0], (const uint16_t *)(D->plan3.D >= 3 ? D->g3x[1] : nullptr), (uint16_t *)D->gx12, m, (int64_t)pl.nblocks);
    HIPCHK(hipGetLastError());
  }
  for (const void *f : {reinterpret_cast<const void *>(k_sweep3<uint16_t, false>), reinterpret_cast<const void *>(k_sweep3<int32_t, false>), reinterpret_cast<const void *>(k_sweep3<uint16_t, true>),
                        reinterpret_cast<const void *>(k_sweep3<int32_t, true>), reinterpret_cast<const void *>(k_sweep3p<uint16_t>), reinterpret_cast<const void *>(k_sweep3p<int32_t>),
                        reinterpret_cast<const void *>(k_sweep3f)})
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  D->e3_ready = true;
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

static void launch_prestage(bwgr_panel *P, const SweepArgs &a_in, const SweepPlan &pl) {
  SweepArgs a = a_in;
  a.gate3 = pl.gate3;
  const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
  const int64_t tasks = 4ll * (j1 - j0);
  const bool s3 = a.gate3 > 0.0f;
  const bool fxa = pl.engine == 4 && pl.fx;   // an affine sweep on the fixed-point streamers
  const int sh_add = P->data->sw.sh_add;   // test hook: less headroom, to leave the range on purpose
  int xbits = 0; while ((1 << xbits) < std::max(1, P->data->xmax)) ++xbits;   // (the fixed-point scales: the residual, and what k_prestage knows of the steps times the largest |x|)
  if (s3 || fxa) hipLaunchKernelGGL(k_escale_reset, dim3(1), dim3(1), 0, P->stream, a.sc);
  // the variates drawn ahead (draws_ahead, below) when they are this very iteration's: same streams, same counters, same flags, this range inside theirs
  const int dflags = a.flags & (SWF_SELECT | SWF_VB_VEC);
  const bool have_draws = P->draws_valid && P->draws_iter == a.iter && P->draws_marker0 == a.marker0 && P->draws_flags == dflags &&
                          P->draws_sc == (const void *)a.sc && P->draws_j0 <= j0 && P->draws_j1 >= j1 && memcmp(&P->draws_rng, &a.rng, sizeof(Rng)) == 0 &&
                          !(a.flags & (SWF_MH | SWF_EM_ANY));
  a.draws = nullptr;
  if (have_draws) { const hipError_t he = hipStreamWaitEvent(P->stream, P->draws_ready, 0); if (he == hipSuccess) a.draws = P->draws; else { fprintf(stderr, "bwgr: draws wait failed: %s\n", hipGetErrorString(he)); (void)hipGetLastError(); } }
  if (a.draws) {
    hipLaunchKernelGGL(k_prestage_fin, dim3((unsigned)std::min<int64_t>(2048, (j1 - j0 + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
    { const hipError_t he = hipEventRecord(P->draws_free, P->stream); if (he != hipSuccess) { fprintf(stderr, "bwgr: draws_free record failed: %s\n", hipGetErrorString(he)); (void)hipGetLastError(); } }
    P->draws_valid = false;   // (consumed: the buffer is the next iteration's from here)
  } else hipLaunchKernelGGL(k_prestage, dim3((unsigned)std::min<int64_t>(4096, (tasks + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
  if (s3) {   // the sweep's fixed-point scale, then the in-block speculative terms on that grid
    hipLaunchKernelGGL(k_escale, dim3(1), dim3(1024), 0, P->stream, a.e, P->data->plan.ld, a.sc, xbits, a.gate3, sh_add);
    if (a.flags & SWF_CENTRE) {   // the rejected steps' share of sum(e_stored), block by block (the whole panel: launch_prestage is called with every block)
      hipLaunchKernelGGL(k_cen_tot, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, 0);
      hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, a, (int)P->data->plan.nblocks, 0);
    }
    hipLaunchKernelGGL(k_spec3, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, P->data->gram16 ? (const uint16_t *)P->data->gramp16 : (const uint16_t *)nullptr);
    if (std::isinf(a.gate3)) return;
  }
  if (pl.engine == 4) {
    if (pl.fx) hipLaunchKernelGGL(k_escale, dim3(1), dim3(1024), 0, P->stream, a.e, P->data->plan.ld, a.sc, xbits, INFINITY, sh_add);   // (|b0|, the noise terms)
    hipLaunchKernelGGL(k_affine_inv, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(512), S2W_INV_LDS, P->stream, a, P->winv, (a.flags & SWF_DELTA2) ? 2.0 : 1.0);
    return;
  }
  if (P->data->plan.pipelined) {
    const int sel = (a.flags & SWF_SELECT) ? 1 : 0;
    const unsigned nb = (unsigned)(a.blk_end - a.blk_begin);
    if ((a.flags & SWF_CENTRE) && sel) {   // the fp64 engine's share of an implicitly centred iteration (the float steps themselves; runs on k_sweep2's side of the gate)
      hipLaunchKernelGGL(k_cen_tot, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, 1);
      hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, a, (int)P->data->plan.nblocks, 1);
    }
    if (P->data->is_f32) hipLaunchKernelGGL(k_spec<double>, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, sel);
    else hipLaunchKernelGGL(k_spec<int32_t>, dim3(nb), dim3(128), 0, P->stream, a, a.blk_begin, sel);
  }
}

// The next iteration's variates, enqueued beside this iteration's sweep (see k_draws) where the plan says so.  `a` = this iteration's arguments
// over the whole panel.  Failing to set it up is not an error: k_prestage draws for itself whenever the buffer is not this iteration's.
static void draws_ahead(bwgr_panel *P, const SweepArgs &a, const SweepPlan &pl, hipEvent_t before_sweep) {
  if (!pl.draws) return;
  if (!P->draws) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);   // (lo: the numerically largest = the lowest priority)
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(k_draws), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess) { (void)hipGetLastError(); return; }
    if (!P->own.take({{&P->draws, sizeof(double) * 5 * (size_t)P->data->p}, DevBufs::want_stream(&P->draws_stream, hipStreamNonBlocking, lo),
                      DevBufs::want_event(&P->draws_ready, hipEventDisableTiming), DevBufs::want_event(&P->draws_free, hipEventDisableTiming)})) return;
    (void)hipEventRecord(P->draws_free, P->stream);
  }
  const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
  // after this iteration's k_prestage has read the buffer (draws_free) -- or, the first time, after what is enqueued so far; 160 workgroups with 96 KB of
  // LDS each: at most 160 compute units, none of them one that runs a workgroup of the sweep
  // (... and after the iteration's speculative terms, which are bandwidth-bound and would share the chip with it: the event in front of the sweep)
  { const hipError_t h1 = hipStreamWaitEvent(P->draws_stream, P->draws_free, 0), h2 = hipStreamWaitEvent(P->draws_stream, before_sweep, 0);
    if (h1 != hipSuccess || h2 != hipSuccess) { fprintf(stderr, "bwgr: draws_ahead waits failed: %s / %s\n", hipGetErrorString(h1), hipGetErrorString(h2)); (void)hipGetLastError(); return; } }
  hipLaunchKernelGGL(k_draws, dim3(160), dim3(1024), 96 * 1024, P->draws_stream, a.rng, a.marker0, a.iter + 1u, a.flags, (const ChainScalars *)a.sc, (int64_t)P->data->p, j0, j1, P->draws);
  { const hipError_t h1 = hipGetLastError(); const hipError_t h2 = (h1 == hipSuccess) ? hipEventRecord(P->draws_ready, P->draws_stream) : hipSuccess;
    if (h1 != hipSuccess || h2 != hipSuccess) { fprintf(stderr, "bwgr: k_draws launch / record failed: %s / %s\n", hipGetErrorString(h1), hipGetErrorString(h2)); (void)hipGetLastError(); P->draws_valid = false; return; } }
  P->draws_valid = true; P->draws_rng = a.rng; P->draws_iter = a.iter + 1u; P->draws_marker0 = a.marker0; P->draws_flags = a.flags & (SWF_SELECT | SWF_VB_VEC);
  P->draws_j0 = j0; P->draws_j1 = j1; P->draws_sc = (const void *)a.sc;
}

// The plan of one sweep of blocks [a.blk_begin, a.blk_end) with a.flags over P (redo: the fp64 launch that redoes a fixed-point sweep
// which left its range).  Reads the panel only: nothing is enqueued or allocated.
static SweepPlan plan_sweep(const bwgr_panel *P, const SweepArgs &a, bool redo) {
  SweepPlan pl;
  const Switches &sw = P->data->sw;
  const bool sel = (a.flags & SWF_SELECT) != 0, cen = (a.flags & SWF_CENTRE) != 0;
  const auto spin = [&](const void *fn, int grid, int resident, int threads, size_t lds) { pl.spins[pl.nspins++] = SpinLaunch{fn, grid, resident, threads, lds}; };
  // The selection models' sweeps on a panel that has k_sweep3: the device picks the engine from the chain's current inclusion rate
  // (ChainScalars::inc_rate against the panel's threshold), so both engines' kernels are enqueued and one side leaves at once (a few
  // microseconds per iteration); a threshold >= 1, or a pair run, means k_sweep3 always and the other side is not enqueued at all.
  if (P->data->e3_ready && sel && !(a.flags & SWF_EM_ANY) && !redo) pl.gate3 = (sw.eng3_thr >= 1.0f || P->force3) ? INFINITY : sw.eng3_thr;
  // The affine sweeps of an int8 panel with 16-bit Gram staging: k_sweep2w, with its own streamers (s2w_streamer_fx: 128 rows each,
  // fixed-point residual) where the slab count allows
  const bool winv = sw.winv && P->data->plan.pipelined && !P->data->is_f32 && P->data->winv_nd >= 1 && P->data->plan.K <= 2 * (S2W_QW + S2W_QX) &&
                    !(a.flags & (SWF_SELECT | SWF_EM_ANY | SWF_SERIAL)) && P->data->plan.ldsw > 0 && P->data->plan.ldsw <= (size_t)160 * 1024;
  const bool wfx = sw.wfx && (P->data->plan.R % S2W_FXR) == 0 && P->data->plan.K * (P->data->plan.R / S2W_FXR) <= 255;
  pl.engine = pl.gate3 > 0.0f ? 3 : winv ? 4 : P->data->plan.pipelined ? 2 : 1;
  // Selection sweeps of k_sweep2: three blocks deep.  (The single-barrier sequencer also knows a fourth level, BWGR_LAG=4: it was
  // the default while k_sweep2 also ran the sparse chains; those are k_sweep3's now, and from 5 % of the markers in the model upwards
  // the third cross term's row fetches cost more than the depth gives -- C4-size BayesC at 5 / 19 / 36 % inclusion: 31.4 / 21.3 /
  // 14.5 iter/s at depth 3 against 30.9 / 19.4 / 9.4 at depth 4; BayesCpi at 51 %: 11.1 against 6.7.)  BWGR_LAG=2|3|4 sets it (A/B tests).
  int lag = 2;
  if (P->data->plan.pipelined && sel) {
    // the generic sequencer (32-bit Gram entries, fp32 panels) reads a distance-2 row per accepted marker straight from global memory on
    // one wave: two blocks deep unless asked (us per block at n = 10 000, depth 2 / 3: 1.4 % inclusion 4.53 / 4.67, 10.9 % 5.29 / 14.5,
    // BayesCpi at 52 % 12.7 / 58.0); the 16-bit / single-barrier sequencer stages those rows and knows a third cross term as well
    if (P->data->plan.xdist >= 2 && (sw.lag >= 0 || P->data->gram16)) lag = 3;
    if (P->data->plan.xdist >= 3 && P->data->gram16) lag = 4;   // (a panel with distance-3 blocks fits the lag-4 streamer: plan_panel)
  }
  pl.lag = std::min(lag, (sw.lag >= '2' && sw.lag <= '4') ? sw.lag - '0' : 3);
  if (winv) {   // the affine sweeps' product sequencer: as deep as the panel's cross Gram planes reach (BWGR_WLAG caps it)
    pl.lag = std::min(P->data->winv_nd + 1, sw.wlag_cap);
    if (!wfx) pl.lag = std::min(pl.lag, 4);   // (k_sweep2's streamers hold four tiles)
#ifdef BWGR_EXPERIMENTS
    if (sw.wlag_timing) pl.lag = sw.wlag_timing;   // TIMING ONLY: deeper than the cross terms reach (wrong chain)
#endif
  }
  // streamers, sequencer, and for the selection models the q feeders (the affine recurrence is compute-bound: its
  // sequencer gathers q itself under the recurrence, and a feeder hop in its lag-2 chain measured 15 % slower)
  pl.nfeed = (P->data->plan.pipelined && sel) ? P->data->plan.nfeed : 0;
  // selection models: 16-bit staging and the single-barrier sequencer (the affine recurrence is compute-bound and measured faster on
  // the 32-bit blocks: no conversion in its inner loop)
  pl.g16 = P->data->plan.pipelined && P->data->gram16 && sel;
  // A chain that has the GPU to itself (a root panel without clones) runs 128-row streamers, two to a slab: 80 compute units instead
  // of 41, 15.98-16.18 against 16.49 ms per sweep at C4 (the same chain bit for bit: the slab dots are integer sums).  With clones
  // alive -- chains side by side, pairs -- every chain keeps the 256-row streamers the concurrency counts assume.  BWGR_SOLO3=0: never.
  const bool alone = P->data->plan3.solo3 && !P->data->crowded && P->is_root && P->data->nclones == 0;
  // The next iteration's variates beside the sweep (draws_ahead): selection models with the logistic step, only for a chain alone (beside
  // other chains or shards the idle compute units it would run on are theirs: five chains side by side 255 -> 226 chain-iter/s, three
  // shards 163 -> 119 iter/s with it); BWGR_DRAWS=0 switches it off
  pl.draws = sel && !(a.flags & (SWF_MH | SWF_EM_ANY)) && alone && sw.draws;
  if (pl.gate3 > 0.0f) {
    pl.R3 = P->data->plan3.R3; pl.sub = P->data->plan3.sub3; pl.K3 = P->data->plan3.K3;
#ifdef BWGR_EXPERIMENTS
    pl.dbg3 = sw.dbg3;   // (timing switches, some of which break the chain: the experiment build only)
#endif
    {   // 128-row streamers land their tiles by LDS-DMA (s3_streamer_dma; C4 15.0 -> 13.65 ms per sweep); BWGR_STREAM3=reg: through registers, as the 256-row ones do
      // The DMA streamer forms a tile piece's source as a 32-bit lane offset from the launch's first column (no 64-bit vector arithmetic): only
      // launches whose column range spans less than 4 GiB of one slab take it (p * R < 2^32: 16.7 M markers at R = 256); wider ones keep the
      // register path, whose offsets are size_t.  bwgr_debug_stream3_dma() exposes the rule to the CPU tests.
      const int64_t j_lo = (int64_t)a.blk_begin * a.m, j_hi = std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
      const bool fits32 = stream3_dma_fits(j_hi - j_lo, P->data->plan.R);
      if (sw.stream3 != 'r' && fits32) pl.dbg3 |= (1 << 22);
      if (sw.stream3 == 'd' && fits32) pl.dbg3 |= (1 << 23);   // (EXPERIMENT: the 256-row streamers too, three tile buffers)
    }
    if (P->force3) {   // a pair run (bwgr_chain_run_pair): one k_sweep3p launch, K3 streamers and two sequencers, serves both chains; no redo
      const size_t lds = std::max(s3p_streamer_lds(pl.R3), s3_seq_lds(P->data->plan3.D, P->data->gram16));
      spin(P->data->gram16 ? reinterpret_cast<const void *>(k_sweep3p<uint16_t>) : reinterpret_cast<const void *>(k_sweep3p<int32_t>), pl.K3 + 2, pl.K3 + 2, SW_THREADS, lds);
      return pl;
    }
    if (alone && pl.R3 == 256 && 2 * pl.K3 + 1 <= 256) { pl.R3 = 128; pl.sub = P->data->plan.R / 128; pl.K3 = P->data->plan.K * pl.sub; }
    // one more workgroup, on the sequencer's XCD (workgroups with equal index mod 8 share an XCD), warms that XCD's L2 with what the
    // staging waves load (on for a chain alone on the GPU: 15.61 -> 15.37 ms per sweep at C4 on the steadied kernel; beside other chains
    // the workgroup is not counted by bwgr_panel_max_concurrent, so it stays off there; BWGR_PF3=0|1 decides otherwise)
    const bool pf_on = (sw.pf3 >= 0 ? sw.pf3 == '1' : alone) && pl.K3 + 2 <= 256;
    pl.pf = pf_on ? ((pl.K3 + 2 > 8) ? 8 : pl.K3 + 1) : -1;
    const bool pf2_on = pf_on && pl.pf == 8 && P->data->gram16 && P->data->gx12 && pl.K3 + 3 > 16 && pl.K3 + 3 <= 256 && sw.pf3b;
    pl.pf2 = pf2_on ? 16 : -1; pl.qsplit = 1; pl.skip_vb = (a.flags & SWF_VB_VEC) ? 1 : 0;
    const int grid = pl.K3 + 1 + (pf_on ? 1 : 0) + (pf2_on ? 1 : 0);
    const void *fn = P->data->gram16 ? (cen ? reinterpret_cast<const void *>(k_sweep3<uint16_t, true>) : reinterpret_cast<const void *>(k_sweep3<uint16_t, false>))
                                  : (cen ? reinterpret_cast<const void *>(k_sweep3<int32_t, true>) : reinterpret_cast<const void *>(k_sweep3<int32_t, false>));
    // k_sweep3f (sweep3.hip.h, S3Shape128) is this launch with its geometry as constants and no other role compiled in: taken where the launch is exactly
    // that -- 128 markers a block and their packed stride, 16-bit Gram entries with the distance-1 / 2 records, columns as stored, 128-row DMA streamers
    // with four tile buffers and nothing else asked of dbg3 (the experiment build keeps BWGR_DBG3: the same switches in both kernels), the 4 + 3 digit
    // split; not under the abort hook, whose absent streamer is k_sweep3's.  The same chain bit for bit; bwgr_debug_sweep3_kernel() tells which one runs.
    pl.fixed3 = sw.fixed3 && P->data->gram16 && !cen && P->data->gx12 && P->data->plan.m == S3Shape128::m && P->data->plan.pstride == S3Shape128::pstride &&
                pl.R3 == 128 && (pl.dbg3 & (3 << 22)) == (1 << 22) && pl.qsplit == 1 && !P->debug_withhold;
    spin(pl.fixed3 ? reinterpret_cast<const void *>(k_sweep3f) : fn, grid, grid, SW_THREADS, P->data->plan3.lds3);
  }
  if (!std::isinf(pl.gate3)) {
    if (winv) {
      pl.fx = (wfx && !redo) ? 1 : 0;
      if (!pl.fx) pl.lag = std::min(pl.lag, 4);   // (k_sweep2's streamers -- the range-recovery launch, BWGR_WFX=0 -- hold four tiles)
      pl.nd = std::min(pl.lag - 1, (int)S2W_MAXDIST);
      pl.npf = sw.wpf; pl.ahead = sw.wahead;   // (npf measured at C2: 0 -> 540, 2 -> 636, 4 -> 685 iter/s; 6 and 8 no better)
      pl.wsub = P->data->plan.R / S2W_FXR; pl.wK3 = P->data->plan.K * pl.wsub;
      pl.nq = sw.wnq ? sw.wnq : (pl.wK3 > 48 ? 2 : 1);   // (C2, 40 streamers: one copy 1.10 ms, two 1.21; C4 shape, 80 streamers: 27.8 / 25.6 / 27.6 ms with 1 / 2 / 4)
      // (of the 8 npf workgroups past the sequencer, the npf on its XCD prefetch; the others leave at once)
      const int wgs = pl.fx ? pl.wK3 : P->data->plan.K;
      spin(pl.fx ? reinterpret_cast<const void *>(k_sweep2w<true>) : reinterpret_cast<const void *>(k_sweep2w<false>), wgs + 1 + 8 * pl.npf, wgs + 1 + pl.npf, S2W_THREADS, P->data->plan.ldsw);
    } else if (P->data->plan.pipelined) {
      const void *fn = P->data->is_f32 ? (sel ? reinterpret_cast<const void *>(k_sweep2<float, true>) : reinterpret_cast<const void *>(k_sweep2<float, false>))
                       : pl.g16  ? reinterpret_cast<const void *>(k_sweep2<int8_t, true, uint16_t>)
                       : sel     ? reinterpret_cast<const void *>(k_sweep2<int8_t, true>) : reinterpret_cast<const void *>(k_sweep2<int8_t, false>);
      spin(fn, P->data->plan.K + 1 + pl.nfeed, P->data->plan.K + 1 + pl.nfeed, SW_THREADS, P->data->plan.lds2);
    } else {
      const void *fn = P->data->is_f32 ? (sel ? reinterpret_cast<const void *>(k_sweep<float, true>) : reinterpret_cast<const void *>(k_sweep<float, false>))
                                 : (sel ? reinterpret_cast<const void *>(k_sweep<int8_t, true>) : reinterpret_cast<const void *>(k_sweep<int8_t, false>));
      spin(fn, P->data->plan.K, P->data->plan.K, SW_THREADS, P->data->plan.lds);
    }
  }
  // The fixed-point engines between a snapshot of the state they start from and the fp64 engine that redoes the sweep if they left
  // their range (the reference's update cannot fail, src/Rcpp20260726ai.cpp:681).  Off for the debug abort hook (its launches must time out).
#ifdef BWGR_EXPERIMENTS
  const bool no_recover = sw.no_recover;   // (timing experiments that break the chain on purpose: the experiment build only)
#else
  constexpr bool no_recover = false;
#endif
  if (!redo && (pl.gate3 > 0.0f || (winv && wfx)) && !P->debug_withhold && !no_recover) {
    const SweepPlan r = plan_sweep(P, a, true);
    for (int i = 0; i < r.nspins; ++i) pl.spins[pl.nspins++] = r.spins[i];
    pl.guarded = true;
  }
  return pl;
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
// one engine's launch of the plan (redo: the fp64 launch behind a fixed-point one that left its range)
static void launch_sweep_engine(bwgr_panel *P, const SweepArgs &a_in, const SweepPlan &pl, bool redo) {
  SweepArgs a = a_in;
  if (P->debug_withhold) a.flags |= SWF_DEBUG_WITHHOLD;
  a.gate3 = pl.gate3; a.redo_only = redo ? 1 : 0;
  const bool sel = (a.flags & SWF_SELECT) != 0;
  if (redo && pl.engine == 2) {   // the fp64 engine's speculative terms (k_spec) of the state just restored
    if ((a.flags & SWF_CENTRE) && sel) {   // the running block sums on the float steps (the fixed-point launch left them on its grid): every block, then the scan
      SweepArgs all = a; all.blk_begin = 0; all.blk_end = (int)P->data->plan.nblocks;
      hipLaunchKernelGGL(k_cen_tot, dim3((unsigned)P->data->plan.nblocks), dim3(128), 0, P->stream, all, 0, 2);
      hipLaunchKernelGGL(k_cen_scan, dim3(1), dim3(1024), 0, P->stream, all, (int)P->data->plan.nblocks, 2);
    }
    hipLaunchKernelGGL(k_spec<int32_t>, dim3((unsigned)(a.blk_end - a.blk_begin)), dim3(128), 0, P->stream, a, a.blk_begin, sel ? 1 : 0);
  }
  if (a.gate3 > 0.0f) {   // k_sweep3 (for the implicitly centred columns between its scalar terms' kernels), then the per-marker variances
    Sweep3Args A3;
    sweep3_args(P, a, pl, A3);
    const bool cen = (a.flags & SWF_CENTRE) != 0;
    if (cen) hipLaunchKernelGGL(k_cen_begin, dim3(1), dim3(1024), 0, P->stream, a, 0);
    void *args[] = {&A3};
    spin_launch(pl.spins[0], P->stream, args);
    if (cen) hipLaunchKernelGGL(k_cen_end, dim3(64), dim3(256), 0, P->stream, a, 0);
    if (pl.skip_vb) {   // (every launch: idempotent -- after a range redo the fp64 engine has written the same values from the same expression)
      const int j0 = a.blk_begin * a.m, j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m);
      hipLaunchKernelGGL(k_vb_fill, dim3((unsigned)std::min<int64_t>(1024, (j1 - j0 + 255) / 256)), dim3(256), 0, P->stream, a, j0, j1);
    }
    if (std::isinf(a.gate3)) return;
  }
  const SpinLaunch &L = pl.spins[a.gate3 > 0.0f ? 1 : 0];
  a.nfeed = pl.nfeed; a.lag = pl.lag;
  if (pl.engine == 4) {
    S2WArgs A; memset(&A, 0, sizeof(A));
    A.winv = P->winv; A.qsum = P->qsumw; A.fx = pl.fx; A.nd = pl.nd; A.npf = pl.npf; A.ahead = pl.ahead; A.sub = pl.wsub; A.K3 = pl.wK3; A.nq = pl.nq;
#ifdef BWGR_EXPERIMENTS
    A.dbg = P->data->sw.dbgw;
#endif
    for (int d = 0; d < S2W_MAXDIST; ++d) A.gxt[d] = P->data->gxt[d < P->data->winv_nd ? d : 0];
    if (A.fx) (void)hipMemsetAsync(P->qsumw + (size_t)a.blk_begin * A.nq * 2 * SW_MAXM, 0, sizeof(unsigned long long) * A.nq * 2 * SW_MAXM * (size_t)(a.blk_end - a.blk_begin), P->stream);
    void *args[] = {&a, &A}; spin_launch(L, P->stream, args);
    return;
  }
  const bool cen2 = P->data->plan.pipelined && (a.flags & SWF_CENTRE) && sel && !P->data->is_f32;
  if (cen2) hipLaunchKernelGGL(k_cen_begin, dim3(1), dim3(1024), 0, P->stream, a, redo ? 2 : 1);
  SweepArgs ak = a;
  if (pl.g16) { ak.gramp = P->data->gramp16; ak.gramx = P->data->gramx16; }
  void *args[] = {&ak}; spin_launch(L, P->stream, args);
  if (cen2) hipLaunchKernelGGL(k_cen_end, dim3(64), dim3(256), 0, P->stream, a, redo ? 2 : 1);
}
// the plan's sweep: the fixed-point engines between a snapshot of the state they start from and the fp64 redo (plan_sweep); no redo
// when the snapshot's scratch cannot be had
static void launch_sweep_kernel(bwgr_panel *P, const SweepArgs &a, const SweepPlan &pl) {
  const size_t p = (size_t)P->data->p;
  bool guarded = pl.guarded;
  if (guarded && !P->snap_e && !P->own.take({{&P->snap_e, sizeof(double) * (size_t)P->data->plan.ld}, {&P->snap_b, sizeof(float) * p}, {&P->snap_d, sizeof(float) * p}, {&P->snap_vb, sizeof(float) * p}})) guarded = false;
  SnapArgs sn;
  sn.e = a.e; sn.se = P->snap_e; sn.b = a.b; sn.d = a.d; sn.vb = (a.flags & SWF_VB_VEC) ? a.vb : nullptr; sn.sb = P->snap_b; sn.sd = P->snap_d; sn.svb = P->snap_vb;
  sn.ld = P->data->plan.ld; sn.j0 = a.blk_begin * a.m; sn.j1 = (int)std::min<int64_t>(P->data->p, (int64_t)a.blk_end * a.m); sn.sc = a.sc;
  if (guarded) hipLaunchKernelGGL(k_range_snapshot, dim3(256), dim3(256), 0, P->stream, sn);
  launch_sweep_engine(P, a, pl, false);
  if (guarded) {
    hipLaunchKernelGGL(k_range_recover, dim3(256), dim3(256), 0, P->stream, sn);
    hipLaunchKernelGGL(k_range_flag, dim3(1), dim3(1), 0, P->stream, a.sc);
    (void)reset_exchange(P);
    launch_sweep_engine(P, a, plan_sweep(P, a, true), true);
    hipLaunchKernelGGL(k_redo_clear, dim3(1), dim3(1), 0, P->stream, a.sc);
  }
}

// A handle that a pair run moved onto the pair's stream goes back to the stream it had (its own, or the caller's) when it next sweeps alone:
// one wait, on the handle's stream -- nothing is enqueued on the pair stream, which other pairs' hardware queue shares
static int leave_pair_stream(bwgr_panel *P) {
  if (!P->pre_pair_set) return BWGR_OK;
  hipEvent_t ev;
  HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t he = hipEventRecord(ev, P->stream);
  if (he == hipSuccess) he = hipStreamWaitEvent(P->pre_pair_stream, ev, 0);
  (void)hipEventDestroy(ev);
  if (he != hipSuccess) return fail(BWGR_EHIP, "leaving the pair stream: %s", hipGetErrorString(he));
  P->stream = P->pre_pair_stream; P->pre_pair_set = false;
  return BWGR_OK;
}
// What a sweep alone does before anything of it is enqueued (a refused sweep leaves the chain as it was): back from a pair's stream, the
// plan and its depth, the affine engine's scratch, the occupancy guard, then the zeroed exchange words
static int sweep_begin(bwgr_panel *P, SweepArgs &a, SweepPlan &pl, int *need) {
  CHK(leave_pair_stream(P));
  pl = plan_sweep(P, a, false); a.lag = pl.lag;
  if (pl.engine == 4) CHK(winv_alloc(P));
  CHK(sweep_guard(P, pl, P->stream, nullptr, need));
  return reset_exchange(P);
}
static int launch_sweep(bwgr_panel *P, SweepArgs &a) {
  SweepPlan pl; int need = 0;
  CHK(sweep_begin(P, a, pl, &need));
  P->ps_owner = nullptr;   // the scratch is about to hold this sweep's constants, nobody's iteration
  launch_prestage(P, a, pl);
  launch_sweep_kernel(P, a, pl);
  HIPCHK(hipGetLastError());
  guard_mark(P, P->stream, need);
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

// ------------------------------------------------------------------------------------------------
// panel
// ------------------------------------------------------------------------------------------------
template <typename ST, typename XT>
static int upload(bwgr_panel *P, const void *X, int memloc, int64_t ldx) {
  const int64_t n = P->data->n, p = P->data->p;
  XT *dst = reinterpret_cast<XT *>(P->data->X);
  if (memloc == BWGR_DEVICE) {
    hipLaunchKernelGGL((k_convert<ST, XT>), dim3(4096), dim3(256), 0, P->stream, reinterpret_cast<const ST *>(X), ldx, dst, P->data->plan.ld, (int)n, (int64_t)0, p, P->data->plan.R, p);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // host source: stage column chunks of <= 256 MiB
  const int64_t col_bytes = ldx * (int64_t)sizeof(ST);
  int64_t cols = std::max<int64_t>(1, ((int64_t)256 << 20) / std::max<int64_t>(1, col_bytes));
  cols = std::min(cols, p);
  DevBufs bufs;
  ST *stage = bufs.get<ST>((size_t)(cols * ldx));
  if (!stage) return fail(BWGR_ENOMEM, "panel_create: device allocation failed");
  for (int64_t j0 = 0; j0 < p; j0 += cols) {
    const int64_t nc = std::min(cols, p - j0);
    // the last column may be shorter than ldx in the caller's allocation: copy n rows of it separately
    const size_t bytes = (size_t)((nc - 1) * col_bytes + n * (int64_t)sizeof(ST));
    HIPCHK(hipMemcpyAsync(stage, reinterpret_cast<const ST *>(X) + j0 * ldx, bytes, hipMemcpyHostToDevice, P->stream));
    hipLaunchKernelGGL((k_convert<ST, XT>), dim3(2048), dim3(256), 0, P->stream, stage, ldx, dst, P->data->plan.ld, (int)n, j0, nc, P->data->plan.R, p);
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  return BWGR_OK;
}

// A handle's sweep scratch, made once its data is built (the root's by whoever makes the data, a clone's by bwgr_panel_clone): the
// speculative cross terms of the distances whose Gram blocks the data has, the pre-staged constants, the exchange words, and k_sweep3's
// sums and lists where the data has k_sweep3.  The rest of the scratch comes with the first sweep that needs it; the handle's holder owns all of it.
static int scratch_alloc(bwgr_panel *P) {
  const PanelData *D = P->data;
  const size_t nb = (size_t)D->plan.nblocks;
  const char *who = "panel scratch";
  if (D->plan.xdist >= 2) CHK(own_array(P->own, P->xspec2, nb * SW_MAXM, who));
  if (D->plan.xdist >= 3) CHK(own_array(P->own, P->xspec3, nb * SW_MAXM, who));
  if (D->plan.pipelined) CHK(own_array(P->own, P->ps.quick, nb, who));
  if (!P->own.take({{&P->ps.spec, sizeof(SpecBuf) * nb}, {&P->ps.blocks, sizeof(StageBuf) * nb}, {&P->xpart, sizeof(double) * 2 * (size_t)D->plan.K * SW_MAXM}})) return no_memory(who);
  CHK(alloc_exchange(P));
#if defined(BWGR_STAMPS) || defined(BWGR_EXPERIMENTS)
  CHK(own_array(P->own, P->stamps, 256, who));
  HIPCHK(hipMemset(P->stamps, 0, sizeof(unsigned long long) * 256));
#endif
  if (D->e3_ready) {
    if (!P->own.take({{&P->qsum3, sizeof(unsigned long long) * 2 * SW_MAXM * nb}, {&P->lists3, sizeof(unsigned long long) * S3_LSTRIDE * nb}})) return no_memory(who);
    HIPCHK(hipMemsetAsync(P->lists3, 0, sizeof(unsigned long long) * S3_LSTRIDE * nb, P->stream));
  }
  return BWGR_OK;
}

extern "C" int bwgr_panel_destroy(bwgr_panel *P) {
  if (!P) return BWGR_OK;
  PanelData *D = P->data;
  if (P->is_root && D->nclones > 0) return fail(BWGR_EINVAL, "panel_destroy: %d clone(s) of this panel are still alive", D->nclones);
  if (P->nchains > 0) return fail(BWGR_EINVAL, "panel_destroy: %d chain(s) on this panel are still alive (destroy them first)", P->nchains);
  (void)hipSetDevice(D->device);
  guard_forget(P);
  const bool root = P->is_root;
  delete P;   // the handle's scratch and streams, then the data's arrays and the pair streams
  if (root) delete D;
  else D->nclones--;
  return BWGR_OK;
}

// a10's xx, vx and MSx, and an int8 panel's largest |x|
static int panel_measure(bwgr_panel *P) {
  PanelData *D = P->data;
  const int p = (int)D->p, n = (int)D->n, wpb = 4;
  if (D->is_f32) hipLaunchKernelGGL(k_stats<float>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const float *)D->X, D->plan.R, n, p, D->xx, D->vx);
  else hipLaunchKernelGGL(k_stats<int8_t>, dim3((p + wpb - 1) / wpb), dim3(64 * wpb), 0, P->stream, (const int8_t *)D->X, D->plan.R, n, p, D->xx, D->vx);
  HIPCHK(hipGetLastError());
  CHK(sum_floats(P->stream, {{D->vx, (int64_t)p, &D->MSx}}, "panel_create"));
  if (!D->is_f32) {
    if (!D->xmax_dev) CHK(own_array(D->own, D->xmax_dev, 1, "panel_create"));
    HIPCHK(hipMemsetAsync(D->xmax_dev, 0, sizeof(int), P->stream));
    hipLaunchKernelGGL(k_absmax_i8, dim3(2048), dim3(256), 0, P->stream, (const int8_t *)D->X, D->plan.x_bytes, D->xmax_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&D->xmax, D->xmax_dev, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
  }
  return BWGR_OK;
}

// f(std::integral_constant<int, TJ>()) with TJ = tj, 1 <= tj <= MAXTJ (beyond: MAXTJ): the Gram kernels' block width in sixteens as a template parameter
template <int MAXTJ, typename F> static void with_tj(int tj, F f) {
  if constexpr (MAXTJ > 1) { if (tj < MAXTJ) return with_tj<MAXTJ - 1>(tj, f); }
  f(std::integral_constant<int, MAXTJ>());
}
// Gram blocks X_{b-dist}' X_b of the resident X, b = dist .. nblocks-1, into g[b][m][m]: int32, exact (fp64 for float panels); dist = 0: the diagonal blocks
static void launch_gram(bwgr_panel *P, void *g, int dist) {
  const PanelPlan &pl = P->data->plan;
  const int p = (int)P->data->p, m = pl.m, R = pl.R, tiles = dist ? 2 : 1;
  const dim3 grid((unsigned)(pl.nblocks - dist)), block(256);
  const int64_t ld = pl.ld; hipStream_t st = P->stream;
  const size_t ldsf = (size_t)tiles * m * 65 * sizeof(float), ldsi = (size_t)tiles * m * 33 * sizeof(int32_t);   // the kernels' LDS tiles
  const float *Xf = (const float *)P->data->X; double *gd = (double *)g;
  const int8_t *Xi = (const int8_t *)P->data->X; int32_t *gi = (int32_t *)g;
  const bool f32 = P->data->is_f32 != 0;
  if (!f32 && m == 128) hipLaunchKernelGGL(k_gram_mfma_i8, grid, block, 0, st, Xi, ld, R, p, gi, dist);
  else if (!f32 && dist) with_tj<8>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gramx_i8<decltype(tj)::value>, grid, block, ldsi, st, Xi, ld, R, p, m, gi, dist); });
  else if (f32 && !dist) with_tj<4>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gram_f32<decltype(tj)::value>, grid, block, ldsf, st, Xf, ld, R, p, m, gd); });
  else if (!dist) with_tj<8>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gram_i8<decltype(tj)::value>, grid, block, ldsi, st, Xi, ld, R, p, m, gi); });
  else with_tj<4>(m / 16, [&](auto tj) { hipLaunchKernelGGL(k_gramx_f32<decltype(tj)::value>, grid, block, ldsf, st, Xf, ld, R, p, m, gd, dist); });
}

// the Gram kernels sum a column pair of an int8 panel over every row in int32 (include/bwgr.h, at bwgr_panel_create)
static int gram_range(bool is_f32, int64_t rows, int xmax) {
  const int64_t xm = std::max(xmax, 1);
  if (!is_f32 && rows * xm * xm >= (1ll << 31)) return fail(BWGR_EINVAL, "panel: n * max|x|^2 = %lld does not fit the int32 Gram", (long long)(rows * xm * xm));
  return BWGR_OK;
}
// The Gram arrays the plan lists, from the resident X, and what they say: whether the 16-bit copies are exact (gram16) and how far the affine
// engine's byte planes reach (winv_nd).  Runs again wherever a scratch panel's rows or columns change.
static int panel_build_gram(bwgr_panel *P) {
  PanelData *D = P->data; const PanelPlan &pl = D->plan;
  const int m = pl.m;
  CHK(gram_range(D->is_f32 != 0, D->n, D->xmax));   // (a main panel's largest |x| is known only now; a scratch panel was checked before it was allocated)
  launch_gram(P, D->gram, 0);
  HIPCHK(hipGetLastError());
  for (int dist = 1; dist <= pl.xdist && dist < pl.nblocks; ++dist) {   // off-diagonal blocks (blk-dist, blk): the cross terms of the lag-2 / 3 / 4 pipelines
    launch_gram(P, D->gx[dist], dist);
    HIPCHK(hipGetLastError());
  }
  if (D->is_f32) hipLaunchKernelGGL(k_gram_pack<double>, dim3((unsigned)pl.nblocks), dim3(256), 0, P->stream, (const double *)D->gram, (double *)D->gramp, m, pl.pstride, pl.nblocks);
  else hipLaunchKernelGGL(k_gram_pack<int32_t>, dim3((unsigned)pl.nblocks), dim3(256), 0, P->stream, (const int32_t *)D->gram, (int32_t *)D->gramp, m, pl.pstride, pl.nblocks);
  HIPCHK(hipGetLastError());
  D->gram16 = false;
  if (pl.has16) {
    HIPCHK(hipMemsetAsync(D->gram16_bad, 0, sizeof(int), P->stream));
    hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)D->gramp, D->gramp16, (int64_t)pl.nblocks * pl.pstride, D->gram16_bad);
    if (pl.nblocks > 1)
      hipLaunchKernelGGL(k_gram_narrow, dim3(2048), dim3(256), 0, P->stream, (const int32_t *)D->gx[1] + (size_t)m * m, D->gramx16 + (size_t)m * m, (int64_t)(pl.nblocks - 1) * m * m, D->gram16_bad);
    HIPCHK(hipGetLastError());
    int bad = 1;
    HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
    D->gram16 = (bad == 0) && D->sw.gram16;   // BWGR_GRAM16=0 forces the 32-bit staging (A/B tests)
  }
  // the affine sweeps' sequencer (sweep2w.hip.h) takes the cross blocks as biased byte planes: built where every entry fits 16 bits
  D->winv_nd = 0;
  if (D->gram16 && pl.wdist > 0) {
    HIPCHK(hipMemsetAsync(D->gram16_bad, 0, sizeof(int), P->stream));
    int nd = 0;
    DevBufs bufs;
    int32_t *tmpx = nullptr;   // the distances beyond the panel's own arrays: built here, kept as planes only
    for (int dist = 1; dist <= pl.wdist; ++dist) {
      if (dist > S2W_NEARD) {
        if (!tmpx && !(tmpx = bufs.get<int32_t>((size_t)pl.nblocks * m * m))) { (void)hipGetLastError(); break; }
        launch_gram(P, tmpx, dist);
      }
      const int32_t *src = dist > S2W_NEARD ? tmpx : (const int32_t *)D->gx[dist];
      if (!D->gxt[dist - 1]) CHK(own_array(D->own, D->gxt[dist - 1], (size_t)pl.nblocks * S2W_PBYTES, "panel_create"));
      hipLaunchKernelGGL(k_gx_planes, dim3(4096), dim3(256), 0, P->stream, src, D->gxt[dist - 1], m, (int64_t)pl.nblocks, dist, D->gram16_bad);
      HIPCHK(hipGetLastError());
      nd = dist;
    }
    int bad = 1;
    HIPCHK(hipMemcpyAsync(&bad, D->gram16_bad, sizeof(int), hipMemcpyDeviceToHost, P->stream));
    HIPCHK(hipStreamSynchronize(P->stream));
    D->winv_nd = bad ? 0 : nd;
  }
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

// what only the data can say, each from the last: the columns' statistics, the Gram arrays and their verdicts, k_sweep3's share where the plan tries it
static int panel_setup(bwgr_panel *P) {
  CHK(panel_measure(P));
  CHK(panel_build_gram(P));
  return sweep3_build(P);
}

// The data of a panel of n rows x p markers -- its plan and every device array the plan lists, no values yet -- and its root handle, without
// the sweep scratch (scratch_alloc, once the data is built)
static int panel_alloc(bwgr_panel **out, int is_f32, int64_t n, int64_t p, int device, int block, int nwg, PanelKind kind, const Switches &sw) {
  *out = nullptr;
  CHK(panel_range(n, p));
  CHK(require_device(device));
  PanelPlan pl;
  CHK(plan_panel(pl, is_f32 != 0, n, p, block, nwg, kind, sw));
  bwgr_panel *P = new bwgr_panel();
  PanelData *D = P->data = new PanelData(); P->is_root = true;
  Guard drop([&] { bwgr_panel_destroy(P); });   // until the panel is handed over
  D->device = device; D->n = n; D->p = p; D->is_f32 = is_f32; D->sw = sw; D->plan = pl;
  const size_t packed = (size_t)pl.nblocks * std::max(pl.pstride, 8);
  if (!D->own.take({{&D->X, pl.x_bytes}, {&D->gram, pl.gram_bytes}, {&D->gramp, packed * (is_f32 ? 8 : 4)}, {&D->xx, sizeof(float) * p}, {&D->vx, sizeof(float) * p}}))
    return no_memory("panel_create");
  for (int d = 1; d <= pl.xdist; ++d) CHK(own_array(D->own, D->gx[d], pl.gram_bytes, "panel_create"));
  if (pl.has16 && !D->own.take({{&D->gramp16, packed * 2}, {&D->gramx16, (size_t)pl.nblocks * pl.m * pl.m * 2}, {&D->gram16_bad, sizeof(int)}})) return no_memory("panel_create");
  for (const void *f : {reinterpret_cast<const void *>(k_sweep<int8_t, true>), reinterpret_cast<const void *>(k_sweep<int8_t, false>), reinterpret_cast<const void *>(k_sweep<float, true>),
                        reinterpret_cast<const void *>(k_sweep<float, false>), reinterpret_cast<const void *>(k_sweep2<int8_t, true>), reinterpret_cast<const void *>(k_sweep2<int8_t, false>),
                        reinterpret_cast<const void *>(k_sweep2<int8_t, true, uint16_t>), reinterpret_cast<const void *>(k_sweep2<float, true>), reinterpret_cast<const void *>(k_sweep2<float, false>),
                        reinterpret_cast<const void *>(k_sweep2w<true>), reinterpret_cast<const void *>(k_sweep2w<false>), reinterpret_cast<const void *>(k_affine_inv)})
    HIPCHK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  drop.release();
  *out = P;
  return BWGR_OK;
}
// A scratch panel of P on P's stream: `rows` rows of P's markers (KMUP2, wgr's bagging) or P's columns in another order (bwgr_em).  Either's largest
// |x| is at most P's, so the scratch panel carries P's: panel_build_gram's int32 bound and the fixed-point scales of its sweeps (launch_prestage) are
// then those of the main panel, without a pass over the data.
static int scratch_panel_alloc(bwgr_panel **out, const bwgr_panel *P, int64_t rows, int nwg, PanelKind kind) {
  const PanelData *D = P->data;
  *out = nullptr;
  CHK(gram_range(D->is_f32 != 0, rows, D->xmax));   // refused before anything is allocated or enqueued
  CHK(panel_alloc(out, D->is_f32, rows, D->p, D->device, D->plan.m, nwg, kind, D->sw));
  (*out)->stream = P->stream;
  (*out)->data->xmax = D->xmax;
  return BWGR_OK;
}

extern "C" int bwgr_panel_create(bwgr_panel **out, const void *X, int xtype, int memloc, int64_t n, int64_t p,
                                 int64_t ldx, int device, int block, int nwg) {
  if (!out || !X) return fail(BWGR_EINVAL, "panel_create: null pointer");
  *out = nullptr;
  if (ldx < n) return fail(BWGR_EINVAL, "panel_create: need ldx >= n (n=%lld ldx=%lld)", (long long)n, (long long)ldx);
  if (xtype != BWGR_X_I8 && xtype != BWGR_X_F32 && xtype != BWGR_X_F64) return fail(BWGR_EINVAL, "panel_create: bad xtype %d", xtype);
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "panel_create: bad memloc %d", memloc);
  bwgr_panel *P = nullptr;
  CHK(panel_alloc(&P, xtype != BWGR_X_I8, n, p, device, block, nwg, PANEL_MAIN, read_switches()));
  Guard drop([&] { bwgr_panel_destroy(P); });
  if (xtype == BWGR_X_I8) CHK((upload<int8_t, int8_t>(P, X, memloc, ldx)));
  else if (xtype == BWGR_X_F32) CHK((upload<float, float>(P, X, memloc, ldx)));
  else CHK((upload<double, float>(P, X, memloc, ldx)));
  CHK(panel_setup(P));
  CHK(scratch_alloc(P));
  drop.release();
  *out = P;
  return BWGR_OK;
}

#if defined(BWGR_STAMPS) || defined(BWGR_EXPERIMENTS)
// diagnostic builds only: cumulative per-phase s_memtime ticks of workgroup 0, event counters (not part of include/bwgr.h)
extern "C" int bwgr_debug_stamps(bwgr_panel *P, unsigned long long out[256]) {
  HIPCHK(d2h(P->stream, out, P->stamps, sizeof(unsigned long long) * 256));
  HIPCHK(hipMemset(P->stamps, 0, sizeof(unsigned long long) * 256));
  return BWGR_OK;
}
#endif

// A clone: a second handle on the same data (the genotypes and Gram arrays are read-only during sweeps) with its own sweep scratch and its
// own stream, so that chains on the root panel and on its clones run concurrently on disjoint CUs.
extern "C" int bwgr_panel_clone(bwgr_panel **out, bwgr_panel *src) {
  if (!out || !src) return fail(BWGR_EINVAL, "panel_clone: null pointer");
  *out = nullptr;
  HIPCHK(hipSetDevice(src->data->device));
  HIPCHK(hipStreamSynchronize(src->stream));   // the shared arrays are complete
  bwgr_panel *P = new bwgr_panel();
  P->data = src->data; P->data->nclones++;
  Guard drop([&] { bwgr_panel_destroy(P); });
  if (!(P->stream = P->own.stream(hipStreamNonBlocking, 0))) return fail(BWGR_EHIP, "panel_clone: hipStreamCreate failed");
  CHK(scratch_alloc(P));
  HIPCHK(hipStreamSynchronize(P->stream));   // (k_sweep3's lists are zeroed on it)
  drop.release();
  *out = P;
  return BWGR_OK;
}

// chains (one per panel or clone) whose sweep kernels fit the chip side by side: each takes nwg + 1 (+ feeders) CUs
extern "C" int bwgr_panel_max_concurrent(const bwgr_panel *P, int selection, int *count) {
  if (!P || !count) return fail(BWGR_EINVAL, "null pointer");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, P->data->device));
  SweepArgs a{}; a.flags = selection ? SWF_SELECT : 0u;
  const SweepPlan pl = plan_sweep(P, a, false);
  // selection on a panel with k_sweep3: the device sends a chain above the engine threshold to k_sweep2 (K + 1 + feeders), and a sweep that
  // leaves the fixed-point range is redone there: the larger of the two (K3 + 1: the streamers of chains side by side, never the solo ones)
  int wgs = P->data->plan.K + 1 + pl.nfeed;
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

extern "C" int bwgr_panel_set_stream(bwgr_panel *P, void *hip_stream) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  P->stream = reinterpret_cast<hipStream_t>(hip_stream);
  P->pre_pair_set = false;   // (the caller's choice stands: no return to an earlier stream)
  return BWGR_OK;
}

extern "C" int bwgr_panel_info(const bwgr_panel *P, int64_t info[8]) {
  if (!P || !info) return fail(BWGR_EINVAL, "null pointer");
  info[0] = P->data->n; info[1] = P->data->p; info[2] = P->data->plan.ld; info[3] = P->data->plan.m; info[4] = P->data->plan.K; info[5] = P->data->plan.R;
  info[6] = (int64_t)P->data->plan.x_bytes; info[7] = (int64_t)(2 * P->data->plan.gram_bytes);
  return BWGR_OK;
}

// Which instantiation of the trajectory engine a selection sweep of the whole panel, as it stands now (clones alive, centred or not), is launched as:
// 0 none (the panel's selection sweeps are not k_sweep3's), 1 k_sweep3 / k_sweep3p, 2 k_sweep3f.  For the tests.
extern "C" int bwgr_debug_sweep3_kernel(const bwgr_panel *P, int *which) {
  if (!P || !which) return fail(BWGR_EINVAL, "null pointer");
  SweepArgs a{}; a.flags = SWF_SELECT | (P->data->cen ? SWF_CENTRE : 0u);
  a.m = P->data->plan.m; a.pstride = P->data->plan.pstride; a.blk_begin = 0; a.blk_end = (int)P->data->plan.nblocks;
  const SweepPlan pl = plan_sweep(P, a, false);
  *which = pl.engine != 3 ? 0 : (pl.fixed3 ? 2 : 1);
  return BWGR_OK;
}

extern "C" int bwgr_panel_pipeline(const bwgr_panel *P, int selection, int info[4]) {
  if (!P || !info) return fail(BWGR_EINVAL, "null pointer");
  SweepArgs a{}; a.flags = selection ? SWF_SELECT : 0u;
  const SweepPlan pl = plan_sweep(P, a, false);
  info[0] = pl.engine;
  info[1] = pl.engine == 3 ? P->data->plan3.D : pl.lag;
  info[2] = pl.engine == 3 ? 0 : pl.nfeed;
  info[3] = P->data->is_f32 ? 0 : (P->data->gram16 ? 16 : 32);
  return BWGR_OK;
}

extern "C" int bwgr_panel_stats(bwgr_panel *P, float *xx, float *vx, float *MSx) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  HIPCHK(hipSetDevice(P->data->device));
  if (xx) HIPCHK(d2h(P->stream, xx, P->data->cen ? P->data->xxc : P->data->xx, sizeof(float) * P->data->p));   // (centred panel: the centred columns' norms)
  if (vx) HIPCHK(d2h(P->stream, vx, P->data->vx, sizeof(float) * P->data->p));
  if (MSx) *MSx = P->data->MSx;
  return BWGR_OK;
}

// ------------------------------------------------------------------------------------------------
// what the families' entries share beside the sweep: the row gather, the redo count of the entries without a chain, X * coef, centring
// ------------------------------------------------------------------------------------------------
// The row gather's path, decided here and nowhere else (bwgr_debug_aux_plan exposes it to the CPU tests): 0 = element-wise (float panels, int8
// columns longer than 64 KB), else the columns an int8 workgroup stages in LDS -- ~30 KB of LDS per workgroup: five of them per CU
static int gather_mpw(bool is_f32, int64_t ld) {
  if (is_f32 || ld > 64 * 1024) return 0;
  return (int)std::max<int64_t>(1, std::min<int64_t>(8, (32 * 1024) / ld));
}
static size_t gather_lds(int mpw, int64_t ld) { return (size_t)mpw * (size_t)ld; }   // the staged columns
// row gather of the resident panel P into the subsample panel PB (rows use_d[0..nbag), device array); KMUP2's H = X(Use, j)
static void launch_gather_rows(bwgr_panel *P, bwgr_panel *PB, const int *use_d, int64_t nbag) {
  const int mpw = gather_mpw(P->data->is_f32, P->data->plan.ld);
  if (P->data->is_f32) hipLaunchKernelGGL(k_gather_rows<float>, dim3(4096), dim3(256), 0, P->stream, (const float *)P->data->X, P->data->plan.R, use_d, (int)nbag, (float *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p);
  else if (mpw > 0) {   // a column fits the LDS: stage, pick, write in 16-byte pieces
    hipLaunchKernelGGL(k_gather_rows_i8, dim3((unsigned)((P->data->p + mpw - 1) / mpw)), dim3(256), gather_lds(mpw, P->data->plan.ld), P->stream, (const int8_t *)P->data->X, P->data->plan.R, P->data->plan.ld,
                       use_d, (int)nbag, (int8_t *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p, mpw);
  } else hipLaunchKernelGGL(k_gather_rows<int8_t>, dim3(4096), dim3(256), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.R, use_d, (int)nbag, (int8_t *)PB->data->X, PB->data->plan.R, PB->data->plan.ld, P->data->p);
}

// Sweeps that the calling thread's last bwgr_kmup / bwgr_kmup2 / bwgr_wgr / bwgr_wgr_ex call redid on the fp64 residual after they left the
// fixed-point range (test hook: those entry points have no chain to ask, bwgr_chain_redo_count)
static thread_local int g_last_redo = 0;
extern "C" int bwgr_debug_last_redo(int *count) {
  if (!count) return fail(BWGR_EINVAL, "null pointer");
  *count = g_last_redo;
  return BWGR_OK;
}

// column chunks of the two-stage GEMV: enough workgroups to fill the chip at 16 rows per thread (int8) or 4 (float)
// (the rule, the columns of a chunk and the row workgroups live in the three functions below and nowhere else: bwgr_debug_aux_plan exposes them)
static int gemv_chunks_of(bool is_f32, int64_t p) { return (int)std::min<int64_t>(is_f32 ? 64 : 512, std::max<int64_t>(1, p / 512)); }
static int gemv_cpc_of(int64_t p, int nchunks) { return (int)((p + nchunks - 1) / nchunks); }
static unsigned gemv_row_wgs(bool is_f32, int64_t ld) { return (unsigned)((ld / (is_f32 ? 4 : 16) + 255) / 256); }
static int gemv_chunks(const bwgr_panel *P) { return gemv_chunks_of(P->data->is_f32, P->data->p); }
// The two launch rules without a device (test hook).  out: see include/bwgr.h.
extern "C" int bwgr_debug_aux_plan(int is_f32, int64_t p, int64_t ld, int64_t out[BWGR_AUX_PLAN_NOUT]) {
  if (!out || p < 1 || ld < 128 || ld % 128) return fail(BWGR_EINVAL, "debug_aux_plan: null pointer, p < 1 or ld not a positive multiple of 128");
  const int nchunks = gemv_chunks_of(is_f32 != 0, p), mpw = gather_mpw(is_f32 != 0, ld);
  const int64_t v[BWGR_AUX_PLAN_NOUT] = {nchunks, gemv_cpc_of(p, nchunks), (int64_t)gemv_row_wgs(is_f32 != 0, ld), mpw, (int64_t)gather_lds(mpw, ld)};
  std::copy(v, v + BWGR_AUX_PLAN_NOUT, out);
  return BWGR_OK;
}
template <typename CT>
static void gemv_launch(bwgr_panel *P, const CT *coef_dev, int nchunks, int cpc, double *part) {
  if (P->data->is_f32) {
    dim3 grid(gemv_row_wgs(true, P->data->plan.ld), (unsigned)nchunks);
    hipLaunchKernelGGL((k_gemv_part<float, CT>), grid, dim3(256), 0, P->stream, (const float *)P->data->X, P->data->plan.ld, P->data->plan.R, (int)P->data->p, coef_dev, cpc, part);
  } else {
    dim3 grid(gemv_row_wgs(false, P->data->plan.ld), (unsigned)nchunks);
    hipLaunchKernelGGL((k_gemv_part_i8<CT>), grid, dim3(256), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.ld, P->data->plan.R, (int)P->data->p, coef_dev, cpc, part);
  }
}

// hat = X*B + MU   (src/Rcpp20260726ai.cpp:629-630), fp64 accumulation, deterministic two-stage
template <typename CT>
static int gemv_hat(bwgr_panel *P, const CT *coef_dev, float MU, float *hat_dev, const char *who, bool centred = false) {
  const int nchunks = gemv_chunks(P);
  const int cpc = gemv_cpc_of(P->data->p, nchunks);
  DevBufs bufs;
  double *part = bufs.get<double>((size_t)nchunks * P->data->plan.ld + 1);
  if (!part) return fail(BWGR_ENOMEM, "%s: device allocation failed", who);
  gemv_launch<CT>(P, coef_dev, nchunks, cpc, part);
  double *cen_off = nullptr;
  if constexpr (std::is_same<CT, float>::value) {
    if (centred) {   // X_c B = X B - sum_j mean_j B_j
      cen_off = part + (size_t)nchunks * P->data->plan.ld;
      hipLaunchKernelGGL(k_cen_dot, dim3(1), dim3(1024), 0, P->stream, P->data->csum, coef_dev, P->data->p, 1.0 / (double)P->data->n, cen_off);
    }
  }
  hipLaunchKernelGGL(k_hat_finish, dim3((unsigned)((P->data->n + 255) / 256)), dim3(256), 0, P->stream, part, P->data->plan.ld, nchunks, (int)P->data->n, MU, hat_dev, (const double *)cen_off);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(P->stream));
  return BWGR_OK;
}

// Sweep the IMPLICITLY centred columns x_j - mean(x_j) of an int8 panel from now on (on != 0) or the raw columns again (on == 0): nothing is
// converted or copied -- the genotypes stay int8, the streamers, Gram arrays and MFMA tiles stay those of the raw columns, and the sequencer of
// k_sweep3 carries the scalar terms (sweep3.hip.h, "implicitly centred sweeps").  What changes for the callers: bwgr_panel_stats returns the centred
// columns' squared norms, the fused chains (bwgr_chain_*, bwgr_bayes, bwgr_group_*) run the reference's sweep on the centred columns
// (src/Rcpp20260726ai.cpp:668-682 with X_j - mean_j for X_j; selection models on k_sweep3 only), hat = X_c B + mu, and bwgr_panel_centred answers 1 -- which is
// what makes the marker-sharded sampler of several devices sound without a float copy of the panel.  Refused while chains are alive.
extern "C" int bwgr_panel_set_centred(bwgr_panel *P, int on) {
  if (!P) return fail(BWGR_EINVAL, "null panel");
  if (!P->is_root) return fail(BWGR_EINVAL, "panel_set_centred: set it on the root panel (clones follow it)");
  if (P->data->nchains_all > 0) return fail(BWGR_EINVAL, "panel_set_centred: %d chains are alive on this panel and its clones", P->data->nchains_all);
  HIPCHK(hipSetDevice(P->data->device));
  if (!on) { P->data->cen = false; return BWGR_OK; }
  if (P->data->is_f32) return fail(BWGR_EINVAL, "panel_set_centred: float panels are swept as given (centre the columns before the upload)");
  if (!P->data->e3_ready) return fail(BWGR_EINVAL, "panel_set_centred: this panel has no k_sweep3 (geometry or Gram range): the implicitly centred sweep is k_sweep3's");
  if (!P->data->csum) {   // the panel gets the pair once both arrays exist and are filled
    int32_t *csum = nullptr; float *xxc = nullptr;
    if (!P->data->own.take({{&csum, sizeof(int32_t) * (size_t)P->data->p}, {&xxc, sizeof(float) * (size_t)P->data->p}})) return no_memory("panel_set_centred");
    Guard drop([&] { P->data->own.drop(csum); P->data->own.drop(xxc); });
    const int wpb = 4;
    hipLaunchKernelGGL(k_colsum_i8, dim3((unsigned)((P->data->p + wpb - 1) / wpb)), dim3(64 * wpb), 0, P->stream, (const int8_t *)P->data->X, P->data->plan.R, (int)P->data->n, (int)P->data->p, csum, xxc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(P->stream));
    drop.release();
    P->data->csum = csum; P->data->xxc = xxc;
  }
  P->data->cen = true;
  return BWGR_OK;
}

// ---- are a panel's columns centred?  The marker-sharded partitioned sampler is statistically sound only then (DESIGN.md section 8:
// uncentred genotypes are all collinear through the mean direction, every shard corrects the same stale residual mean and the summed
// corrections overshoot; on centred columns 2 / 4 / 8 shards follow the exact chain: tools/centred_shard_probe.py).  From the panel's
// own statistics: mean_j^2 = (xx_j - (n - 1) vx_j) / n; a column counts as centred when |mean_j| <= 1e-3 sd_j. ----
extern "C" int bwgr_panel_centred(bwgr_panel *P, int *centred) {
  if (!P || !centred) return fail(BWGR_EINVAL, "null pointer");
  if (P->data->cen) { *centred = 1; return BWGR_OK; }   // implicitly centred: exactly
  HIPCHK(hipSetDevice(P->data->device));
  DevBufs bufs;
  int *flag = bufs.get<int>(1), h = 0;
  if (!flag) return fail(BWGR_ENOMEM, "panel_centred: device allocation failed");
  HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), P->stream));
  hipLaunchKernelGGL(k_uncentred, dim3(256), dim3(256), 0, P->stream, P->data->xx, P->data->vx, P->data->p, (double)P->data->n, flag);
  HIPCHK(d2h(P->stream, &h, flag, sizeof(int)));
  *centred = h ? 0 : 1;
  return BWGR_OK;
}

#include "samplers_host.hip.h"
#include "wgr_em_host.hip.h"
#include "group_host.hip.h"
#include "mtfit_host.hip.h"
#include "mrr_host.hip.h"
#include "uvb_host.hip.h"
#include "kernels_host.hip.h"
#include "pegs_host.hip.h"
#include "pegsx_host.hip.h"

// ------------------------------------------------------------------------------------------------
// synthetic data and test hooks
// ------------------------------------------------------------------------------------------------
extern "C" int bwgr_synth_genotypes(void *Xdev, int64_t n, int64_t p, int64_t ldx, int64_t col0, uint64_t seed,
                                    float *freq_dev, int device, void *hip_stream) {
  if (!Xdev || n < 1 || p < 1 || ldx < n || (ldx & 3)) return fail(BWGR_EINVAL, "synth: need ldx >= n and ldx %% 4 == 0");
  CHK(require_device(device));
  hipLaunchKernelGGL(k_synth, dim3(8192), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), (int8_t *)Xdev, ldx, (int)n, p, col0,
                     (uint32_t)seed, (uint32_t)(seed >> 32), freq_dev);
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}

// The grids of the tail, product and finish kernels of the fp64 families for a panel of n rows (ld padded), p markers and k columns of B: what
// the launch sites above use, by name, so that the tests' shape table (tests/tall_cases.py) fails when a grid changes.  Host arithmetic only.
extern "C" int bwgr_debug_launch_plan(int64_t n, int64_t ld, int64_t p, int64_t k, int64_t out[BWGR_LAUNCH_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "launch plan: null pointer");
  if (n < 1 || p < 1 || k < 1 || ld < n || ld % 128 != 0)
    return fail(BWGR_EINVAL, "launch plan: n = %lld, ld = %lld, p = %lld, k = %lld (each at least 1, ld >= n a multiple of 128)", (long long)n, (long long)ld, (long long)p, (long long)k);
  const PxbPlan xp = pxb_plan(ld, p, k);
  const int64_t v[BWGR_LAUNCH_PLAN_NOUT] = {
    MRR_NP, mrr_setup_grid(p), mrr_pass_grid(ld),
    UVB_NP, uvb_pass_grid(ld), uvb_shift_grid(n), uvb_xb_grid(n),
    PXB_ROWS, xp.tiles, xp.slices, xp.chunks, xp.chunk, pxb_finish_grid(n * k),
    XXT_ZERO_WG, KFIN_APPLY_WG, TAIL_THREADS, PXB_CHUNKS_MAX, PXB_MT};
  std::copy(v, v + BWGR_LAUNCH_PLAN_NOUT, out);
  return BWGR_OK;
}

extern "C" int bwgr_debug_variates(int device, uint64_t seed, int kind, double nu, uint32_t marker0, uint32_t iter,
                                   uint32_t purpose, int count, double *out_host) {
  if (!out_host || count < 1) return fail(BWGR_EINVAL, "debug_variates: bad arguments");
  CHK(require_device(device));
  DevBufs bufs;
  double *dev = bufs.get<double>((size_t)count);
  if (!dev) return fail(BWGR_ENOMEM, "debug_variates: device allocation failed");
  hipLaunchKernelGGL(k_debug_variates, dim3((count + 255) / 256), dim3(256), 0, 0, make_rng(seed, 0), kind, nu, marker0, iter, purpose, count, dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpy(out_host, dev, sizeof(double) * count, hipMemcpyDeviceToHost));
  return BWGR_OK;
}
