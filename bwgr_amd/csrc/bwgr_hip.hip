// bwgr_amd/csrc/bwgr_hip.hip -- libbwgr_hip.so, the one translation unit of the C ABI (include/bwgr.h).  This file holds what everything on
// the host stands on: error plumbing, the HIP backend of the holder, the handle structs and their small helpers, and three small entries at its
// end.  The rest is included by role: the switches (switches.h) and the panel plans (panel_plan.hip.h) in front of the handles that hold them;
// a sweep's planning and launching (sweep_host.hip.h) and the panel's building and entries (panel_host.hip.h) behind them; then every family's
// entries (the other *_host.hip.h files).  It defines no kernel: those are the *.hip.h files included at the top.
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
#include "xta.hip.h"
#include "mrr_svd_tail.h"
#include "project.hip.h"
#include "mlm_tail.h"
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
#include "switches.h"         // Switches, read_switches
#include "panel_plan.hip.h"   // PanelPlan / Panel3Plan and their planners: the handles below hold them

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
// Each of PanelData, bwgr_panel, bwgr_chain and bwgr_group owns its device arrays, streams and events through a holder (`own`); the typed
// pointers below are aliases, and deleting the struct releases them.  What is allocated lazily as a group is one take().  The sweep path too: a
// chain's timing pairs (EventPairs), a handle's guard event, hand-over event and draws group.  Only HipBackend creates or destroys a stream or an event.
// k_draws: the next iteration's state-independent variates, drawn on a second (low-priority) stream beside this iteration's sweep (draws_ahead)
struct DrawsAhead {
  double *buf = nullptr; hipStream_t stream = nullptr; hipEvent_t ready = nullptr, free = nullptr;   // the handle's holder's, one take()
  bool valid = false, unavailable = false;   // buf is (behind `ready`) what is described below; the set-up failed once and is not tried again
  Rng rng = {}; uint32_t iter = 0, marker0 = 0; int flags = 0, j0 = 0, j1 = 0; const void *sc = nullptr;
  // they are the variates of the sweep with arguments a over markers [j0_, j1_): same streams, same counters, same flags, this range inside theirs
  bool matches(const SweepArgs &a, int j0_, int j1_) const {
    return valid && iter == a.iter && marker0 == a.marker0 && flags == (a.flags & (SWF_SELECT | SWF_VB_VEC)) && sc == (const void *)a.sc && j0 <= j0_ && j1 >= j1_ &&
           memcmp(&rng, &a.rng, sizeof(Rng)) == 0 && !(a.flags & (SWF_MH | SWF_EM_ANY));
  }
  // the chain with scalars sc_ goes away: variates drawn ahead for it are nobody's now (k_draws reads the chain's df from them, so it is waited for)
  void forget(const void *sc_) {
    if (sc == sc_) { if (stream) (void)hipStreamSynchronize(stream); valid = false; sc = nullptr; }
  }
};

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
  std::vector<int> pair_users;             // ... and the handles on each right now (pair_stream_count): a pair takes an idle one before a new one is made
};

struct bwgr_panel {
  PanelData *data = nullptr;
  bool is_root = false;       // made with the data, which it frees; false: a clone
  DevBufs own;                // the sweep scratch, the exchange words, the lazy groups, a clone's stream, the draws group, the guard and hand-over events
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
  DrawsAhead draws;           // the next iteration's variates, drawn beside this iteration's sweep (draws_ahead)
  // occupancy guard: the compute units this handle's enqueued sweeps hold while they run, the stream they run on, and an event behind the last of them
  hipEvent_t guard_ev = nullptr; int guard_cus = 0; hipStream_t guard_stream = nullptr; bool guard_listed = false;
  hipEvent_t handover_ev = nullptr;   // for the handle's moves between streams (hand_over); like guard_ev the holder's, made on first use
  int debug_withhold = 0;     // test hook: the next sweeps run with slab workgroup 0 missing (bwgr_debug_withhold)
  int nchains = 0;            // live chains on this handle: panel_destroy refuses while any is alive
};

struct bwgr_chain {
  bwgr_panel *P = nullptr;
  DevBufs own;                        // the state arrays (e: unless the caller gave one) and the timing pairs' events
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
  EventPairs<HipBackend> timing;      // a pair around each sweep launch since the last bwgr_chain_sweep_ms
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
// stream `later` goes on after what is pending on stream `earlier`: ev is recorded on earlier, and later waits for it.  (The wait captures the
// event's state when it is enqueued, so an event that is recorded again later still serves its earlier waits: one event per owner is enough.)
static hipError_t stream_after(hipStream_t later, hipStream_t earlier, hipEvent_t ev) {
  const hipError_t e = hipEventRecord(ev, earlier);
  return e != hipSuccess ? e : hipStreamWaitEvent(later, ev, 0);
}
// ... through *ev, an event of `own` made the first time: a handle's own hand-over event (onto a pair's stream and back), or a call's
static hipError_t hand_over(DevBufs &own, hipEvent_t *ev, hipStream_t later, hipStream_t earlier) {
  if (!*ev && !(*ev = own.event(hipEventDisableTiming))) return hipErrorOutOfMemory;
  return stream_after(later, earlier, *ev);
}

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


// what every family's entries share: a sweep's plan and launch train, then the panel's building and its entries
#include "sweep_host.hip.h"
#include "panel_host.hip.h"
// the families' entries
#include "samplers_host.hip.h"
#include "wgr_em_host.hip.h"
#include "group_host.hip.h"
#include "mtfit_host.hip.h"
#include "mrr_host.hip.h"
#include "mrr_svd_host.hip.h"
#include "mlm_host.hip.h"
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
