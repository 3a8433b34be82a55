// bwgr_amd/csrc/group_host.hip.h -- the host entries of the multi-GPU group: the RCCL loader, bwgr_group and the bwgr_group_* entries.  Part of
// bwgr_hip.hip, which includes it after samplers_host.hip.h (the chains it drives) and everything else it uses (fail, HIPCHK, DevBufs, no_memory,
// Guard, bwgr_panel_set_centred / bwgr_panel_centred); it defines no kernel: k_group_sum is chain.hip.h's.
// ------------------------------------------------------------------------------------------------
// Multi-GPU inside the library (row e): bwgr_group_* -- one marker shard per device of this process, the residual replicated,
// ONE host thread, one stream per device, RCCL all-reduces of the residual delta (n fp64) on those streams at the exchange
// rounds.  This is what an R process (the reference's only host, R/wgr.R:2) needs in order to use more than one GPU through a
// .Call; bwgr_amd/dist.py remains the torchrun driver of the benchmark (one process per GPU).  For G > 1 this is the
// partitioned sampler of DESIGN.md section 8 (statistical parity); G = 1 is the plain exact chain.
// RCCL is loaded with dlopen on first use, so single-GPU users never touch it.
// ------------------------------------------------------------------------------------------------
#include <dlfcn.h>
namespace {
typedef struct ncclComm *bwgr_ncclComm_t;
struct RcclApi {
  void *h = nullptr;
  int (*CommInitAll)(bwgr_ncclComm_t *, int, const int *) = nullptr;
  int (*CommDestroy)(bwgr_ncclComm_t) = nullptr;
  int (*AllReduce)(const void *, void *, size_t, int, int, bwgr_ncclComm_t, hipStream_t) = nullptr;
  int (*GroupStart)() = nullptr;
  int (*GroupEnd)() = nullptr;
  const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load() {
  if (g_rccl.h) return BWGR_OK;
  void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return fail(BWGR_EHIP, "group: cannot load librccl.so (%s)", dlerror());
  RcclApi a; a.h = h;
  a.CommInitAll = (int (*)(bwgr_ncclComm_t *, int, const int *))dlsym(h, "ncclCommInitAll");
  a.CommDestroy = (int (*)(bwgr_ncclComm_t))dlsym(h, "ncclCommDestroy");
  a.AllReduce = (int (*)(const void *, void *, size_t, int, int, bwgr_ncclComm_t, hipStream_t))dlsym(h, "ncclAllReduce");
  a.GroupStart = (int (*)())dlsym(h, "ncclGroupStart");
  a.GroupEnd = (int (*)())dlsym(h, "ncclGroupEnd");
  a.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
  if (!a.CommInitAll || !a.CommDestroy || !a.AllReduce || !a.GroupStart || !a.GroupEnd) return fail(BWGR_EHIP, "group: librccl.so lacks an expected symbol");
  g_rccl = a;
  return BWGR_OK;
}
constexpr int BWGR_NCCL_FLOAT64 = 8, BWGR_NCCL_SUM = 0;   // ncclFloat64, ncclSum (rccl.h)
}  // namespace

struct bwgr_group {
  int G = 0;
  int model = 0;
  int64_t n = 0, p = 0;
  int block = 0, bps = 1, rounds = 1;
  std::vector<int> dev;
  std::vector<int64_t> lo, hi;
  std::vector<bwgr_panel *> P;
  std::vector<bwgr_chain *> C;
  std::vector<std::unique_ptr<DevBufs>> own;   // [g], on shard g's device: delta, sums, and of shards side by side the stream and ev_sweep (own[0]: ev_sum, total, total_sums)
  std::vector<double *> delta, sums;
  std::vector<bwgr_ncclComm_t> comm;
  bool use_comm = false;
  bool centred = true;        // every shard's columns are centred (bwgr_panel_centred): what makes G > 1 statistically sound
  float MSx_total = 0;
  // several shards on ONE device (every entry of `devices` equal): the shards' sweeps run side by side on their own streams, each on its own
  // compute units, and an exchange round is a sum kernel between events -- no RCCL.  One exact chain is a latency-bound pipeline that fills a
  // third of the chip; the partitioned sampler's shards fill the rest.
  bool same_dev = false;
  std::vector<hipStream_t> streams;
  std::vector<hipEvent_t> ev_sweep;      // [g]: shard g's round_sweep (or sums) is enqueued up to here
  hipEvent_t ev_sum[2] = {nullptr, nullptr};
  double *total[2] = {nullptr, nullptr}; // the summed residual deltas of a round, by round parity (ld doubles each); total_sums likewise (2 doubles)
  double *total_sums[2] = {nullptr, nullptr};
  uint64_t round_no = 0;
};

extern "C" int bwgr_group_destroy(bwgr_group *Gp) {
  if (!Gp) return BWGR_OK;
  for (size_t g = 0; g < Gp->C.size(); ++g) if (Gp->C[g]) bwgr_chain_destroy(Gp->C[g]);
  for (size_t g = 0; g < Gp->P.size(); ++g) {
    (void)hipSetDevice(Gp->dev[g]);
    if (Gp->P[g]) bwgr_panel_destroy(Gp->P[g]);
  }
  if (Gp->use_comm) for (bwgr_ncclComm_t c : Gp->comm) if (c) g_rccl.CommDestroy(c);
  for (size_t g = 0; g < Gp->own.size(); ++g) { (void)hipSetDevice(Gp->dev[g]); Gp->own[g].reset(); }
  delete Gp;
  return BWGR_OK;
}

// X: HOST matrix, column-major n x p (ldx >= n), any bwgr_xtype; y: n host floats.  Device g of `devices` stages the
// block-aligned column shard [lo_g, hi_g) (as bwgr_amd/dist.py::shard_bounds) and runs the chain of that shard.
// markers_per_sync: markers swept per device between two residual all-reduces (0: 131072 / ndev, the benchmark's default; 131072 for shards
// side by side on one device).
extern "C" int bwgr_group_sound(const bwgr_group *Gp, int *sound);

static int group_create_impl(bwgr_group **out, int ndev, const int *devices, const void *X, int xtype, int64_t n, int64_t p,
                             int64_t ldx, int block, const float *y, int model, float it, float bi, float pi, float df, float R2,
                             uint64_t seed, int rng_mode, int64_t markers_per_sync, int centre, int memloc = BWGR_HOST) {
  if (!out || !devices || !X || !y) return fail(BWGR_EINVAL, "group_create: null pointer");
  if (memloc != BWGR_HOST && memloc != BWGR_DEVICE) return fail(BWGR_EINVAL, "group_create: bad memloc %d", memloc);
  if (memloc == BWGR_DEVICE && ndev > 1 && !std::all_of(devices, devices + ndev, [&](int d) { return d == devices[0]; }))
    return fail(BWGR_EINVAL, "group_create: a device-resident X serves shards of that one device only");
  if (centre && xtype != BWGR_X_I8) return fail(BWGR_EINVAL, "group_create_centred: implicit centring is for int8 genotypes (centre float columns before the call)");
  *out = nullptr;
  if (ndev < 1 || ndev > 64) return fail(BWGR_EINVAL, "group_create: ndev = %d", ndev);
  for (int g = 1; g < ndev; ++g) for (int h = 0; h < g; ++h)
    if (devices[g] == devices[h] && !std::all_of(devices, devices + ndev, [&](int d) { return d == devices[0]; }))
      return fail(BWGR_EINVAL, "group_create: a device may appear once, or every shard sits on the same device (shards side by side on one GPU)");
  if (xtype != BWGR_X_I8 && xtype != BWGR_X_F32 && xtype != BWGR_X_F64) return fail(BWGR_EINVAL, "group_create: bad xtype %d", xtype);
  const int mmax = (xtype == BWGR_X_I8) ? SW_MAXM : 64;
  const int m = block > 0 ? block : mmax;
  const int64_t nblk = (p + m - 1) / m, per = (nblk + ndev - 1) / ndev;
  if ((int64_t)(ndev - 1) * per * m >= p) return fail(BWGR_EINVAL, "group_create: p = %lld has only %lld blocks of %d markers: too few for %d devices", (long long)p, (long long)nblk, m, ndev);
  bwgr_group *Gp = new bwgr_group();
  Gp->G = ndev; Gp->model = model; Gp->n = n; Gp->p = p; Gp->block = m;
  Gp->dev.assign(devices, devices + ndev);
  Gp->same_dev = ndev > 1 && std::all_of(devices, devices + ndev, [&](int d) { return d == devices[0]; });
  Gp->P.assign(ndev, nullptr); Gp->C.assign(ndev, nullptr); Gp->delta.assign(ndev, nullptr); Gp->sums.assign(ndev, nullptr);
  for (int g = 0; g < ndev; ++g) Gp->own.emplace_back(new DevBufs());
  Guard drop([&] { bwgr_group_destroy(Gp); });
  const size_t esz = (xtype == BWGR_X_I8) ? 1 : (xtype == BWGR_X_F32 ? 4 : 8);
  double msx = 0.0;
  for (int g = 0; g < ndev; ++g) {
    const int64_t lo = std::min<int64_t>(p, (int64_t)g * per * m), hi = std::min<int64_t>(p, (int64_t)(g + 1) * per * m);
    Gp->lo.push_back(lo); Gp->hi.push_back(hi);
    CHK(bwgr_panel_create(&Gp->P[g], reinterpret_cast<const unsigned char *>(X) + (size_t)lo * (size_t)ldx * esz, xtype, memloc, n, hi - lo, ldx, devices[g], m, 0));
    if (Gp->same_dev) {   // shards of one device: each on a stream of its own; from three shards on, 256-row streamers (K3 + 1 units a shard instead of 2 K3 + 2)
      hipStream_t q = Gp->own[g]->stream(hipStreamNonBlocking, 0);
      if (!q) return fail(BWGR_EHIP, "group_create: no stream for shard %d", g);
      Gp->streams.push_back(q);
      Gp->P[g]->stream = q;   // (no wait: bwgr_panel_create hands a panel over with nothing pending on its stream)
      if (ndev > 2 && Gp->P[g]->data->sw.solo3 < 0) Gp->P[g]->data->crowded = true;   // (an explicit BWGR_SOLO3 decides otherwise: experiments)
    }
    if (centre) CHK(bwgr_panel_set_centred(Gp->P[g], 1));   // the shard's own column means (rows are not sharded)
    msx += (double)Gp->P[g]->data->MSx;
    int cen = 1;
    CHK(bwgr_panel_centred(Gp->P[g], &cen));
    if (!cen) Gp->centred = false;
  }
  Gp->MSx_total = (float)msx;
  if (ndev > 1 && !Gp->centred) {
    if (!Gp->P[0]->data->sw.group_allow_uncentred)
      return fail(BWGR_EINVAL, "group_create: the columns of X are not centred, and on uncentred columns the marker-sharded sampler of %d devices is "
                               "statistically unsound (every shard corrects the same stale residual mean: DESIGN.md section 8).  Pass centred columns "
                               "(x_j - mean(x_j), float: the posterior of b and hat is the same under the sampler's flat intercept prior), use one "
                               "device, or set BWGR_GROUP_ALLOW_UNCENTRED=1 to run it knowingly", ndev);
  }
  for (int g = 0; g < ndev; ++g) {
    CHK(bwgr_chain_create_sharded(&Gp->C[g], Gp->P[g], model, y, BWGR_HOST, it, bi, pi, df, R2, seed, rng_mode, Gp->lo[g], p, Gp->MSx_total, nullptr));
    if (hipSetDevice(devices[g]) != hipSuccess || !Gp->own[g]->take({{&Gp->delta[g], sizeof(double) * (size_t)Gp->P[g]->data->plan.ld}, {&Gp->sums[g], sizeof(double) * 2}}))
      return no_memory("group_create");
    if (Gp->P[g]->data->plan.ld != Gp->P[0]->data->plan.ld) return fail(BWGR_EINVAL, "group_create: shards disagree on the padded row count");
  }
  // (shards side by side exchange through one kernel on the same card, not a ring over xGMI, but every exchange is a launch boundary for all of
  // them: 131072 markers per shard between two exchanges there)
  const int64_t mps = markers_per_sync > 0 ? markers_per_sync : std::max<int64_t>(m, Gp->same_dev ? 131072 : 131072 / ndev);
  Gp->bps = (int)std::max<int64_t>(1, mps / m);
  int64_t nbmax = 0;
  for (int g = 0; g < ndev; ++g) nbmax = std::max<int64_t>(nbmax, Gp->P[g]->data->plan.nblocks);
  Gp->rounds = (int)((nbmax + Gp->bps - 1) / Gp->bps);
  Gp->use_comm = (ndev > 1 && !Gp->same_dev) || (Gp->P[0]->data->sw.group_force_comm && !Gp->same_dev);   // (BWGR_GROUP_FORCE_COMM=1, tests: exercise the RCCL path with a single device)
  if (Gp->same_dev) {
    if (hipSetDevice(devices[0]) != hipSuccess) return fail(BWGR_EHIP, "group_create: hipSetDevice failed");
    Gp->ev_sweep.assign(ndev, nullptr);
    for (int g = 0; g < ndev; ++g) if (!(Gp->ev_sweep[g] = Gp->own[g]->event(hipEventDisableTiming))) return fail(BWGR_EHIP, "group_create: no event for shard %d's sweeps", g);
    for (int k = 0; k < 2; ++k) {
      if (!Gp->own[0]->take({DevBufs::want_event(&Gp->ev_sum[k], hipEventDisableTiming), {&Gp->total[k], sizeof(double) * (size_t)Gp->P[0]->data->plan.ld}, {&Gp->total_sums[k], sizeof(double) * 2}}))
        return no_memory("group_create");
    }
  }
  if (Gp->use_comm) {
    CHK(rccl_load());
    Gp->comm.assign(ndev, nullptr);
    const int nr = g_rccl.CommInitAll(Gp->comm.data(), ndev, devices);
    if (nr != 0) return fail(BWGR_EHIP, "group_create: ncclCommInitAll failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nr) : "?");
  }
  drop.release();
  *out = Gp;
  return BWGR_OK;
}

extern "C" int bwgr_group_create(bwgr_group **out, int ndev, const int *devices, const void *X, int xtype, int64_t n, int64_t p,
                                 int64_t ldx, int block, const float *y, int model, float it, float bi, float pi, float df, float R2,
                                 uint64_t seed, int rng_mode, int64_t markers_per_sync) {
  return group_create_impl(out, ndev, devices, X, xtype, n, p, ldx, block, y, model, it, bi, pi, df, R2, seed, rng_mode, markers_per_sync, 0);
}
// ... on the implicitly centred columns of an int8 matrix (bwgr_panel_set_centred on every shard): sound with several devices, int8 in HBM
extern "C" int bwgr_group_create_centred(bwgr_group **out, int ndev, const int *devices, const void *X, int xtype, int64_t n, int64_t p,
                                         int64_t ldx, int block, const float *y, int model, float it, float bi, float pi, float df, float R2,
                                         uint64_t seed, int rng_mode, int64_t markers_per_sync, int memloc) {
  return group_create_impl(out, ndev, devices, X, xtype, n, p, ldx, block, y, model, it, bi, pi, df, R2, seed, rng_mode, markers_per_sync, 1, memloc);
}
static int group_allreduce(bwgr_group *Gp, std::vector<double *> &buf, size_t count) {
  int nr = g_rccl.GroupStart();
  for (int g = 0; g < Gp->G && nr == 0; ++g)
    nr = g_rccl.AllReduce(buf[g], buf[g], count, BWGR_NCCL_FLOAT64, BWGR_NCCL_SUM, Gp->comm[g], Gp->P[g]->stream);
  const int ne = g_rccl.GroupEnd();
  if (nr == 0) nr = ne;
  if (nr != 0) return fail(BWGR_EHIP, "group: ncclAllReduce failed: %s", g_rccl.GetErrorString ? g_rccl.GetErrorString(nr) : "?");
  return BWGR_OK;
}

extern "C" int bwgr_group_sound(const bwgr_group *Gp, int *sound) {
  if (!Gp || !sound) return fail(BWGR_EINVAL, "null pointer");
  *sound = (Gp->G == 1 || Gp->centred) ? 1 : 0;   // one device: the exact chain; more: sound on centred columns only
  return BWGR_OK;
}

// one exchange among the shards of one device: every shard's stream has produced buf[g]; stream 0 sums them into `total` (by round parity, so
// that the readers of the previous round are never overwritten: a buffer's next writer waits for events that every reader's stream records later)
static int group_local_sum(bwgr_group *Gp, std::vector<double *> &buf, size_t count, double *const total[2], double **out) {
  const int k = (int)(Gp->round_no++ & 1u);
  SumPtrs sp;
  for (int g = 0; g < Gp->G; ++g) { sp.src[g] = buf[g]; HIPCHK(hipEventRecord(Gp->ev_sweep[g], Gp->streams[g])); }
  for (int g = 1; g < Gp->G; ++g) HIPCHK(hipStreamWaitEvent(Gp->streams[0], Gp->ev_sweep[g], 0));
  hipLaunchKernelGGL(k_group_sum, dim3((unsigned)std::min<size_t>(64, (count + 255) / 256)), dim3(256), 0, Gp->streams[0], sp, Gp->G, total[k], (int64_t)count);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(Gp->ev_sum[k], Gp->streams[0]));
  for (int g = 1; g < Gp->G; ++g) HIPCHK(hipStreamWaitEvent(Gp->streams[g], Gp->ev_sum[k], 0));
  *out = total[k];
  return BWGR_OK;
}
static int group_run_same_device(bwgr_group *Gp, int iters) {
  HIPCHK(hipSetDevice(Gp->dev[0]));
  for (int k = 0; k < iters; ++k) {
    for (int r = 0; r < Gp->rounds; ++r) {
      for (int g = 0; g < Gp->G; ++g) {
        const int nb = (int)Gp->P[g]->data->plan.nblocks;
        const int lo = std::min(nb, r * Gp->bps), hi = std::min(nb, (r + 1) * Gp->bps);
        CHK(bwgr_chain_round_sweep(Gp->C[g], lo, hi, Gp->delta[g]));
      }
      double *tot = nullptr;
      CHK(group_local_sum(Gp, Gp->delta, (size_t)Gp->P[0]->data->plan.ld, Gp->total, &tot));
      for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_round_apply(Gp->C[g], tot));
    }
    for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_get_sums_dev(Gp->C[g], Gp->sums[g]));
    double *tot2 = nullptr;
    CHK(group_local_sum(Gp, Gp->sums, 2, Gp->total_sums, &tot2));
    for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_end_iteration_dev(Gp->C[g], tot2));
  }
  return BWGR_OK;
}

extern "C" int bwgr_group_run(bwgr_group *Gp, int iters) {
  if (!Gp) return fail(BWGR_EINVAL, "null group");
  if (iters < 0) return fail(BWGR_EINVAL, "group_run: iters < 0");
  if (Gp->same_dev) return group_run_same_device(Gp, iters);
  if (!Gp->use_comm) return bwgr_chain_run(Gp->C[0], iters);   // one device: the plain exact chain
  for (int k = 0; k < iters; ++k) {
    for (int r = 0; r < Gp->rounds; ++r) {
      for (int g = 0; g < Gp->G; ++g) {
        const int nb = (int)Gp->P[g]->data->plan.nblocks;
        const int lo = std::min(nb, r * Gp->bps), hi = std::min(nb, (r + 1) * Gp->bps);   // (lo == hi: a device that has run out of blocks still takes part)
        CHK(bwgr_chain_round_sweep(Gp->C[g], lo, hi, Gp->delta[g]));
      }
      CHK(group_allreduce(Gp, Gp->delta, (size_t)Gp->P[0]->data->plan.ld));
      for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_round_apply(Gp->C[g], Gp->delta[g]));
    }
    for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_get_sums_dev(Gp->C[g], Gp->sums[g]));
    CHK(group_allreduce(Gp, Gp->sums, 2));
    for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_end_iteration_dev(Gp->C[g], Gp->sums[g]));
  }
  return BWGR_OK;
}

extern "C" int bwgr_group_sync(bwgr_group *Gp) {
  if (!Gp) return fail(BWGR_EINVAL, "null group");
  for (int g = 0; g < Gp->G; ++g) CHK(bwgr_chain_sync(Gp->C[g]));
  return BWGR_OK;
}

extern "C" int bwgr_group_info(const bwgr_group *Gp, int64_t info[4]) {
  if (!Gp || !info) return fail(BWGR_EINVAL, "null pointer");
  info[0] = Gp->G; info[1] = Gp->rounds; info[2] = (int64_t)Gp->bps * Gp->block; info[3] = Gp->use_comm ? 1 : 0;
  return BWGR_OK;
}

// the reference's return list over the whole panel (host outputs; any may be NULL): b, d, pval: p floats; vb: p floats for the
// per-marker-variance models, else 1; hat: n floats
extern "C" int bwgr_group_result(bwgr_group *Gp, float *mu, float *b, float *d, float *hat, float *vb, float *ve, float *h2,
                                 float *MSx, float *pi_out, float *pval) {
  if (!Gp) return fail(BWGR_EINVAL, "null group");
  const bool per = per_marker_vb(Gp->model);
  std::vector<float> hg(hat ? (size_t)Gp->n : 0), vbl;
  float mu0 = 0, ve0 = 0, h20 = 0, msx0 = 0, pi0 = 0, vbs = 0;
  double vg = 0.0;
  if (hat) for (int64_t i = 0; i < Gp->n; ++i) hat[i] = 0.0f;
  for (int g = 0; g < Gp->G; ++g) {
    const int64_t lo = Gp->lo[g], pg = Gp->hi[g] - lo;
    float mug, veg, h2g, msxg, pig;
    vbl.assign(per ? (size_t)pg : 1, 0.0f);
    CHK(bwgr_chain_result(Gp->C[g], &mug, b ? b + lo : nullptr, d ? d + lo : nullptr, hat ? hg.data() : nullptr, vbl.data(), &veg, &h2g,
                          &msxg, &pig, pval ? pval + lo : nullptr));
    if (g == 0) { mu0 = mug; ve0 = veg; h20 = h2g; msx0 = msxg; pi0 = pig; vbs = vbl[0]; }
    if (per) { for (int64_t j = 0; j < pg; ++j) { vg += (double)vbl[(size_t)j]; if (vb) vb[lo + j] = vbl[(size_t)j]; } }
    if (hat) for (int64_t i = 0; i < Gp->n; ++i) hat[i] += hg[(size_t)i] - mug;   // X_g B_g
  }
  if (hat) for (int64_t i = 0; i < Gp->n; ++i) hat[i] += mu0;
  if (!per && vb) vb[0] = vbs;
  if (mu) *mu = mu0;
  if (ve) *ve = ve0;
  if (h2) *h2 = per ? (float)(vg / (vg + (double)ve0)) : h20;   // (the common-variance models form vg from MSx over all shards already)
  if (MSx) *MSx = msx0;
  if (pi_out) *pi_out = pi0;
  return BWGR_OK;
}
