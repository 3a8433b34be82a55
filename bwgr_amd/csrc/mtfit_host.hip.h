// bwgr_amd/csrc/mtfit_host.hip.h -- the host scaffolding of the multi-trait fits: what bwgr_mrr (mrr_host.hip.h), bwgr_pegs (pegs_host.hip.h) and
// bwgr_pegsx (pegsx_host.hip.h) do alike around their own algebra.  Part of bwgr_hip.hip, before mrr_host.hip.h; it defines no kernel (they are
// mrr.hip.h and pegs.hip.h) and no entry but the plan hooks of the plans it holds.
//   the plans:   mrr_plan (LDS of k_mrr_solve / k_mrr_linv), pegs_dense_plan (the dense leg), pegs_sparse_plan (the sparse legs), the grids
//                the launch sites share
//   mrr_sweep:   one panel design's share of a sweep
//   mrrd_sweep:  a dense design's share of a sweep on the block train of mrr_dense.hip.h, and its plan (mrr_dense_plan)
//   MtList:      what an effect list says, checked on the host (mt_check_effects, worded with the caller's name)
//   MtFit:       a fit's masks, device arrays and effects, and one member function per step the entries repeat; the entries keep their loops
// ------------------------------------------------------------------------------------------------
// The LDS plan of k_mrr_solve and k_mrr_linv for k traits and npat missingness patterns, decided here and nowhere else: the solve stages
// the markers' k x k inverses (64 k^2 doubles) when they fit beside its fixed arrays, then as many of the block's per-pattern Gram matrices
// as the rest of the budget holds (ngl); it reads patterns ngl.. from global memory, and without linv_lds fetches each marker's row of
// its inverse one marker ahead.  bwgr_debug_mrr_plan exposes it to the CPU tests.
static constexpr size_t MRR_LDS_MAX = 160 * 1024;
static constexpr int MRR_NP = 64;             // workgroups (= partials) of the tail reductions k_mrr_ey and k_mrr_tilde, 256 rows or markers each per trip
static constexpr int MRR_SETUP_WG = 8192;     // workgroups of k_mrr_setup_cols at most, four markers (one per wave) each per trip
static constexpr int TAIL_THREADS = 256;      // threads per workgroup of the tail, product and finish kernels of the fp64 families
// the grids the launch sites below and bwgr_debug_launch_plan share
static inline int64_t mrr_setup_grid(int64_t p) { return std::min<int64_t>((p + 3) / 4, MRR_SETUP_WG); }
static inline int64_t mrr_pass_grid(int64_t ld) { return std::min<int64_t>(ld / 64, MRR_PASS_WG); }
struct MrrPlan { int linv_lds, ngl; size_t lds_solve, lds_linv; };
static MrrPlan mrr_plan(int k, int npat) {
  MrrPlan pl;
  const size_t lds_fixed = mrr_solve_lds(0, 0), linv_b = sizeof(double) * MRR_MB * k * k;
  pl.linv_lds = lds_fixed + linv_b <= MRR_LDS_MAX ? 1 : 0;
  pl.ngl = (int)std::min<size_t>((size_t)npat, (MRR_LDS_MAX - lds_fixed - (pl.linv_lds ? linv_b : 0)) / (MRR_MB * MRR_MB * 4));
  pl.lds_solve = mrr_solve_lds(pl.ngl, pl.linv_lds ? MRR_MB * k * k : 0);
  pl.lds_linv = linv_b;
  return pl;
}
extern "C" int bwgr_debug_mrr_plan(int k, int npat, int *linv_lds, int *ngl, int64_t *solve_lds_bytes, int64_t *linv_lds_bytes) {
  if (k < 1 || k > MRR_KMAX || npat < 1 || npat > k) return BWGR_EINVAL;
  const MrrPlan pl = mrr_plan(k, npat);
  if (linv_lds) *linv_lds = pl.linv_lds;
  if (ngl) *ngl = pl.ngl;
  if (solve_lds_bytes) *solve_lds_bytes = (int64_t)pl.lds_solve;
  if (linv_lds_bytes) *linv_lds_bytes = (int64_t)pl.lds_linv;
  return BWGR_OK;
}

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

// The sparse legs' plan, decided here and nowhere else (bwgr_debug_pegs_sparse_plan exposes it to the CPU tests): the set-up kernel and the
// disjoint leg run one column per wave, four per workgroup and trip; the serial leg is one wave; the disjoint leg is taken exactly where the
// host found no row in two columns and the caller did not force the serial leg.
struct PegsSparsePlan { int setup_threads, serial_threads, disjoint_threads, disjoint; int64_t setup_wg, serial_wg, disjoint_wg, trip_cols; size_t ws_bytes; };
static PegsSparsePlan pegs_sparse_plan(int64_t n, int64_t q, int64_t nnz, int k, bool disjoint) {
  PegsSparsePlan pl;
  pl.setup_threads = TAIL_THREADS; pl.setup_wg = std::min<int64_t>((q + 3) / 4, MRR_SETUP_WG);
  pl.serial_threads = 64; pl.serial_wg = 1;
  pl.disjoint_threads = 256; pl.disjoint_wg = std::min<int64_t>((q + 3) / 4, PEGS_SPARSE_WG);
  pl.trip_cols = pl.disjoint_wg * 4;
  pl.disjoint = disjoint ? 1 : 0;
  const size_t nq = (size_t)q, qk = nq * (size_t)k, nz = (size_t)nnz;
  pl.ws_bytes = 2 * nz * (sizeof(double) + sizeof(int32_t)) + sizeof(int64_t) * (nq + 1 + (size_t)n + 1)       // CSC and CSR
                + sizeof(double) * (5 * qk + qk * (size_t)k + MRR_KMAX) + sizeof(int32_t) * nq;                   // XX, XSX, tilde, b, d2; Linv; db2; order
  return pl;
}
extern "C" int bwgr_debug_pegs_sparse_plan(int64_t n, int64_t q, int64_t nnz, int64_t max_col_nnz, int k, int disjoint, int64_t out[BWGR_PEGS_SPARSE_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "pegs sparse plan: null pointer");
  if (n < 1 || q < 1 || nnz < 0 || nnz > CSC_MAX_NNZ || max_col_nnz < 0 || max_col_nnz > nnz || max_col_nnz > n || k < 1 || k > BWGR_MRR_MAXK)
    return fail(BWGR_EINVAL, "pegs sparse plan: n = %lld, q = %lld (each at least 1), nnz = %lld (0 .. 2^31 - 1), max_col_nnz = %lld (0 .. min(nnz, n)), k = %d (1 <= k <= %d)",
                (long long)n, (long long)q, (long long)nnz, (long long)max_col_nnz, k, BWGR_MRR_MAXK);
  const PegsSparsePlan pl = pegs_sparse_plan(n, q, nnz, k, disjoint != 0);
  out[0] = pl.setup_threads; out[1] = pl.setup_wg; out[2] = pl.serial_threads; out[3] = pl.serial_wg; out[4] = pl.disjoint_threads; out[5] = pl.disjoint_wg;
  out[6] = pl.trip_cols; out[7] = pl.disjoint; out[8] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

// workgroups of k_pegs_dense_setup for an effect of q columns: one column per wave, four per workgroup and trip (MtFit::setup_effect and
// bwgr_debug_pegs_launch_plan share it)
static inline int64_t pegs_dense_setup_grid(int64_t q) { return std::min<int64_t>((q + 3) / 4, MRR_SETUP_WG); }

// One design's share of a sweep (:866-902): what its launch train reads and writes on the device.  bwgr_mrr has one; bwgr_pegs one per
// panel effect, all against the same residual (MrrSweepShared).
struct MrrLeg {
  const bwgr_panel *P = nullptr;
  int64_t p = 0, nblk = 0;
  int8_t *Xs = nullptr; int32_t *ordd = nullptr, *gram = nullptr;
  double *xbar = nullptr, *Sd = nullptr, *XXd = nullptr, *XSXd = nullptr, *tilde = nullptr, *bd = nullptr, *Linv = nullptr, *db2 = nullptr;
};
struct MrrSweepShared {
  int64_t ld; int G, npat;
  const uint32_t *ztd; const uint8_t *zmd;
  double *ed, *part, *dB, *iGd;     // the residual [trait][ld]; the pass's partial dots; the block's delta b; k x k staging of iG
};
// (the caller asks bufs.failed() once, after all its gets)
static void mrr_leg_alloc(DevBufs &bufs, MrrLeg &L, const bwgr_panel *P, int npat, int k) {
  L.P = P; L.p = P->data->p; L.nblk = (L.p + MRR_MB - 1) / MRR_MB;
  const size_t np = (size_t)L.p, pk = np * k;
  L.Xs = bufs.get<int8_t>(P->data->plan.x_bytes);
  L.ordd = bufs.get<int32_t>(np); L.gram = bufs.get<int32_t>((size_t)L.nblk * npat * MRR_MB * MRR_MB);
  L.xbar = bufs.get<double>(np); L.Sd = bufs.get<double>(npat * np);
  L.XXd = bufs.get<double>(pk); L.XSXd = bufs.get<double>(pk); L.tilde = bufs.get<double>(pk); L.bd = bufs.get<double>(pk); L.Linv = bufs.get<double>(pk * k);
  L.db2 = bufs.get<double>(MRR_KMAX);
}
// order -> k_permute_cols -> k_mrr_gram -> k_mrr_linv -> [k_mrr_pass(b-1 | b), k_mrr_solve(b)] for every block -> k_mrr_pass(last | -);
// mc.iVe and iG (host, k x k) are the sweep's.  Leaves sum_j (delta b_jt)^2 in L.db2.
static int mrr_sweep(hipStream_t st, const MrrLeg &L, const MrrSweepShared &W, const MrrConst &mc, const MrrPlan &plan, const std::vector<int> &order,
                     const double *iG) {
  const PanelData *D = L.P->data;
  const int R = D->plan.R, k = mc.k, npat = W.npat, G = W.G;
  const int64_t p = L.p, ld = W.ld, nblk = L.nblk;
  const int cps = (int)((size_t)R / 16);
  HIPCHK(h2d(st, L.ordd, order.data(), (size_t)p));
  hipLaunchKernelGGL(k_permute_cols, dim3(8192), dim3(256), 0, st, (const uint4 *)D->X, (uint4 *)L.Xs, (const int32_t *)L.ordd, p, D->plan.K, cps);
  hipLaunchKernelGGL(k_mrr_gram, dim3((unsigned)nblk, (unsigned)((npat + 3) / 4)), dim3(256), 0, st, (const int8_t *)L.Xs, R, p, ld, W.zmd, npat, L.gram);
  HIPCHK(h2d(st, W.iGd, iG, (size_t)k * k));
  hipLaunchKernelGGL(k_mrr_linv, dim3((unsigned)((p + 63) / 64)), dim3(64), plan.lds_linv, st, (const double *)L.XXd, (const double *)W.iGd, mc, p, L.Linv);
  HIPCHK(zero(st, L.db2, (size_t)MRR_KMAX));
  HIPCHK(hipGetLastError());
  for (int64_t blk = 0; blk <= nblk; ++blk) {
    MrrPassArgs pa; pa.Xs = L.Xs; pa.R = R; pa.p = p; pa.ld = ld; pa.nblk = (int)nblk; pa.zb = W.ztd; pa.e = W.ed; pa.dB = W.dB; pa.part = W.part;
    pa.prev = blk > 0 ? (int)(blk - 1) : -1; pa.next = blk < nblk ? (int)blk : -1; pa.k = k;
    hipLaunchKernelGGL(k_mrr_pass, dim3(G), dim3(256), 0, st, pa);
    if (blk == nblk) break;
    MrrSolveArgs sa; sa.part = W.part; sa.G = G; sa.order = L.ordd; sa.blk = (int)blk; sa.p = p; sa.gram = L.gram; sa.xbar = L.xbar; sa.S = L.Sd; sa.XX = L.XXd;
    sa.Linv = L.Linv; sa.b = L.bd; sa.dB = W.dB; sa.db2 = L.db2; sa.ngl = plan.ngl; sa.linv_lds = plan.linv_lds;
    hipLaunchKernelGGL(k_mrr_solve, dim3(1), dim3(256), plan.lds_solve, st, sa, mc);
  }
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}

// The dense train's plan (mrr_dense.hip.h), decided here and nowhere else: bwgr_debug_mrr_dense_plan exposes it to the
// CPU tests, and mrrd_leg_alloc, mrrd_sweep and bwgr_mrr_dense take every grid, LDS size and array length from it.  The solve's LDS is
// mrr_plan's arithmetic with an fp64 Gram: a pattern's matrix is 32 KB, so at most 3 or 4 are staged and the rest are read from global memory.
struct MrrDensePlan {
  int64_t ld, nblk, edge, tiles, pass_wg, trips, cols_wg, hat_wg;   // edge: columns of the last block; trips: tiles a pass workgroup takes at most
  int linv_lds, ngl;
  size_t lds_gram, lds_pass, lds_solve, lds_linv, ws_bytes;
};
static MrrDensePlan mrr_dense_plan(int64_t n, int64_t r, int k, int npat) {
  MrrDensePlan pl;
  pl.ld = (n + 127) / 128 * 128;
  pl.nblk = (r + MRR_MB - 1) / MRR_MB;
  pl.edge = r - (pl.nblk - 1) * MRR_MB;
  pl.tiles = pl.ld / 64;
  pl.pass_wg = mrr_pass_grid(pl.ld);
  pl.trips = (pl.tiles + pl.pass_wg - 1) / pl.pass_wg;
  pl.cols_wg = mrr_setup_grid(r);                                   // k_mrrd_centre and k_mrrd_setup: one column per wave, four per workgroup and trip
  pl.hat_wg = (n + 255) / 256;
  const size_t lds_fixed = mrrd_solve_lds(0, 0), linv_b = sizeof(double) * MRR_MB * k * k, gram_b = sizeof(double) * MRR_MB * MRR_MB;
  pl.linv_lds = lds_fixed + linv_b <= MRR_LDS_MAX ? 1 : 0;
  pl.ngl = (int)std::min<size_t>((size_t)npat, (MRR_LDS_MAX - lds_fixed - (pl.linv_lds ? linv_b : 0)) / gram_b);
  pl.lds_solve = mrrd_solve_lds(pl.ngl, pl.linv_lds ? MRR_MB * k * k : 0);
  pl.lds_linv = linv_b;
  pl.lds_gram = sizeof(double) * 2 * MRRD_GT * MRRD_GP + sizeof(int) * MRR_MB;                                  // (static, for the record)
  pl.lds_pass = sizeof(double) * (MRR_MB * MRRD_XP + 64 * MRR_KMAX + MRR_MB * MRR_KMAX) + sizeof(int) * 2 * MRR_MB;
  const size_t nl = (size_t)pl.ld, nr = (size_t)r, rk = nr * (size_t)k;
  pl.ws_bytes = sizeof(double) * (nl * nr + (size_t)pl.nblk * npat * MRR_MB * MRR_MB + 4 * rk + rk * k + MRR_KMAX)   // X_c, Grams, XX XSX tilde b, Linv, db2
                + sizeof(int32_t) * nr                                                                               // the order
                + 2 * sizeof(uint32_t) * nl + (size_t)npat * nl + sizeof(double) * (2 * (size_t)k * nl + (size_t)n * k)   // masks, y, e, hat
                + sizeof(double) * ((size_t)pl.pass_wg * (MRR_MB + 1) * MRR_KMAX + MRR_MB * MRR_KMAX + MRR_KMAX + 1024 + (size_t)MRR_NP * (MRR_KMAX * MRR_KMAX + MRR_KMAX) + MRR_KMAX);
  return pl;
}
extern "C" int bwgr_debug_mrr_dense_plan(int64_t n, int64_t r, int k, int npat, int64_t out[BWGR_MRR_DENSE_PLAN_NOUT]) {
  if (!out) return fail(BWGR_EINVAL, "mrr_dense plan: null pointer");
  if (n < 2 || r < 1 || r > 0x7FFFFF00ll || k < 1 || k > BWGR_MRR_MAXK || npat < 1 || npat > k)
    return fail(BWGR_EINVAL, "mrr_dense plan: n = %lld (at least 2), r = %lld (1 .. 2147483392), k = %d (1 <= k <= %d), npat = %d (1 <= npat <= k)",
                (long long)n, (long long)r, k, BWGR_MRR_MAXK, npat);
  const MrrDensePlan pl = mrr_dense_plan(n, r, k, npat);
  out[0] = pl.ld; out[1] = pl.nblk; out[2] = pl.edge; out[3] = pl.tiles; out[4] = pl.pass_wg; out[5] = pl.trips; out[6] = pl.cols_wg; out[7] = pl.hat_wg;
  out[8] = pl.linv_lds; out[9] = pl.ngl; out[10] = (int64_t)pl.lds_gram; out[11] = (int64_t)pl.lds_pass; out[12] = (int64_t)pl.lds_solve;
  out[13] = (int64_t)pl.lds_linv; out[14] = (int64_t)pl.ws_bytes;
  return BWGR_OK;
}

// A dense design's share of a sweep on the train of mrr_dense.hip.h, against the same residual (MrrSweepShared) as mrr_sweep's
struct MrrDenseLeg {
  int64_t r = 0;
  double *Xc = nullptr, *gram = nullptr, *XXd = nullptr, *XSXd = nullptr, *tilde = nullptr, *bd = nullptr, *Linv = nullptr, *db2 = nullptr;
  int32_t *ordd = nullptr;
};
// (the caller asks bufs.failed() once, after all its gets)
static void mrrd_leg_alloc(DevBufs &bufs, MrrDenseLeg &L, const MrrDensePlan &pl, int64_t r, int npat, int k) {
  L.r = r;
  const size_t nr = (size_t)r, rk = nr * k;
  L.Xc = bufs.get<double>((size_t)pl.ld * nr); L.gram = bufs.get<double>((size_t)pl.nblk * npat * MRR_MB * MRR_MB);
  L.XXd = bufs.get<double>(rk); L.XSXd = bufs.get<double>(rk); L.tilde = bufs.get<double>(rk); L.bd = bufs.get<double>(rk); L.Linv = bufs.get<double>(rk * k);
  L.db2 = bufs.get<double>(MRR_KMAX); L.ordd = bufs.get<int32_t>(nr);
}
// order -> k_mrrd_gram -> k_mrr_linv -> [k_mrrd_pass(b-1 | b), k_mrrd_solve(b)] for every block -> k_mrrd_pass(last | -); mc.iVe and iG (host,
// k x k) are the sweep's.  zbd: the pattern words.  Leaves sum_j (delta b_jt)^2 in L.db2.
static int mrrd_sweep(hipStream_t st, const MrrDenseLeg &L, const MrrSweepShared &W, const uint32_t *zbd, const MrrConst &mc, const MrrDensePlan &pl,
                      const std::vector<int> &order, const double *iG) {
  const int k = mc.k, npat = W.npat;
  const int64_t r = L.r, ld = W.ld, nblk = pl.nblk;
  HIPCHK(h2d(st, L.ordd, order.data(), (size_t)r));
  hipLaunchKernelGGL(k_mrrd_gram, dim3((unsigned)nblk, (unsigned)npat), dim3(256), 0, st, (const double *)L.Xc, ld, r, (const int32_t *)L.ordd, zbd, npat, L.gram);
  HIPCHK(h2d(st, W.iGd, iG, (size_t)k * k));
  hipLaunchKernelGGL(k_mrr_linv, dim3((unsigned)((r + 63) / 64)), dim3(64), pl.lds_linv, st, (const double *)L.XXd, (const double *)W.iGd, mc, r, L.Linv);
  HIPCHK(zero(st, L.db2, (size_t)MRR_KMAX));
  HIPCHK(hipGetLastError());
  for (int64_t blk = 0; blk <= nblk; ++blk) {
    MrrdPassArgs pa; pa.X = L.Xc; pa.r = r; pa.ld = ld; pa.order = L.ordd; pa.zt = W.ztd; pa.e = W.ed; pa.dB = W.dB; pa.part = W.part;
    pa.prev = blk > 0 ? (int)(blk - 1) : -1; pa.next = blk < nblk ? (int)blk : -1; pa.k = k;
    hipLaunchKernelGGL(k_mrrd_pass, dim3((unsigned)pl.pass_wg), dim3(256), 0, st, pa);
    if (blk == nblk) break;
    MrrdSolveArgs sa; sa.part = W.part; sa.G = (int)pl.pass_wg; sa.order = L.ordd; sa.blk = (int)blk; sa.r = r; sa.gram = L.gram; sa.XX = L.XXd; sa.Linv = L.Linv;
    sa.b = L.bd; sa.dB = W.dB; sa.db2 = L.db2; sa.ngl = pl.ngl; sa.linv_lds = pl.linv_lds;
    hipLaunchKernelGGL(k_mrrd_solve, dim3(1), dim3(256), pl.lds_solve, st, sa, mc);
  }
  HIPCHK(hipGetLastError());
  return BWGR_OK;
}

// a dense effect on the device
struct PegsDense {
  int64_t q = 0;
  double *Zd = nullptr, *XXd = nullptr, *XSXd = nullptr, *tilde = nullptr, *bd = nullptr, *Linv = nullptr, *db2 = nullptr;
  int32_t *ordd = nullptr;
};

// a sparse effect on the device: the matrix column-compressed (the legs) and row-major (the fitted values)
struct PegsSparse {
  int64_t q = 0, nnz = 0;
  bool disjoint = false;                   // the leg a sweep takes (the plan's verdict)
  int64_t *colptr = nullptr, *rowptr = nullptr;
  int32_t *rowidx = nullptr, *colidx = nullptr, *ordd = nullptr;
  double *val = nullptr, *rval = nullptr, *XXd = nullptr, *XSXd = nullptr, *tilde = nullptr, *bd = nullptr, *Linv = nullptr, *db2 = nullptr, *d2 = nullptr;
};

// ------------------------------------------------------------------------------------------------
// What an effect list says, checked on the host.  It is a thing of its own, and not part of MtFit, because a call reads its traits in between:
// they need the list's ld, and are copied from asynchronously, so they are declared before the MtFit (see there).
struct MtList {
  const bwgr_pegs_effect_ex *eff = nullptr;
  int neff = 0;
  int64_t n = 0, ld = 0;
  const bwgr_panel *P0 = nullptr;          // the first panel effect: its device, its row padding and its stream are the fit's
  hipStream_t st = nullptr;
  std::vector<std::vector<double>> Zc;     // per dense effect, Z without its padding rows (MtFit takes them over)
  std::vector<CsrCopy> csr;                // per sparse effect, its row-major copy (MtFit takes them over)
  std::vector<char> disjoint;              // per sparse effect, whether no row occurs in two columns
  bool train = false;                      // a dense effect is swept by the block train of mrr_dense.hip.h (bwgr_mrr_dense), not by the dense leg
};
// The refusals every effect list meets, worded with the caller's name (`coef`: what it calls an effect's coefficients); none needs a device.
// Then the device: the first panel's, or `device` where every effect is dense.
static int mt_check_effects(const char *who, const char *coef, const bwgr_pegs_effect_ex *eff, int neff, int64_t n, int device, double *const *outs, MtList &E) {
  E.eff = eff; E.neff = neff; E.n = n;
  for (int e = 0; e < neff; ++e) {
    if (!outs[e]) return fail(BWGR_EINVAL, "%s: null pointer (%s of effect %d)", who, coef, e);
    const bwgr_panel *P = eff[e].panel;
    if (P) {
      if (P->data->is_f32) return fail(BWGR_EINVAL, "%s: effect %d's panel holds fp32 genotypes; %s takes int8 panels only", who, e, who);
      if (P->data->n != n) return fail(BWGR_EINVAL, "%s: effect %d has %lld rows, Y %lld", who, e, (long long)P->data->n, (long long)n);
      if (!E.P0) E.P0 = P;
      if (P->data->device != E.P0->data->device)
        return fail(BWGR_EINVAL, "%s: effect %d's panel is on device %d, the first panel on device %d", who, e, P->data->device, E.P0->data->device);
      if (P->data->plan.ld != E.P0->data->plan.ld)
        return fail(BWGR_EINVAL, "%s: effect %d's panel pads its rows to ld = %lld, the first panel to %lld (make the panels with the same block / nwg)", who, e,
                    (long long)P->data->plan.ld, (long long)E.P0->data->plan.ld);
    } else if (eff[e].colptr) {
      if (eff[e].Z) return fail(BWGR_EINVAL, "%s: effect %d has both Z and colptr (a dense and a sparse effect at once)", who, e);
      if (!eff[e].rowidx || !eff[e].val) return fail(BWGR_EINVAL, "%s: null pointer (rowidx or val of sparse effect %d)", who, e);
      if (eff[e].q < 1 || eff[e].q > 0x7FFFFF00ll)
        return fail(BWGR_EINVAL, "%s: sparse effect %d: q = %lld columns (at least 1, at most 2147483392)", who, e, (long long)eff[e].q);
      CscFault bad;
      if (!csc_validate(n, eff[e].q, eff[e].colptr, eff[e].rowidx, eff[e].val, bad))
        return fail(BWGR_EINVAL, "%s: sparse effect %d: %s (column %lld, entry %lld; n = %lld rows, q = %lld columns)", who, e, csc_why(bad.what), (long long)bad.col,
                    (long long)bad.entry, (long long)n, (long long)eff[e].q);
    } else {
      if (!eff[e].Z) return fail(BWGR_EINVAL, "%s: effect %d has neither a panel nor Z nor colptr", who, e);
      if (eff[e].q < 1 || eff[e].q > 0x7FFFFF00ll || eff[e].ldz < n)
        return fail(BWGR_EINVAL, "%s: effect %d: q = %lld columns of Z, ldz = %lld (q at least 1, ldz at least n = %lld)", who, e, (long long)eff[e].q,
                    (long long)eff[e].ldz, (long long)n);
    }
  }
  E.Zc.resize((size_t)neff); E.csr.resize((size_t)neff); E.disjoint.assign((size_t)neff, 0);
  for (int e = 0; e < neff; ++e)
    if (!eff[e].panel && eff[e].colptr) {
      E.disjoint[(size_t)e] = csc_row_disjoint(n, eff[e].q, eff[e].colptr, eff[e].rowidx) ? 1 : 0;
      csc_to_csr(n, eff[e].q, eff[e].colptr, eff[e].rowidx, eff[e].val, E.csr[(size_t)e]);
    } else if (!eff[e].panel) {
      int64_t r = 0, j = 0;
      if (!compact_z(eff[e].Z, n, eff[e].q, eff[e].ldz, E.Zc[(size_t)e], &r, &j))
        return fail(BWGR_EINVAL, "%s: effect %d: Z[%lld, %lld] is not finite", who, e, (long long)r, (long long)j);
    }
  if (E.P0) HIPCHK(hipSetDevice(E.P0->data->device)); else CHK(require_device(device));
  E.ld = E.P0 ? E.P0->data->plan.ld : (n + 127) / 128 * 128;
  E.st = E.P0 ? E.P0->stream : nullptr;
  return BWGR_OK;
}

// one effect of a fit: a panel's leg, a sparse or a dense effect, and what the entries read of any
struct MtEffect {
  bool panel = false, sparse = false, train = false;   // train: a dense design on the block train (dl), not on the dense leg (dense)
  int64_t m = 0;                           // its columns
  MrrLeg leg; PegsDense dense; PegsSparse sp; MrrDenseLeg dl;
  double *b() const { return train ? dl.bd : panel ? leg.bd : sparse ? sp.bd : dense.bd; }
  double *tilde() const { return train ? dl.tilde : panel ? leg.tilde : sparse ? sp.tilde : dense.tilde; }
  double *XX() const { return train ? dl.XXd : panel ? leg.XXd : sparse ? sp.XXd : dense.XXd; }
  double *XSX() const { return train ? dl.XSXd : panel ? leg.XSXd : sparse ? sp.XSXd : dense.XSXd; }
  double *db2() const { return train ? dl.db2 : panel ? leg.db2 : sparse ? sp.db2 : dense.db2; }
};

// A multi-trait fit on the device: k traits over the rows of an effect list, all effects against one residual.  An entry makes one after its
// checks and its traits, then masks() -> alloc() (and its own gets; it asks bufs.failed() once) -> upload(), and calls the steps from its own
// loops.  Every step enqueues on st what the entries enqueued there before, in the same order; the ones that return results end in d2h's wait.
struct MtFit {
  // Host data.  What an asynchronous copy reads -- Zc, csr, order, the mask words, d, off -- stands BEFORE bufs: members go away in reverse order, so
  // the holder's wait for the stream comes first (devbufs.h; tests/devbufs_check.cpp shows the semantics).  The same holds for what a caller
  // hands to upload() and sweep_effect(): its traits and its iG are declared before its MtFit.
  const int64_t n, ld; const int k; const hipStream_t st;
  std::vector<std::vector<double>> Zc;
  std::vector<CsrCopy> csr;
  const bwgr_pegs_effect_ex *src;          // the caller's effects: a sparse effect's CSC arrays are copied from where they are
  std::vector<CumulativeOrder> order;      // per effect, the column order of sweep s
  bool natural_order = false;              // every sweep walks the columns 0, 1, ... (mrr_svd, :1176): the orders stay the identity they start as
  std::vector<uint32_t> zt, zb;            // bit t: row observed for trait t; bit g: row observed in pattern g
  std::vector<uint8_t> zm;
  std::vector<double> d, off;              // k each, for stage_vec(): the mu shift (or the TH form's diagonal); the fitted values' offset (zero unless written)
  MrrConst mc;                             // (the entries set iVe before every sweep)
  int npat = 0, G = 0, nch_max = 1;
  MrrPlan plan; PegsDensePlan dpl; MrrDensePlan tpl;   // tpl: of the one effect on the dense train, where there is one
  // Device data
  DevBufs bufs;
  uint32_t *zbd = nullptr, *ztd = nullptr; uint8_t *zmd = nullptr;
  double *yd = nullptr, *ed = nullptr, *part = nullptr, *dB = nullptr, *tpart = nullptr, *sumyd = nullptr, *hatd = nullptr, *hpart = nullptr, *htmp = nullptr;
  static constexpr size_t SMALL_IG = 512, SMALL_VEC = 768, SMALL_LEN = 1024;
  double *small = nullptr, *iGd = nullptr, *vecd = nullptr;   // small: [0, SMALL_IG) reduction results; iGd = small + SMALL_IG: k x k; vecd = small + SMALL_VEC: a staged k-vector
  std::vector<MtEffect> eff;
  MrrSweepShared W;

  MtFit(MtList &E, int k_) : n(E.n), ld(E.ld), k(k_), st(E.st), Zc(std::move(E.Zc)), csr(std::move(E.csr)), src(E.eff), d((size_t)k_), off((size_t)k_, 0.0), bufs(E.st),
                              eff((size_t)E.neff) {
    for (int e = 0; e < E.neff; ++e) {
      eff[(size_t)e].panel = E.eff[e].panel != nullptr;
      eff[(size_t)e].sparse = !E.eff[e].panel && E.eff[e].colptr != nullptr;
      eff[(size_t)e].train = E.train && !eff[(size_t)e].panel && !eff[(size_t)e].sparse;
      if (eff[(size_t)e].sparse) {
        eff[(size_t)e].sp.nnz = E.eff[e].colptr[E.eff[e].q];
        eff[(size_t)e].sp.disjoint = pegs_sparse_plan(E.n, E.eff[e].q, eff[(size_t)e].sp.nnz, k_, E.disjoint[(size_t)e] && !(E.eff[e].flags & BWGR_PEGS_SERIAL)).disjoint != 0;
      }
      eff[(size_t)e].leg.P = E.eff[e].panel;
      eff[(size_t)e].m = E.eff[e].panel ? E.eff[e].panel->data->p : E.eff[e].q;
      order.emplace_back((size_t)eff[(size_t)e].m);
    }
  }
  // MrrConst and the mask words from the traits and their missingness patterns
  void masks(const TraitSet &S, const Patterns &pat) {
    npat = (int)pat.rep.size();
    memset(&mc, 0, sizeof(mc));
    mc.k = k; mc.npat = npat;
    for (int t = 0; t < k; ++t) { mc.pt[t] = pat.id[(size_t)t]; mc.nt[t] = S.nt[(size_t)t]; }
    zt.resize((size_t)ld); zb.resize((size_t)ld);
    pack_row_bits(S, (int64_t)0, k, zt.data());
    pack_row_bits(S, pat.rep.data(), npat, zb.data());
    append_byte_masks(S, pat.rep.data(), npat, zm);
  }
  // every array of the fit and of its effects; `summed`: the effects' fitted values are added up in hatd, a panel's through htmp
  void alloc(bool want_hat, bool summed) {
    const size_t nl = (size_t)ld, nn = (size_t)n;
    G = (int)mrr_pass_grid(ld);
    zbd = bufs.get<uint32_t>(nl); ztd = bufs.get<uint32_t>(nl); zmd = bufs.get<uint8_t>((size_t)npat * nl);
    yd = bufs.get<double>(k * nl); ed = bufs.get<double>(k * nl);
    part = bufs.get<double>((size_t)G * (MRR_MB + 1) * MRR_KMAX); dB = bufs.get<double>(MRR_MB * MRR_KMAX + MRR_KMAX);
    small = bufs.get<double>(SMALL_LEN);
    if (small) { iGd = small + SMALL_IG; vecd = small + SMALL_VEC; }
    tpart = bufs.get<double>((size_t)MRR_NP * (MRR_KMAX * MRR_KMAX + MRR_KMAX)); sumyd = bufs.get<double>(MRR_KMAX);
    bool panels = false;
    for (MtEffect &E : eff) {
      if (E.panel) {
        mrr_leg_alloc(bufs, E.leg, E.leg.P, npat, k);
        nch_max = std::max(nch_max, (int)std::min<int64_t>(64, E.m));
        panels = true;
      } else if (E.train) {
        tpl = mrr_dense_plan(n, E.m, k, npat);
        mrrd_leg_alloc(bufs, E.dl, tpl, E.m, npat, k);
      } else if (E.sparse) {
        PegsSparse &S = E.sp;
        S.q = E.m;
        const size_t nq = (size_t)S.q, qk = nq * k, nz = std::max<size_t>((size_t)S.nnz, 1);
        S.colptr = bufs.get<int64_t>(nq + 1); S.rowidx = bufs.get<int32_t>(nz); S.val = bufs.get<double>(nz);
        S.rowptr = bufs.get<int64_t>(nn + 1); S.colidx = bufs.get<int32_t>(nz); S.rval = bufs.get<double>(nz);
        S.XXd = bufs.get<double>(qk); S.XSXd = bufs.get<double>(qk); S.tilde = bufs.get<double>(qk); S.bd = bufs.get<double>(qk); S.d2 = bufs.get<double>(qk);
        S.Linv = bufs.get<double>(qk * k); S.db2 = bufs.get<double>(MRR_KMAX); S.ordd = bufs.get<int32_t>(nq);
      } else {
        PegsDense &D = E.dense;
        D.q = E.m;
        const size_t nq = (size_t)D.q, qk = nq * k;
        D.Zd = bufs.get<double>(nn * nq); D.XXd = bufs.get<double>(qk); D.XSXd = bufs.get<double>(qk); D.tilde = bufs.get<double>(qk); D.bd = bufs.get<double>(qk);
        D.Linv = bufs.get<double>(qk * k); D.db2 = bufs.get<double>(MRR_KMAX); D.ordd = bufs.get<int32_t>(nq);
      }
    }
    if (want_hat) hatd = bufs.get<double>(nn * k);
    if (want_hat && panels) hpart = bufs.get<double>((size_t)nch_max * k * nl);
    if (want_hat && panels && summed) htmp = bufs.get<double>(nn * k);
    plan = mrr_plan(k, npat);
    dpl = pegs_dense_plan(n, 1, k);
    W = {ld, G, npat, ztd, zmd, ed, part, dB, iGd};
  }
  // the masks, y, e = y and the traits' sums (sumy == nullptr: zeros, for a fit that centres nothing)
  int upload(const TraitSet &S, const double *sumy) {
    const size_t nl = (size_t)ld;
    HIPCHK(h2d(st, zbd, zb.data(), nl));
    HIPCHK(h2d(st, ztd, zt.data(), nl));
    HIPCHK(h2d(st, zmd, zm.data(), zm.size()));
    HIPCHK(h2d(st, yd, S.y.data(), k * nl));
    HIPCHK(h2d(st, ed, S.y.data(), k * nl));
    if (sumy) HIPCHK(h2d(st, sumyd, sumy, (size_t)k)); else HIPCHK(zero(st, sumyd, (size_t)MRR_KMAX));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_linv), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrr_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_mrrd_solve), hipFuncAttributeMaxDynamicSharedMemorySize, (int)MRR_LDS_MAX));
    return BWGR_OK;
  }
  // a dense effect's Z, a sparse effect's two copies; b = 0
  int stage_effect(int e) {
    const MtEffect &E = eff[(size_t)e];
    if (E.sparse) {
      const PegsSparse &S = E.sp;
      const CsrCopy &R = csr[(size_t)e];
      HIPCHK(h2d(st, S.colptr, src[e].colptr, (size_t)S.q + 1));
      HIPCHK(h2d(st, S.rowptr, R.rowptr.data(), (size_t)n + 1));
      if (S.nnz > 0) {
        HIPCHK(h2d(st, S.rowidx, src[e].rowidx, (size_t)S.nnz));
        HIPCHK(h2d(st, S.val, src[e].val, (size_t)S.nnz));
        HIPCHK(h2d(st, S.colidx, R.col.data(), (size_t)S.nnz));
        HIPCHK(h2d(st, S.rval, R.val.data(), (size_t)S.nnz));
      }
    } else if (!E.panel && !E.train) HIPCHK(h2d(st, E.dense.Zd, Zc[(size_t)e].data(), Zc[(size_t)e].size()));   // (a train's design: stage_train)
    HIPCHK(zero(st, E.b(), (size_t)E.m * k));
    return BWGR_OK;
  }
  // The design of an effect on the dense train into its padded copy, centred by its all-rows column means.  Host X (column stride ldx = ld, read
  // asynchronously: it outlives the fit) or device X of column stride ldx.
  int stage_train(int e, const double *X, int64_t ldx, bool on_device) {
    const MrrDenseLeg &L = eff[(size_t)e].dl;
    if (on_device) {
      hipLaunchKernelGGL(k_mrrd_centre, dim3((unsigned)tpl.cols_wg), dim3(TAIL_THREADS), 0, st, X, ldx, n, L.r, ld, L.Xc);
    } else {
      HIPCHK(h2d(st, L.Xc, X, (size_t)ld * (size_t)L.r));
      hipLaunchKernelGGL(k_mrrd_centre, dim3((unsigned)tpl.cols_wg), dim3(TAIL_THREADS), 0, st, (const double *)L.Xc, ld, n, L.r, ld, L.Xc);
    }
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // The design of an effect on the dense train written by the caller, uncentred: fill(copy, ld) enqueues on st what writes the n x r design
  // into the padded copy, zeros on its rows n .. ld-1 (MLM: the projection of mlm_host.hip.h).  Everything after runs in the centre = 0 mode.
  template <typename Fill> int stage_train_by(int e, Fill fill) {
    CHK(fill(eff[(size_t)e].dl.Xc, ld));
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // out (n x k) = the train effect's X_c b plus the staged k-vector, for every row
  int train_hat(int e, double *out) {
    const MrrDenseLeg &L = eff[(size_t)e].dl;
    hipLaunchKernelGGL(k_mrrd_hat, dim3((unsigned)tpl.hat_wg), dim3(256), 0, st, (const double *)L.Xc, n, L.r, ld, k, (const double *)L.bd, (const double *)vecd, out);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // XX, XSX and tilde of the effect's columns, one launch: a panel's centred where `centre` (then xbar too), a dense or sparse effect's as they are
  int setup_effect(int e, int centre) {
    const MtEffect &E = eff[(size_t)e];
    if (E.train) {
      hipLaunchKernelGGL(k_mrrd_setup, dim3((unsigned)tpl.cols_wg), dim3(TAIL_THREADS), 0, st, (const double *)E.dl.Xc, n, E.dl.r, ld, (const uint32_t *)zbd,
                         (const double *)yd, mc, E.dl.XXd, E.dl.XSXd, E.dl.tilde);
    } else if (E.panel) {
      const MrrLeg &L = E.leg;
      const PanelData *D = L.P->data;
      hipLaunchKernelGGL(k_mrr_setup_cols, dim3((unsigned)mrr_setup_grid(L.p)), dim3(TAIL_THREADS), 0, st, (const int8_t *)D->X, D->plan.R, (int)n, L.p, ld,
                         (const uint32_t *)zbd, (const double *)yd, (const double *)sumyd, mc, centre, L.xbar, L.Sd, L.XXd, L.XSXd, L.tilde);
    } else if (E.sparse) {
      const PegsSparse &S = E.sp;
      const PegsSparsePlan sp = pegs_sparse_plan(n, S.q, S.nnz, k, S.disjoint);
      hipLaunchKernelGGL(k_pegs_sparse_setup, dim3((unsigned)sp.setup_wg), dim3(sp.setup_threads), 0, st, (const int64_t *)S.colptr, (const int32_t *)S.rowidx,
                         (const double *)S.val, S.q, ld, (const uint32_t *)ztd, (const double *)yd, mc, S.XXd, S.XSXd, S.tilde);
    } else {
      const PegsDense &D = E.dense;
      hipLaunchKernelGGL(k_pegs_dense_setup, dim3((unsigned)pegs_dense_setup_grid(D.q)), dim3(TAIL_THREADS), 0, st, (const double *)D.Zd, n, D.q, ld,
                         (const uint32_t *)ztd, (const double *)yd, mc, D.XXd, D.XSXd, D.tilde);
    }
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // A reduction over an effect's m columns, partials in a fixed order: the k^2 products b'tilde (mode 0; mode 1: the TH form with its k traces, iG's
  // diagonal at dvec), or the k column sums of `third` (mode 2)
  int reduce(const double *b, const double *tilde, const double *third, int64_t m, int mode, int nout, const double *dvec, double *out) {
    hipLaunchKernelGGL(k_mrr_tilde, dim3(MRR_NP, nout), dim3(256), 0, st, b, tilde, third, m, mode, mc, dvec, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, MRR_NP, nout, small);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, out, small, sizeof(double) * nout));
    return BWGR_OK;
  }
  // effect e's share of sweep `numit`, against mc.iVe and iG (host, k x k): mrr_sweep, or k_mrr_linv -> k_pegs_dense_leg, or k_mrr_linv ->
  // k_pegs_sparse_leg / k_pegs_sparse_leg_disjoint -> db2 from the per-column (delta b)^2 in column-index order
  int sweep_effect(int e, int numit, const double *iG) {
    const std::vector<int> &ord = natural_order ? order[(size_t)e].current() : order[(size_t)e].next(numit);
    if (eff[(size_t)e].train) return mrrd_sweep(st, eff[(size_t)e].dl, W, zbd, mc, tpl, ord, iG);
    if (eff[(size_t)e].panel) return mrr_sweep(st, eff[(size_t)e].leg, W, mc, plan, ord, iG);
    if (eff[(size_t)e].sparse) {
      const PegsSparse &S = eff[(size_t)e].sp;
      const PegsSparsePlan sp = pegs_sparse_plan(n, S.q, S.nnz, k, S.disjoint);
      HIPCHK(h2d(st, S.ordd, ord.data(), (size_t)S.q));
      HIPCHK(h2d(st, iGd, iG, (size_t)k * k));
      hipLaunchKernelGGL(k_mrr_linv, dim3((unsigned)((S.q + 63) / 64)), dim3(64), plan.lds_linv, st, (const double *)S.XXd, (const double *)iGd, mc, S.q, S.Linv);
      PegsSparseArgs A;
      A.colptr = S.colptr; A.rowidx = S.rowidx; A.val = S.val; A.ld = ld; A.q = S.q; A.zt = ztd; A.e = ed; A.order = S.ordd; A.XX = S.XXd; A.Linv = S.Linv;
      A.b = S.bd; A.d2 = S.d2;
      if (sp.disjoint) hipLaunchKernelGGL(k_pegs_sparse_leg_disjoint, dim3((unsigned)sp.disjoint_wg), dim3(sp.disjoint_threads), 0, st, A, mc);
      else hipLaunchKernelGGL(k_pegs_sparse_leg, dim3((unsigned)sp.serial_wg), dim3(sp.serial_threads), 0, st, A, mc);
      hipLaunchKernelGGL(k_mrr_tilde, dim3(MRR_NP, k), dim3(256), 0, st, (const double *)S.bd, (const double *)S.tilde, (const double *)S.d2, S.q, 2, mc,
                         (const double *)nullptr, tpart);
      hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, MRR_NP, k, S.db2);
      HIPCHK(hipGetLastError());
      return BWGR_OK;
    }
    const PegsDense &D = eff[(size_t)e].dense;
    HIPCHK(h2d(st, D.ordd, ord.data(), (size_t)D.q));
    HIPCHK(h2d(st, iGd, iG, (size_t)k * k));
    hipLaunchKernelGGL(k_mrr_linv, dim3((unsigned)((D.q + 63) / 64)), dim3(64), plan.lds_linv, st, (const double *)D.XXd, (const double *)iGd, mc, D.q, D.Linv);
    PegsLegArgs A;
    A.Z = D.Zd; A.n = n; A.ld = ld; A.q = (int)D.q; A.zt = ztd; A.e = ed; A.order = D.ordd; A.XX = D.XXd; A.Linv = D.Linv; A.b = D.bd; A.db2 = D.db2;
    hipLaunchKernelGGL(k_pegs_dense_leg, dim3(1), dim3(dpl.threads), dpl.lds_bytes, st, A, mc);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // ey[0, k): e'y per trait over its observed rows; ey[k, 2k): the sums of e
  int residual_sums(double *ey) {
    hipLaunchKernelGGL(k_mrr_ey, dim3(MRR_NP, k), dim3(256), 0, st, (const double *)ed, (const double *)yd, ld, k, tpart);
    hipLaunchKernelGGL(k_mrr_finish, dim3(1), dim3(256), 0, st, (const double *)tpart, MRR_NP, 2 * k, small);
    HIPCHK(hipGetLastError());
    HIPCHK(d2h(st, ey, small, sizeof(double) * 2 * k));
    return BWGR_OK;
  }
  // sum_j (delta b_jt)^2 of the effect's last sweep, per trait
  int read_db2(int e, double *out) { HIPCHK(d2h(st, out, eff[(size_t)e].db2(), sizeof(double) * k)); return BWGR_OK; }
  // after a sweep: TH[s * k + t] = sum_j b_js tilde_jt, and the sweep's sum of (delta b)^2 over the traits
  int effect_sums(int e, double *TH, double *db2) {
    const MtEffect &E = eff[(size_t)e];
    double t_[MRR_KMAX];
    CHK(reduce(E.b(), E.tilde(), E.XSX(), E.m, 0, k * k, nullptr, TH));
    CHK(read_db2(e, t_));
    *db2 = 0.0;
    for (int t = 0; t < k; ++t) *db2 += t_[t];
    return BWGR_OK;
  }
  // v (d or off) into the staged k-vector
  int stage_vec(const std::vector<double> &v) { HIPCHK(h2d(st, vecd, v.data(), (size_t)k)); return BWGR_OK; }
  // e -= d on every trait's observed rows
  int mu_shift() {
    CHK(stage_vec(d));
    hipLaunchKernelGGL(k_mrr_mu_shift, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st, ed, (const uint32_t *)ztd, ld, (int)n, k, (const double *)vecd);
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // out (n x k) = a panel effect's X b plus the staged k-vector, for every row
  int panel_hat(int e, double *out) {
    const MrrLeg &L = eff[(size_t)e].leg;
    const PanelData *D = L.P->data;
    const int nch = (int)std::min<int64_t>(64, L.p);       // marker chunks
    const int64_t cpc = (L.p + nch - 1) / nch;
    hipLaunchKernelGGL(k_mrr_hat_part, dim3((unsigned)((ld + 255) / 256), nch), dim3(256), 0, st, (const int8_t *)D->X, D->plan.R, L.p, ld, (int)n, k, (const double *)L.bd, cpc, hpart);
    hipLaunchKernelGGL(k_mrr_hat_finish, dim3((unsigned)std::min<int64_t>((n * k + 255) / 256, 4096)), dim3(256), 0, st, (const double *)hpart, nch, ld, (int)n, k,
                       (const double *)vecd, out);
    return BWGR_OK;
  }
  // hatd += the effect's share (a panel's with the staged k-vector, which the summing fits leave zero)
  int add_effect_hat(int e) {
    const MtEffect &E = eff[(size_t)e];
    if (E.panel) {
      CHK(panel_hat(e, htmp));
      hipLaunchKernelGGL(k_pegs_add, dim3((unsigned)std::min<int64_t>((n * k + 255) / 256, 4096)), dim3(256), 0, st, hatd, (const double *)htmp, (int64_t)n * k);
    } else if (E.sparse) {
      hipLaunchKernelGGL(k_pegs_sparse_hat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const int64_t *)E.sp.rowptr, (const int32_t *)E.sp.colidx,
                         (const double *)E.sp.rval, n, k, (const double *)E.sp.bd, hatd);
    } else {
      hipLaunchKernelGGL(k_pegs_zb, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const double *)E.dense.Zd, n, E.m, k, (const double *)E.dense.bd, hatd);
    }
    HIPCHK(hipGetLastError());
    return BWGR_OK;
  }
  // the effect's coefficients as an m x k column-major matrix
  int read_b(int e, double *out) {
    const int64_t m = eff[(size_t)e].m;
    std::vector<double> bh((size_t)m * k);
    HIPCHK(d2h(st, bh.data(), eff[(size_t)e].b(), sizeof(double) * m * k));
    for (int t = 0; t < k; ++t) for (int64_t j = 0; j < m; ++j) out[(size_t)t * m + j] = bh[(size_t)j * k + t];
    return BWGR_OK;
  }
};
